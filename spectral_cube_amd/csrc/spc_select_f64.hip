// spc_select_f64.hip - order statistics of float64 rays along the spectral axis (gfx950): spc_percentile_axis0_f64,
// spc_sigma_clip_axis0_f64.
//
// The reference's median / percentile / mad_std (dask_spectral_cube.py:657-731) and sigma_clip_spectrally (:851-878,
// centre = median | mean, spread = std | mad_std) on the float64 samples as they are, rays of up to 4096 samples
// (spc_select.hip is the float32 twin).  Three forms, chosen by sort64_launch (SPC_SELECT64 = 1, read once per process, keeps
// the keys in LDS for every length):
// rays of up to 1024 samples keep their keys in registers and meet over DPP row rotations (a radix select; the clip loop
// with spread = std runs on the same resident keys); longer rays select a key byte at a time from keys in LDS; the clip
// loop of longer rays, and of spread = mad_std, reads a bitonic-sorted ray.  The selections give the sorted rays' order
// statistics (numpy's `_lerp` of the same two samples) bit for bit.
#include "spc_wide.h"

#include <algorithm>
#include <type_traits>

namespace {

// The sorted form (round 5; today only the clip loop of rays the register form does not take): a block sorts
// its TS = 4096 / NZP adjacent rays (order-preserving 64-bit keys, excluded / NaN samples last) in 32 KB of LDS with a bitonic
// network, then one lane per ray runs the clip loop on the sorted ray - its order statistics directly (numpy's linear rule,
// its `_lerp` form), the loop as a shrinking window [a, b) of the sorted samples (clipping removes the two ends of a sorted ray;
// mean and std of a window are two scans of it, nanstd's two-pass form).  The clipped cube is written in a last sweep over the
// rays: a sample survives when its key lies between the window's end keys.
constexpr int kSortKeys = 4096;          // 32 KB of keys per block: four or five blocks per CU (16384 keys, one block: 41 ms per 5e8 voxels;
                                         // 8192: 21.8; 4096: 14.7 - the network's barriers and LDS round trips want other blocks to run beside them)
constexpr unsigned long long kExcl = ~0ull;
__device__ __forceinline__ unsigned long long fkey64(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double funkey64(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
struct Sort64Args {
    Cube64 c;
    MaskDev64 m;
    int nzp, ts;                 // padded ray length (power of two), rays per block
    double q, scale;
    const double* center;        // NULL, or (ny, nx): keys of |x - center|
    double* out;                 // percentile: (ny, nx); sigma clip: (nz, ny, nx) C-contiguous
    double lo_s, hi_s;
    int maxiters, cen_mean, spread_mad;
};
__global__ __launch_bounds__(256) void sort64_kernel(const Sort64Args A) {
    __shared__ unsigned long long keys[kSortKeys];           // [sample][ray]: consecutive lanes = consecutive rays
    __shared__ unsigned long long s_wlo[64], s_whi[64];
    const int t = threadIdx.x, TS = A.ts, NZP = A.nzp, L = 256 / TS;
    const int64_t tiles_x = (A.c.nx + TS - 1) / TS;
    const int64_t y = blockIdx.x / tiles_x, x0 = (blockIdx.x % tiles_x) * TS;
    const int r = t % TS, jz = t / TS;
    const bool col_in = x0 + r < A.c.nx;
    const double cen = (A.center && col_in) ? A.center[y * A.c.nx + x0 + r] : 0.0;
    {   // (eight samples requested together per lane, their channels clamped into the ray)
        constexpr int kIn = 8;
        const bool arr = (A.m.flags & SPC_MASK_ARRAY) != 0;
        const int64_t xc = col_in ? x0 + r : A.c.nx - 1;
        const double* pd = A.c.p + y * A.c.row_stride + xc;
        const uint8_t* pmk = arr ? A.m.arr + y * A.m.row_stride + xc : nullptr;
        for (int z0 = jz; z0 < NZP; z0 += L * kIn) {
            double vv[kIn];
            unsigned mk[kIn];
#pragma unroll
            for (int q = 0; q < kIn; ++q) {
                const int64_t zc = min((int64_t)(z0 + q * L), A.c.nz - 1);
                vv[q] = pd[zc * A.c.plane_stride];
                mk[q] = arr ? pmk[zc * A.m.plane_stride] : 1u;
            }
#pragma unroll
            for (int q = 0; q < kIn; ++q) {
                const int z = z0 + q * L;
                if (z < NZP) {
                    double v = vv[q];
                    bool ok = col_in && z < A.c.nz && spc_pred_valid(A.m, v) && mk[q] != 0u;
                    if (A.center) { v = fabs(v - cen); ok = ok && (v == v); }
                    keys[z * TS + r] = ok ? fkey64(v) : kExcl;
                }
            }
        }
    }
    __syncthreads();
    const int half = (TS * NZP) >> 1;
    for (int k = 2; k <= NZP; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int idx = t; idx < half; idx += 256) {
                const int ray = idx % TS, p = idx / TS;
                const int i = ((p / j) * 2 * j) + (p % j), l = i + j;
                const bool up = (i & k) == 0;
                const unsigned long long a = keys[i * TS + ray], b = keys[l * TS + ray];
                if ((a > b) == up) { keys[i * TS + ray] = b; keys[l * TS + ray] = a; }
            }
            __syncthreads();
        }
    }
    if (t < TS && x0 + t < A.c.nx) {
        const int ray = t;
        int lo = 0, hi = NZP;                                  // n = number of keys below the excluded one
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid * TS + ray] == kExcl) hi = mid; else lo = mid + 1; }
        const int n = lo;
        auto val = [&](int i) { return funkey64(keys[i * TS + ray]); };
        auto quantile = [&](int a, int cnt, double q) {        // numpy: virtual index q / 100 (cnt - 1), _lerp between its neighbours
            if (q == 50.0) {
                const int m = a + (cnt - 1) / 2;
                return (cnt & 1) ? val(m) : 0.5 * (val(m) + val(m + 1));
            }
            const double vi = q / 100.0 * (double)(cnt - 1);
            int p = (int)floor(vi);
            p = min(max(p, 0), cnt - 1);
            const int p1 = min(p + 1, cnt - 1);
            const double g = vi - (double)p, va = val(a + p), vb = val(a + p1), d = vb - va;
            return g >= 0.5 ? __dsub_rn(vb, __dmul_rn(d, 1.0 - g)) : __dadd_rn(va, __dmul_rn(d, g));   // (numpy's _lerp: a product, then a sum - never one fused operation)
        };
        // median of |x - med| over the window: the deviations below and above the median are two ascending sequences (walking
        // away from it) - their merge is walked up to the middle ranks
        auto mad = [&](int a, int cnt, double med) {
            int lo = a, hi = a + cnt;                          // first entry above the median
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (val(mid) > med) hi = mid; else lo = mid + 1; }
            int i = lo - 1, j = lo;                            // i walks down (<= med), j walks up (> med)
            const int r1 = (cnt - 1) / 2, r2 = cnt / 2;
            double d1 = 0.0, d2 = 0.0;
            for (int rank = 0; rank <= r2; ++rank) {
                const double dl = i >= a ? med - val(i) : INFINITY, dh = j < a + cnt ? val(j) - med : INFINITY;
                double d;
                if (dl <= dh) { d = dl; --i; } else { d = dh; ++j; }
                if (rank == r1) d1 = d;
                if (rank == r2) d2 = d;
            }
            return (cnt & 1) ? d1 : 0.5 * (d1 + d2);
        };
        int a = 0, b = n, it = 0;
        while (b > a && (A.maxiters < 0 || it < A.maxiters)) {
            ++it;
            const int cnt = b - a;
            double sum = 0.0;
            for (int i = a; i < b; ++i) sum += val(i);
            const double mean = sum / (double)cnt;
            double ss = 0.0;
            for (int i = a; i < b; ++i) { const double dv = val(i) - mean; ss = fma(dv, dv, ss); }
            const double medw = quantile(a, cnt, 50.0);
            const double sd = A.spread_mad ? 1.482602218505602 * mad(a, cnt, medw) : sqrt(ss / (double)cnt);
            const double c = A.cen_mean ? mean : medw;
            const double lob = c - A.lo_s * sd, hib = c + A.hi_s * sd;
            int na = a, nb = b;
            while (na < nb && val(na) < lob) ++na;
            while (nb > na && val(nb - 1) > hib) --nb;
            // (a NaN bound - an infinite sample in the window - clips nothing: the comparisons are false, as numpy's)
            if (na == a && nb == b) break;
            a = na; b = nb;
        }
        s_wlo[ray] = b > a ? keys[a * TS + ray] : 1ull;      // empty window: lo > hi, nothing survives
        s_whi[ray] = b > a ? keys[(b - 1) * TS + ray] : 0ull;
    }
    __syncthreads();
    if (col_in) {
        const unsigned long long wlo = s_wlo[r], whi = s_whi[r];
        for (int z = jz; z < A.c.nz; z += L) {
            double v;
            const bool ok = inc64(A.c, A.m, z, y, x0 + r, v);
            const unsigned long long k = ok ? fkey64(v) : kExcl;
            A.out[((int64_t)z * A.c.ny + y) * A.c.nx + x0 + r] = (k >= wlo && k <= whi) ? v : NAN;
        }
    }
}

// Round 6: median / percentile / mad_std of float64 rays WITHOUT a sort.  The bitonic network moved ~720 bytes through LDS per
// sample (45 barrier-separated stages at 512 channels); here the keys of TS = min(16, 8192 / NZP) adjacent rays go to LDS once
// (64 KB: 128 contiguous bytes per plane and block at TS = 16) and the lower order statistic of numpy's rule is pinned down one
// key BYTE at a time: eight passes count, for every ray, the keys that share the bytes found so far by their next byte (LDS
// atomics on 16 x 128 packed 16-bit counters), 256 / TS threads per ray add the counters up and one of them walks to the bin
// that holds the rank.  A ninth pass gives the number of keys <= the one found and the smallest key above it: the upper order
// statistic is one or the other.  The results are the sorted rays' - numpy's `_lerp` of the same two samples - bit for bit.
constexpr int kSelKeys64 = 8192, kSelRays64 = 16;
__global__ __launch_bounds__(256) void select64_kernel(const Sort64Args A) {
    __shared__ unsigned long long keys[kSelKeys64];          // [sample][ray]
    __shared__ unsigned hist[kSelRays64 * 128];              // [ray][bin & 127]: low half = bins 0 .. 127, high half = bins 128 .. 255
    __shared__ unsigned s_part[256];                         // [ray][thread of the ray]
    __shared__ unsigned long long s_prefix[kSelRays64], s_next[kSelRays64];
    __shared__ int s_rank[kSelRays64], s_n[kSelRays64], s_le[kSelRays64];
    const int t = threadIdx.x, TS = A.ts, NZP = A.nzp, L = 256 / TS;
    const int64_t tiles_x = (A.c.nx + TS - 1) / TS;
    const int64_t y = blockIdx.x / tiles_x, x0 = (blockIdx.x % tiles_x) * TS;
    const int r = t % TS, jz = t / TS;
    const bool col_in = x0 + r < A.c.nx;
    const double cen = (A.center && col_in) ? A.center[y * A.c.nx + x0 + r] : 0.0;
    {   // (eight samples requested together per lane, their channels clamped into the ray)
        constexpr int kIn = 8;
        const bool arr = (A.m.flags & SPC_MASK_ARRAY) != 0;
        const int64_t xc = col_in ? x0 + r : A.c.nx - 1;
        const double* pd = A.c.p + y * A.c.row_stride + xc;
        const uint8_t* pmk = arr ? A.m.arr + y * A.m.row_stride + xc : nullptr;
        for (int z0 = jz; z0 < NZP; z0 += L * kIn) {
            double vv[kIn];
            unsigned mk[kIn];
#pragma unroll
            for (int q = 0; q < kIn; ++q) {
                const int64_t zc = min((int64_t)(z0 + q * L), A.c.nz - 1);
                vv[q] = pd[zc * A.c.plane_stride];
                mk[q] = arr ? pmk[zc * A.m.plane_stride] : 1u;
            }
#pragma unroll
            for (int q = 0; q < kIn; ++q) {
                const int z = z0 + q * L;
                if (z < NZP) {
                    double v = vv[q];
                    bool ok = col_in && z < A.c.nz && spc_pred_valid(A.m, v) && mk[q] != 0u;
                    if (A.center) { v = fabs(v - cen); ok = ok && (v == v); }
                    keys[z * TS + r] = ok ? fkey64(v) : kExcl;
                }
            }
        }
    }
    if (t < TS) { s_prefix[t] = 0ull; s_rank[t] = 0; s_n[t] = 0; s_le[t] = 0; s_next[t] = kExcl; }
    const int nkeys = TS * NZP;
    const int ray_s = t / L, l = t % L;                        // scan: L threads per ray, TS bins each
    for (int d = 7; d >= 0; --d) {
        const int shift = 8 * d;
        for (int i = t; i < TS * 128; i += 256) hist[i] = 0u;
        __syncthreads();
        for (int i = t; i < nkeys; i += 256) {
            const unsigned long long k = keys[i];
            const int ray = i % TS;
            // (the bytes above the current one: equal to the prefix found so far; d = 7: every key but the excluded ones)
            const bool match = k != kExcl && (d == 7 || (k >> (shift + 8)) == (s_prefix[ray] >> (shift + 8)));
            if (match) {
                const unsigned b = (unsigned)(k >> shift) & 255u;
                atomicAdd(&hist[ray * 128 + (b & 127u)], (b & 128u) ? 65536u : 1u);
            }
        }
        __syncthreads();
        {   // bins [l TS, (l + 1) TS) of ray ray_s: all in one half of the packed counters
            unsigned sum = 0;
            const int b0 = l * TS;
            for (int b = b0; b < b0 + TS; ++b) { const unsigned w = hist[ray_s * 128 + (b & 127)]; sum += (b & 128) ? (w >> 16) : (w & 0xffffu); }
            s_part[ray_s * L + l] = sum;
        }
        __syncthreads();
        if (l == 0) {
            int rank = s_rank[ray_s];
            if (d == 7) {                                      // the ray's count, and the rank of the lower order statistic
                int n = 0;
                for (int g = 0; g < L; ++g) n += (int)s_part[ray_s * L + g];
                s_n[ray_s] = n;
                if (A.q == 50.0) rank = (n - 1) / 2;
                else { rank = (int)floor(A.q / 100.0 * (double)(n - 1)); rank = min(max(rank, 0), n - 1); }
                if (n <= 0) rank = 0;
            }
            int g = 0;
            while (g < L - 1 && rank >= (int)s_part[ray_s * L + g]) { rank -= (int)s_part[ray_s * L + g]; ++g; }
            int b = g * TS;
            for (;;) {
                const unsigned w = hist[ray_s * 128 + (b & 127)];
                const int c = (int)((b & 128) ? (w >> 16) : (w & 0xffffu));
                if (rank < c || b == g * TS + TS - 1) break;
                rank -= c; ++b;
            }
            s_rank[ray_s] = rank;
            s_prefix[ray_s] |= (unsigned long long)b << shift;
        }
        __syncthreads();
    }
    for (int i = t; i < nkeys; i += 256) {                      // keys <= the one found, and the smallest one above it
        const unsigned long long k = keys[i];
        const int ray = i % TS;
        if (k != kExcl) {
            if (k <= s_prefix[ray]) atomicAdd(&s_le[ray], 1);
            else atomicMin(&s_next[ray], k);
        }
    }
    __syncthreads();
    if (t < TS && x0 + t < A.c.nx) {
        const int n = s_n[t];
        double res = NAN;
        if (n > 0) {
            const unsigned long long klo = s_prefix[t];
            int p;
            double g = 0.0;
            if (A.q == 50.0) { p = (n - 1) / 2; g = (n & 1) ? 0.0 : 0.5; }
            else { const double vi = A.q / 100.0 * (double)(n - 1); p = min(max((int)floor(vi), 0), n - 1); g = vi - (double)p; }
            const int p1 = min(p + 1, n - 1);
            const unsigned long long khi = (p1 == p || p1 < s_le[t]) ? klo : s_next[t];
            const double va = funkey64(klo), vb = funkey64(khi);
            if (A.q == 50.0) res = (n & 1) ? va : 0.5 * (va + vb);
            else { const double d = vb - va; res = g >= 0.5 ? __dsub_rn(vb, __dmul_rn(d, 1.0 - g)) : __dadd_rn(va, __dmul_rn(d, g)); }   // (numpy's _lerp, unfused)
        }
        A.out[y * A.c.nx + x0 + t] = res * A.scale;
    }
}

// Rays of up to 1024 samples: the keys stay in REGISTERS (round 6, second form).  A block = 16 adjacent rays (128 contiguous
// bytes per plane), a wave = 4 of them, and the 16 lanes that share a ray are ONE DPP row (lane = 16 ray + slice, slice s holds
// the samples z = s + 16 i): whatever the lanes of a ray have to agree on - the sixteen counters of a digit pass, the count of
// keys below the one found, the smallest key above it - meets through four row rotations (v_add / v_min with row_ror 8, 4, 2, 1),
// with no LDS, no barrier, no atomics; every wave runs on its own.  Radix 16: sixteen passes over the KPL key registers of a
// lane (a bit-field extract, a prefix compare on the word that holds the digit, 8-bit counters in four packed words), after
// which every lane of the row walks the sixteen totals to the digit.
template <int N> struct U32Arr { unsigned v[N]; };
__device__ __forceinline__ unsigned row_ror_u32(unsigned v, int n) {       // lane i of a row of 16 takes lane (i + n) mod 16 ... of its row
    switch (n) {
        case 8: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);
        case 4: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false);
        case 2: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xf, 0xf, false);
        default: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xf, 0xf, false);
    }
}
__device__ __forceinline__ unsigned swap16_u32(unsigned v) {           // lane i takes lane i ^ 16 (ds_swizzle, bit mode: and 0x1f, xor 0x10)
    return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, 0x401f);
}
// LPR = 16 | 32 lanes per ray: one DPP row, or two neighbouring rows of the same wave (rays of 513 .. 1024 samples: 64 keys per lane
// do not fit the registers)
template <int LPR>
__device__ __forceinline__ unsigned row_sum_u32(unsigned v) {
    v += row_ror_u32(v, 8); v += row_ror_u32(v, 4); v += row_ror_u32(v, 2); v += row_ror_u32(v, 1);
    if (LPR == 32) v += swap16_u32(v);
    return v;
}
template <int LPR>
__device__ __forceinline__ unsigned long long row_min_u64(unsigned long long v) {
#pragma unroll
    for (int n = 8; n >= 1; n >>= 1) {
        const unsigned lo = row_ror_u32((unsigned)v, n), hi = row_ror_u32((unsigned)(v >> 32), n);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o < v ? o : v;
    }
    if (LPR == 32) {
        const unsigned long long o = ((unsigned long long)swap16_u32((unsigned)(v >> 32)) << 32) | swap16_u32((unsigned)v);
        v = o < v ? o : v;
    }
    return v;
}
// the one read of the cube: lane (ray, slice s) takes the samples z = s + LPR i of its ray as order-preserving keys (hi / lo words);
// excluded, NaN and out-of-range samples become the all-ones key, which no valid sample maps to and which sorts last
template <int KPL, int LPR>
__device__ __forceinline__ void row_load_keys(const Sort64Args& A, int64_t y, int64_t xc, bool col_in, int sl, double cen,
                                              unsigned (&khi)[KPL], unsigned (&klo)[KPL]) {
    const bool arr = (A.m.flags & SPC_MASK_ARRAY) != 0;
    const double* pd = A.c.p + y * A.c.row_stride + xc;
    const uint8_t* pmk = arr ? A.m.arr + y * A.m.row_stride + xc : nullptr;
    constexpr int CH = KPL < 16 ? KPL : 16;                  // samples requested together per lane (all 64 at once: 128 registers of loads in flight)
#pragma unroll
    for (int i0 = 0; i0 < KPL; i0 += CH) {
        double vv[CH];
        unsigned mk[CH];
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            const int64_t zc = min((int64_t)(sl + LPR * (i0 + q)), A.c.nz - 1);
            vv[q] = pd[zc * A.c.plane_stride];
            mk[q] = arr ? pmk[zc * A.m.plane_stride] : 1u;
        }
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            const int i = i0 + q;
            double v = vv[q];
            bool ok = col_in && (sl + LPR * i) < A.c.nz && spc_pred_valid(A.m, v) && mk[q] != 0u;
            if (A.center) { v = fabs(v - cen); ok = ok && (v == v); }
            const unsigned long long k = ok ? fkey64(v) : kExcl;
            khi[i] = (unsigned)(k >> 32); klo[i] = (unsigned)k;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// the key of 0-based rank `rank` (< n = the ray's valid keys) among the keys of the row's lanes: sixteen digit passes, HI selects
// the word the digit lies in (static per unrolled body, uniform per pass).  The excluded key - all ones - is counted like any
// other: it is the LARGEST key, so it never moves the bin that holds a rank below n (leaving its test out saves two of ten
// instructions per key and pass).  The descent stops as soon as every ray of the wave has ONE key left under its prefix
// (distinct samples: after nine or ten of the sixteen passes): that key is the smallest - the only - key of the row that
// matches the prefix.  All lanes of the wave call it (wave-uniform control flow); every lane of a row gets the row's key.
template <int KPL, int LPR>
__device__ __forceinline__ unsigned long long row_descend(const unsigned (&khi)[KPL], const unsigned (&klo)[KPL], int rank, int n) {
    int left = n;                                            // keys of the ray under the prefix found so far
    unsigned phi = 0u, plo = 0u;                             // the key's bits found so far
    auto pass = [&](auto hi_c, const int shift) {           // shift: bit offset of the digit inside its word
        constexpr bool HI = decltype(hi_c)::value;
        const unsigned above = shift >= 28 ? 0u : (0xffffffffu << (shift + 4));       // the bits of this word above the digit
        const unsigned pre = (HI ? phi : plo) & above;
        unsigned long long c4 = 0ull, ev = 0ull, od = 0ull;  // sixteen 4-bit counters; 8-bit counters of the even / odd bins
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const unsigned w = HI ? khi[i] : klo[i];
            bool m = (w & above) == pre;
            if (!HI) m = m && (khi[i] == phi);
            const unsigned b4 = __builtin_amdgcn_ubfe(w, (unsigned)shift, 4u) << 2;
            c4 += (unsigned long long)(m ? 1u : 0u) << b4;
            if ((i % 15) == 14 || i == KPL - 1) {            // a 4-bit counter holds 15
                ev += c4 & 0x0f0f0f0f0f0f0f0full;
                od += (c4 >> 4) & 0x0f0f0f0f0f0f0f0full;
                c4 = 0ull;
            }
        }
        // the ray's totals: 16-bit fields (<= 1024 keys per ray) summed over the row.  word[h][g] with h = even / odd bins,
        // g = 0 .. 3: fields (bits 0-15, bits 16-31) = 8-bit fields (f, f + 2) of the h-counters' word (g >> 1), f = g & 1
        unsigned tw[2][4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned long long src = h ? od : ev;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const unsigned word = (unsigned)(src >> (32 * (g >> 1)));
                tw[h][g] = row_sum_u32<LPR>((word >> (8 * (g & 1))) & 0x00ff00ffu);
            }
        }
        unsigned digit = 15u;
        bool found = false;
        left = 0;
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            // bin b = 8-bit field f = b >> 1 of the (b & 1)-counters: word f >> 2, field f & 3 = (f & 1) + 2 * ((f >> 1) & 1)
            const int f = b >> 1, g = 2 * (f >> 2) + (f & 1), half = (f >> 1) & 1;
            const int cb = (int)((tw[b & 1][g] >> (16 * half)) & 0xffffu);
            const bool here = !found && rank < cb;
            left = here ? cb : left;
            digit = here ? (unsigned)b : digit;
            rank = (found || here) ? rank : rank - cb;
            found = found || here;
        }
        if (HI) phi |= digit << shift; else plo |= digit << shift;
    };
    // The leading digits EVERY valid key of the ray shares need no pass (positive samples within a factor of a few share their sign,
    // exponent and then some: the bench's 1000 +- 1 shares five of the ten digits a descent otherwise walks): AND and OR of the
    // ray's keys differ where its keys do; the wave starts at the first digit that differs in ANY of its rays.
    int start = 0;
    {
        unsigned ah = 0xffffffffu, al = 0xffffffffu, oh = 0u, ol = 0u;
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const bool ex = (khi[i] & klo[i]) == 0xffffffffu;      // (the excluded key is all ones: neutral for AND, kept out of OR)
            ah &= khi[i]; al &= klo[i];
            oh |= ex ? 0u : khi[i]; ol |= ex ? 0u : klo[i];
        }
        ah &= row_ror_u32(ah, 8); al &= row_ror_u32(al, 8); oh |= row_ror_u32(oh, 8); ol |= row_ror_u32(ol, 8);
        ah &= row_ror_u32(ah, 4); al &= row_ror_u32(al, 4); oh |= row_ror_u32(oh, 4); ol |= row_ror_u32(ol, 4);
        ah &= row_ror_u32(ah, 2); al &= row_ror_u32(al, 2); oh |= row_ror_u32(oh, 2); ol |= row_ror_u32(ol, 2);
        ah &= row_ror_u32(ah, 1); al &= row_ror_u32(al, 1); oh |= row_ror_u32(oh, 1); ol |= row_ror_u32(ol, 1);
        if (LPR == 32) { ah &= swap16_u32(ah); al &= swap16_u32(al); oh |= swap16_u32(oh); ol |= swap16_u32(ol); }
        const unsigned dh = ah ^ oh, dl = al ^ ol;
        int shared = dh ? (__builtin_clz(dh) >> 2) : 8 + (dl ? (__builtin_clz(dl) >> 2) : 8);
        if (n <= 1) shared = 16;                             // nothing to tell apart: this ray holds nobody back
        start = min(__builtin_amdgcn_readlane(shared, 0), __builtin_amdgcn_readlane(shared, 32));
        if (LPR == 16) start = min(start, min(__builtin_amdgcn_readlane(shared, 16), __builtin_amdgcn_readlane(shared, 48)));
        if (start >= 16) return ((unsigned long long)ah << 32) | al;     // every ray of the wave: one distinct key (or none)
        phi = start >= 8 ? ah : (start > 0 ? (ah & (0xffffffffu << (32 - 4 * start))) : 0u);
        plo = start > 8 ? (al & (0xffffffffu << (64 - 4 * start))) : 0u;
    }
    int stop_hi = -1, stop_lo = -1;                          // the shift of the last pass made in either word (-1: none)
    for (int shift = 28 - 4 * start; shift >= 0; shift -= 4) {          // (start >= 8: no pass in the high word)
        pass(std::integral_constant<bool, true>{}, shift);
        stop_hi = shift;
        if (__all(left <= 1)) break;
    }
    if (start >= 8 || !__all(left <= 1)) {
        for (int shift = start > 8 ? 28 - 4 * (start - 8) : 28; shift >= 0; shift -= 4) {
            pass(std::integral_constant<bool, false>{}, shift);
            stop_lo = shift;
            if (__all(left <= 1)) break;
        }
    }
    if (stop_lo != 0) {                                      // stopped early: pick the one key that is left up
        const unsigned mh = stop_lo >= 0 ? 0xffffffffu : (0xffffffffu << stop_hi);
        const unsigned ml = stop_lo >= 0 ? (0xffffffffu << stop_lo) : 0u;
        unsigned long long cand = kExcl;
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const bool mt = ((khi[i] & mh) == phi) && ((klo[i] & ml) == plo);
            const unsigned long long k = ((unsigned long long)khi[i] << 32) | klo[i];
            cand = (mt && k < cand) ? k : cand;
        }
        cand = row_min_u64<LPR>(cand);
        if (left == 1) { phi = (unsigned)(cand >> 32); plo = (unsigned)cand; }   // (a ray with duplicates left ran all sixteen passes)
    }
    return ((unsigned long long)phi << 32) | plo;
}

// keys <= the one found, and the smallest key above it (the upper order statistic of numpy's rule is one or the other)
template <int KPL, int LPR>
__device__ __forceinline__ void row_le_next(const unsigned (&khi)[KPL], const unsigned (&klo)[KPL], unsigned long long kfound,
                                            unsigned& le, unsigned long long& nxt) {
    unsigned l = 0;
    unsigned long long nx = kExcl;
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
        const unsigned long long k = ((unsigned long long)khi[i] << 32) | klo[i];
        l += (k <= kfound) ? 1u : 0u;
        nx = (k > kfound && k < nx) ? k : nx;
    }
    le = row_sum_u32<LPR>(l);
    nxt = row_min_u64<LPR>(nx);
}
template <int KPL, int LPR>
__device__ __forceinline__ int row_count_valid(const unsigned (&khi)[KPL], const unsigned (&klo)[KPL]) {
    unsigned nloc = 0;
#pragma unroll
    for (int i = 0; i < KPL; ++i) nloc += ((khi[i] & klo[i]) != 0xffffffffu) ? 1u : 0u;      // (valid keys never are all ones)
    return (int)row_sum_u32<LPR>(nloc);
}

template <int KPL, int LPR>
__global__ __launch_bounds__(16 * LPR) void select64_reg_kernel(const Sort64Args A) {
    constexpr int RW = 64 / LPR;                             // rays per wave
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, rr = lane / LPR, sl = lane % LPR;
    const int64_t tiles_x = (A.c.nx + 15) / 16;
    const int64_t y = blockIdx.x / tiles_x, x0 = (blockIdx.x % tiles_x) * 16;
    const int64_t x = x0 + RW * wave + rr;
    const bool col_in = x < A.c.nx;
    const int64_t xc = col_in ? x : A.c.nx - 1;
    const double cen = A.center ? A.center[y * A.c.nx + xc] : 0.0;
    unsigned khi[KPL], klo[KPL];
    row_load_keys<KPL, LPR>(A, y, xc, col_in, sl, cen, khi, klo);
    // valid samples of the ray, and the rank of the lower order statistic (numpy's rule)
    const int n = row_count_valid<KPL, LPR>(khi, klo);
    int p = 0;
    double g = 0.0;
    if (A.q == 50.0) { p = (n - 1) / 2; g = (n & 1) ? 0.0 : 0.5; }
    else { const double vi = A.q / 100.0 * (double)(n - 1); p = min(max((int)floor(vi), 0), max(n - 1, 0)); g = vi - (double)p; }
    if (n <= 0) p = 0;
    const unsigned long long kfound = row_descend<KPL, LPR>(khi, klo, p, n);
    unsigned le;
    unsigned long long nxt;
    row_le_next<KPL, LPR>(khi, klo, kfound, le, nxt);
    if (sl == 0 && col_in) {
        double res = NAN;
        if (n > 0) {
            const int p1 = min(p + 1, n - 1);
            const unsigned long long kh = (p1 == p || p1 < (int)le) ? kfound : nxt;
            const double va = funkey64(kfound), vb = funkey64(kh);
            if (A.q == 50.0) res = (n & 1) ? va : 0.5 * (va + vb);
            else { const double d = vb - va; res = g >= 0.5 ? __dsub_rn(vb, __dmul_rn(d, 1.0 - g)) : __dadd_rn(va, __dmul_rn(d, g)); }
        }
        A.out[y * A.c.nx + x] = res * A.scale;
    }
}

// sigma_clip_spectrally on the same resident keys (centre = median | mean, spread = std): an iteration is the window's count, its
// mean and its sum of squared deviations (float64 lane partials added over the row in a fixed order: the result does not depend
// on scheduling), the median by row_descend, astropy's bounds; a clipped sample's key becomes the excluded key.  A wave iterates
// until none of ITS rays changes (a converged ray recomputes the same bounds and clips nothing) or maxiters is reached.
template <int LPR>
__device__ __forceinline__ double row_sum_f64(double v) {
#pragma unroll
    for (int n = 8; n >= 1; n >>= 1) {
        const unsigned long long u = (unsigned long long)__double_as_longlong(v);
        const unsigned lo = row_ror_u32((unsigned)u, n), hi = row_ror_u32((unsigned)(u >> 32), n);
        v += __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    }
    if (LPR == 32) {
        const unsigned long long u = (unsigned long long)__double_as_longlong(v);
        v += __longlong_as_double((long long)(((unsigned long long)swap16_u32((unsigned)(u >> 32)) << 32) | swap16_u32((unsigned)u)));
    }
    return v;
}
template <int KPL, int LPR>
__global__ __launch_bounds__(16 * LPR) void sigma_clip64_reg_kernel(const Sort64Args A) {
    constexpr int RW = 64 / LPR;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, rr = lane / LPR, sl = lane % LPR;
    const int64_t tiles_x = (A.c.nx + 15) / 16;
    const int64_t y = blockIdx.x / tiles_x, x0 = (blockIdx.x % tiles_x) * 16;
    const int64_t x = x0 + RW * wave + rr;
    const bool col_in = x < A.c.nx;
    const int64_t xc = col_in ? x : A.c.nx - 1;
    unsigned khi[KPL], klo[KPL];
    row_load_keys<KPL, LPR>(A, y, xc, col_in, sl, 0.0, khi, klo);
    int it = 0;
    for (;;) {
        if (!(A.maxiters < 0 || it < A.maxiters)) break;     // (uniform)
        ++it;
        const int cnt = row_count_valid<KPL, LPR>(khi, klo);
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const unsigned long long k = ((unsigned long long)khi[i] << 32) | klo[i];
            sum += (k != kExcl) ? funkey64(k) : 0.0;
        }
        const double mean = row_sum_f64<LPR>(sum) / (double)cnt;
        double ss = 0.0;
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const unsigned long long k = ((unsigned long long)khi[i] << 32) | klo[i];
            const double dv = funkey64(k) - mean;
            ss = (k != kExcl) ? fma(dv, dv, ss) : ss;
        }
        const double sd = sqrt(row_sum_f64<LPR>(ss) / (double)cnt);
        double c = mean;
        if (!A.cen_mean) {                                   // (uniform)
            const int p = max((cnt - 1) / 2, 0);
            const unsigned long long kf = row_descend<KPL, LPR>(khi, klo, p, cnt);
            unsigned le;
            unsigned long long nxt;
            row_le_next<KPL, LPR>(khi, klo, kf, le, nxt);
            const unsigned long long kh = ((cnt & 1) || p + 1 < (int)le) ? kf : nxt;
            c = (cnt & 1) ? funkey64(kf) : 0.5 * (funkey64(kf) + funkey64(kh));
        }
        const double lob = c - A.lo_s * sd, hib = c + A.hi_s * sd;
        unsigned changed = 0;
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const unsigned long long k = ((unsigned long long)khi[i] << 32) | klo[i];
            const double v = funkey64(k);
            // (a NaN bound - an infinite sample in the window - clips nothing: the comparisons are false, as numpy's)
            const bool out = (k != kExcl) && (cnt > 0) && ((v < lob) || (v > hib));
            khi[i] = out ? 0xffffffffu : khi[i]; klo[i] = out ? 0xffffffffu : klo[i];
            changed |= out ? 1u : 0u;
        }
        if (!__any(changed != 0u)) break;                    // none of this wave's rays changed
    }
    if (col_in) {
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const int z = sl + LPR * i;
            if (z < A.c.nz) {
                const unsigned long long k = ((unsigned long long)khi[i] << 32) | klo[i];
                A.out[((int64_t)z * A.c.ny + y) * A.c.nx + x] = (k != kExcl) ? funkey64(k) : NAN;
            }
        }
    }
}

static int sort64_launch(Sort64Args& A, const spc_cube_f64* cube, bool clip, hipStream_t st) {
    if (cube->nz > 4096) {
        spc_set_error("rays of more than 4096 samples have no float64 order statistics (got %lld)", (long long)cube->nz);
        return SPC_ERR_UNSUPPORTED;
    }
    int nzp = 2;
    while (nzp < cube->nz) nzp <<= 1;
    // SPC_SELECT64, read once per process.  2, the default: rays of up to 1024 samples keep their keys in registers; 1: the keys
    // in LDS for every length.  The clip loop sorts wherever it does not take the register form.
    static const bool regs = spc_switch("SPC_SELECT64", 2) != 1;
    A.nzp = nzp; A.ts = clip ? std::min(64, kSortKeys / nzp) : std::min(kSelRays64, kSelKeys64 / nzp);
    const int64_t nb = ((cube->nx + A.ts - 1) / A.ts) * cube->ny;
    SPC_REQUIRE(nb < (1LL << 31), "map too large for one launch");
    // the register forms (not the clip loop with stdfunc = mad_std: a second descent over |x - median| - the sorted form below):
    // 16 rays per block, 16 lanes per ray with 8, 16 or 32 keys each, or - 513 .. 1024 samples - 32 lanes per ray with 32 keys each
    if (regs && cube->nz <= 1024 && !(clip && A.spread_mad)) {
        const int64_t nbr = ((cube->nx + 15) / 16) * cube->ny;
        SPC_REQUIRE(nbr < (1LL << 31), "map too large for one launch");
        const int kpl = (int)((cube->nz + 15) / 16);
        dim3 grid((unsigned)nbr);
        auto row = [&](auto kpl_c, auto lpr_c) {
            constexpr int KPL = decltype(kpl_c)::value, LPR = decltype(lpr_c)::value;
            if (clip) hipLaunchKernelGGL((sigma_clip64_reg_kernel<KPL, LPR>), grid, dim3(16 * LPR), 0, st, A);
            else hipLaunchKernelGGL((select64_reg_kernel<KPL, LPR>), grid, dim3(16 * LPR), 0, st, A);
        };
        using std::integral_constant;
        if (kpl <= 8) row(integral_constant<int, 8>{}, integral_constant<int, 16>{});
        else if (kpl <= 16) row(integral_constant<int, 16>{}, integral_constant<int, 16>{});
        else if (kpl <= 32) row(integral_constant<int, 32>{}, integral_constant<int, 16>{});
        else row(integral_constant<int, 32>{}, integral_constant<int, 32>{});
        SPC_LAUNCH_CHECK();
        return SPC_OK;
    }
    if (clip) hipLaunchKernelGGL(sort64_kernel, dim3((unsigned)nb), dim3(256), 0, st, A);
    else hipLaunchKernelGGL(select64_kernel, dim3((unsigned)nb), dim3(256), 0, st, A);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

}  // namespace

extern "C" {

int spc_percentile_axis0_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, double q,
                             const double* d_center, double scale, double* d_out) {
    Sort64Args A{};
    int rc = cube64_args(cube, mask, &A.c, &A.m, true);       // (rays along y: the view with the first two axes exchanged)
    if (rc) return rc;
    SPC_REQUIRE(d_out != nullptr, "d_out is NULL");
    SPC_REQUIRE(q >= 0.0 && q <= 100.0, "percentile must lie in [0, 100], got %g", q);
    SPC_DEVICE(device);
    A.q = q; A.scale = scale; A.center = d_center; A.out = d_out;
    return sort64_launch(A, cube, false, (hipStream_t)stream);
}

int spc_sigma_clip_axis0_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, double sigma_lower,
                             double sigma_upper, int maxiters, int center_is_mean, int spread_is_mad, double* d_out) {
    Sort64Args A{};
    int rc = cube64_args(cube, mask, &A.c, &A.m);
    if (rc) return rc;
    SPC_REQUIRE(d_out != nullptr, "d_out is NULL");
    SPC_DEVICE(device);
    A.lo_s = sigma_lower; A.hi_s = sigma_upper; A.maxiters = maxiters; A.cen_mean = center_is_mean; A.spread_mad = spread_is_mad; A.out = d_out;
    A.q = 50.0; A.scale = 1.0;
    return sort64_launch(A, cube, true, (hipStream_t)stream);
}

}  // extern "C"
