// spc_select_impl.h - what the float32 order-statistics units share (spc_select.hip, spc_select_global.hip,
// and through spc_sigma_clip_impl.h spc_sigma_clip.hip and spc_sigma_clip_mad.hip): the order-preserving key of a float, the one read of the cube that turns TS adjacent rays into
// register-resident keys (sel_load_keys), the radix-16 descent over those keys (ray_select, with its candidate ranking and
// its cache of earlier descents), the packing of sparse rays into LDS (sel_compact), and on the host the block shape for a
// ray length, the run-time-to-template hand-over the launch tables use, and the cube / mask set-up of an argument struct.
//
// Internal linkage throughout, as in spc_wide.h: every unit that includes this has its own copy, and a kernel's argument
// types stay unit-local.  Units that include it need -fno-vectorize -fno-slp-vectorize (Makefile: SELECT_UNITS).
#pragma once
#include "spc_common.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace {

// tuning constants of the register-resident kernels (sel_load_keys_impl, ray_select)
constexpr int kSelInflight = 8;          // loads in flight per lane, 256-thread blocks
constexpr int kSelInflightWide = 32;     // ... 512-thread blocks without a mask array
constexpr int kSelFirstVote = 1;         // first pass after which a descent asks whether every ray's bin is small enough to rank

// ---- host: launch tables -----------------------------------------------------------------------------------
// A run-time bool reaches a kernel's template argument as a std::bool_constant handed to a generic lambda; a table row names
// its integers as SelInt<N>{}.  The tables name the combinations that exist - they are not Cartesian.
template <int N> using SelInt = std::integral_constant<int, N>;
template <class F>
static inline void sel_with_bool(bool b, F&& f) {
    if (b) f(std::true_type{}); else f(std::false_type{});
}
// keys per lane for rays of nz samples shared by `lanes` lanes: 16, 32, 64, or 128 (8 spaxels per 256-thread block only)
static inline int sel_kpl(int64_t nz, int lanes) {
    const int need = (int)((nz + lanes - 1) / lanes);
    return need <= 16 ? 16 : (need <= 32 ? 32 : (need <= 64 ? 64 : 128));
}
// spaxels per 256-thread block: 32 up to 512 samples (8 lanes per ray), 16 up to 1024 (16 lanes), 8 up to 4096 (32 lanes)
static inline int sel_ts256(int64_t nz) { return nz <= 512 ? 32 : (nz <= 1024 ? 16 : 8); }

// ---- host: the leading members every argument struct of these units shares ----------------------------------
// (cube, nz, ny, nx, row_stride, plane_stride, mask) from a checked cube and its mask; WithKeys: also the key interval of
// the mask's predicate terms (key_min, key_span - sel_key_range below)
static inline void sel_key_range(uint32_t flags, float thr_lo, float thr_hi, uint32_t* kmin, uint32_t* span);
template <bool WithKeys, class Args>
static inline int sel_set_cube(Args* A, const spc_cube_f32* cube, const spc_mask* mask) {
    const int rc = spc_mask_to_dev(mask, cube, &A->mask);
    if (rc) return rc;
    if constexpr (WithKeys) sel_key_range(A->mask.flags, A->mask.thr_lo, A->mask.thr_hi, &A->key_min, &A->key_span);
    A->cube = cube->d_data;
    A->nz = cube->nz; A->ny = cube->ny; A->nx = cube->nx;
    A->row_stride = cube->row_stride; A->plane_stride = cube->plane_stride;
    return SPC_OK;
}

// Block -> tile order that keeps `g` neighbouring tiles of a row on ONE XCD (blocks go round the 8 XCDs by index): a tile
// of 16 spaxels is half a 128-byte line per plane, and the block holding the other half should find it in the same L2.
// (g = 16.  1024^3: the clip kernel's read + write floor 4.21 -> 3.28 ms, the 256-thread selection 2.97 -> 2.65 ms;
//  groups of 2 / 4 / 8: 3.95 / 3.54 / 3.32 - 3.6 ms; no effect on the 512-thread selection.  It rides in the kernel
//  arguments: as a constant in the kernels it cost several of them scalar registers - profiles/retired_switches_resources.txt)
constexpr int kXcdGroup = 16;
__device__ __forceinline__ int64_t sel_tile_of_block(int64_t bid, int64_t nblocks, int g) {
    if (g <= 1) return bid;
    const int64_t span = 8 * (int64_t)g, whole = nblocks / span * span;
    if (bid >= whole) return bid;
    const int64_t base = bid / span * span, r = bid - base;
    return base + (r % 8) * g + r / 8;
}

__device__ __forceinline__ uint32_t fkey(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float funkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

typedef float f32x4s __attribute__((ext_vector_type(4)));

// ---- rays resident in REGISTERS: ONE read of the cube (round 2) ------------------------------------------
// The streaming descents (spc_select.hip) read the cube once per digit (8 or 17 reads): 18.7 ms for a median at 1024^3, 3.6 % of the
// roofline of a single read.  Here a block owns TS adjacent spaxels (TS x 4 bytes contiguous per plane: 32- to
// 128-byte segments) and reads their rays ONCE: 256 / TS lanes share a ray, a lane turns its KPL = ceil(nz / lanes)
// <= 64 samples (z = j + lanes * i) into order-preserving keys (excluded / NaN samples become the largest key,
// which no valid float maps to) and keeps them in registers.  A digit pass of the radix-16 descent is then 7 VALU
// instructions per key: sixteen 4-bit counters in ONE 64-bit register (the digit picks the field: one shift, one
// add, no dynamic indexing, no atomics), emptied into 8-bit counters every 15 keys; the per-ray totals meet in a
// 16-counter LDS histogram (three rotating buffers: one barrier per digit) and every lane of the ray walks the
// sixteen totals to the digit.  LDS only carries the histograms (a few KB): the ~105 VGPRs set the occupancy
// (4 waves per SIMD).  The descent stops early: once four digits (16 bits) are known, the samples that still match
// are few (their number is the count of the selected bin); if no ray of the block has more than kCandMax of them,
// they are gathered into LDS and ranked directly (each lane of the ray ranks its share against all candidates)
// instead of four more passes over all keys.  Rays with many equal or near-equal samples (quantised data) take all
// eight passes.  The upper order statistic of an interpolated percentile is either the same value (ties) or the
// smallest key above the first: one more sweep over the registers.
// (A first version kept the keys in LDS - 64 KB per block, 2 waves per SIMD, an LDS read per key and pass: 6.25 ms
// where this one takes 2.5 - 3.2 ms.)
constexpr int kCandMax = 32;

// What a descent ranks: the resident keys themselves, or - for the MAD - the keys of |x - centre| formed on the fly
// from the resident keys (float32 subtraction like numpy's; the excluded key stays the largest)
struct KeyIdentity {
    __device__ __forceinline__ uint32_t operator()(uint32_t k) const { return k; }
};
struct KeyAbsDev {
    float center;
    __device__ __forceinline__ uint32_t operator()(uint32_t k) const {
        const float v = fabsf(funkey(k) - center);
        return (k != 0xffffffffu && v == v) ? fkey(v) : 0xffffffffu;
    }
};

template <int KPL, bool FIRST, class XF>
__device__ __forceinline__ void count_keys(const uint32_t (&key)[KPL], uint32_t prefix, int b, const XF& xf,
                                           unsigned long long& accE, unsigned long long& accO) {
    constexpr unsigned long long kNib = 0x0f0f0f0f0f0f0f0full;
    unsigned long long a = 0ull;
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
        const uint32_t ki = xf(key[i]);
        if (FIRST) {
            a += 1ull << ((ki >> 28) * 4u);
        } else {
            const uint32_t tt = (ki ^ prefix) >> b;              // < 16 exactly for the samples inside the prefix
            const unsigned long long one = (tt < 16u) ? 1ull : 0ull;
            a += one << ((tt * 4u) & 63u);
        }
        if (i % 15 == 14 || i == KPL - 1) {                      // a 4-bit field holds 15
            accE += a & kNib;
            accO += (a >> 4) & kNib;
            a = 0ull;
            __builtin_amdgcn_sched_barrier(0);                   // (keeps the scheduler from expanding all keys at once)
        }
    }
}

// ---- the one read of the cube: TS rays into register keys ------------------------------------------------
// Lane (r, j) takes samples z = j + L k (L = 256 / TS lanes per ray, k < KPL) of ray r; an excluded / NaN / out-of-range
// sample becomes the largest key.
//  * Validity is ONE unsigned range test on the key: NaN samples, isfinite and the threshold comparisons of the mask all
//    select an interval of the order-preserving key (sel_key_range on the host), so (key - kmin) < span replaces round 2's
//    five float compares and their scalar ANDs (35 - 40 issue slots per key with the addressing below - as much as the
//    four digit passes of the selection that follows).  A lane whose column lies beyond the image gets span 0.
//  * DESC: a key slot is addressed through a buffer descriptor whose base is advanced by L planes per slot in SCALAR
//    arithmetic; a lane's offset (its column and its first plane) is one 32-bit register shared by all its loads.  Slots
//    that can run past the last plane (only the upper half of the slots can, by the launcher's choice of KPL) send the
//    lanes beyond it to offset 0 of the last slot that exists - always inside the cube - and drop the sample by the
//    validity test.  The launcher picks DESC when L planes and TS columns stay below 2 GiB of byte offset
//    (sel_desc_fits); larger planes keep 64-bit per-lane addresses (clamped to the last plane).
// cen: select on |x - cen| when CEN (mad_std).
static inline bool sel_desc_fits(int ts, int64_t plane_stride, int64_t x_stride, int bt = 256) {
    const int64_t L = bt / ts;
    return (L * plane_stride + ts * x_stride) * 4 < (1ll << 31);
}
static inline uint32_t sel_host_key(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// mask predicate (isfinite, > >= < <= thresholds; NaN never valid) -> the keys it includes: [*kmin, *kmin + *span)
static inline void sel_key_range(uint32_t flags, float thr_lo, float thr_hi, uint32_t* kmin, uint32_t* span) {
    float lim, lo, hi;
    spc_canonical_pred(flags, thr_lo, thr_hi, &lim, &lo, &hi);              // |v| <= lim && !(v <= lo) && !(v >= hi)
    *kmin = 0u;
    *span = 0u;
    if (!(lim >= 0.f)) return;
    uint64_t a = sel_host_key(-lim), b = sel_host_key(lim);
    if (lo == lo) a = std::max<uint64_t>(a, (uint64_t)sel_host_key(lo == 0.f ? 0.f : lo) + 1u);      // v > lo; both zeros: > +0
    if (hi == hi) {
        const uint64_t h = sel_host_key(hi == 0.f ? -0.f : hi);                                     // v < hi; both zeros: < -0
        if (h == 0u) return;
        b = std::min<uint64_t>(b, h - 1u);
    }
    if (b < a) return;
    *kmin = (uint32_t)a;
    *span = (uint32_t)(b - a + 1u);
}

__device__ __forceinline__ uint32_t fkey_bits(uint32_t u) {
    return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}

template <int TS, int KPL, bool ARR, bool DESC, bool CEN, int BT>
__device__ __forceinline__ int sel_load_keys_impl(const float* cube, int64_t plane_stride, int64_t x_stride, int64_t tile_off,
                                                  const uint8_t* marr, int64_t m_plane_stride, int64_t m_x_stride, int64_t m_tile_off,
                                                  int rc, int j, int nz, bool col_in, uint32_t kmin, uint32_t span1,
                                                  float cen, uint32_t (&key)[KPL]) {
    constexpr int L = BT / TS;
    // loads in flight per lane: the raw samples land in the key registers themselves (converted in place), so a whole
    // group costs no registers beyond the mask bytes.  Round 2 / 3a kept 8 in flight (2 KB per wave, 40 KB per CU): the
    // load phase ran at 2.1 TB/s - latency-bound - and made up 2.0 of the kernel's 2.9 ms at 1024^3.
    // 512-thread blocks (round 4, tools/bench_select_bt.py at 1024^3): 16 / 32 / 64 in flight - no mask 1.95 / 1.87 / 1.93 ms against 2.00,
    // uint8 mask 2.18 / 2.33 ms against 2.24 (its bytes wait in registers of their own); the 256-thread table loses with more than 8.
    constexpr int kWant = BT == 512 ? (ARR ? 16 : kSelInflightWide) : kSelInflight;
    constexpr int U = KPL < kWant ? KPL : kWant;
    constexpr int kChk0 = (KPL == 16) ? 0 : KPL / 2;             // first slot that can run past the last plane
    int mine = 0;
    const uint32_t span_l = col_in ? span1 : 0u;
    const int last = (nz - 1) / L;                               // the last slot that holds a sample (uniform)
    // which of the slots kChk0 .. KPL - 1 hold a sample of THIS lane: a bit each (sign-extended bit extracts below - no
    // compare, no scalar mask per slot)
    const int nk = min(max((nz - j + L - 1) / L - kChk0, 0), KPL - kChk0);
    const unsigned long long vbits = nk >= 64 ? ~0ull : ((1ull << nk) - 1ull);
    const uint32_t vb0 = (uint32_t)vbits, vb1 = (uint32_t)(vbits >> 32);
    const unsigned voff = (unsigned)(((int64_t)rc * x_stride + (int64_t)j * plane_stride) * 4);
    const unsigned moff = ARR ? (unsigned)((int64_t)rc * m_x_stride + (int64_t)j * m_plane_stride) : 0u;
    const uint64_t step = (uint64_t)(L * plane_stride) * 4u, mstep = ARR ? (uint64_t)(L * m_plane_stride) : 0u;
    const char* kb = reinterpret_cast<const char*>(cube + tile_off);          // slot base (DESC), advanced in scalar arithmetic
    const char* mb = ARR ? reinterpret_cast<const char*>(marr + m_tile_off) : nullptr;
    const float* p = cube + tile_off + (int64_t)rc * x_stride;                 // (64-bit form)
    const uint8_t* pm = ARR ? marr + m_tile_off + (int64_t)rc * m_x_stride : nullptr;
#pragma unroll
    for (int i0 = 0; i0 < KPL; i0 += U) {
        unsigned mk[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u;
            const bool chk = i >= kChk0;
            // all ones when the slot holds a sample of this lane
            const uint32_t vmu = chk ? (uint32_t)__builtin_amdgcn_sbfe((int)((i - kChk0) < 32 ? vb0 : vb1), (i - kChk0) & 31, 1) : 0xffffffffu;
            if (DESC) {
                if (i > 0) {
                    const bool adv = !chk || (i <= last);
                    kb += adv ? step : 0u;
                    if (ARR) mb += adv ? mstep : 0u;
                }
                const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)kb, 0, (int)0xffffffffu, 0x00020000);
                key[i] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, (int)(voff & vmu), 0, /*nt*/ 2);
                if (ARR) {
                    const auto rm = __builtin_amdgcn_make_buffer_rsrc((void*)mb, 0, (int)0xffffffffu, 0x00020000);
                    mk[u] = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(rm, (int)(moff & vmu), 0, 2);
                } else {
                    mk[u] = 1u;
                }
            } else {
                const int z = chk ? min(j + L * i, nz - 1) : j + L * i;
                key[i] = __float_as_uint(__builtin_nontemporal_load(p + (int64_t)z * plane_stride));
                mk[u] = ARR ? pm[(int64_t)z * m_plane_stride] : 1u;
            }
        }
        __builtin_amdgcn_sched_barrier(0);                       // (all loads of the group first)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u;
            const uint32_t raw = key[i];
            uint32_t k = fkey_bits(raw);
            // (beyond the last plane: the excluded key fails the range test)
            if (i >= kChk0) k |= ~(uint32_t)__builtin_amdgcn_sbfe((int)((i - kChk0) < 32 ? vb0 : vb1), (i - kChk0) & 31, 1);
            bool ok = (k - kmin) < span_l;
            if (ARR) ok = ok && (mk[u] != 0u);
            if (CEN) {
                // (an infinite raw under "no isfinite" passes and |inf - cen| stays a valid key unless cen is the same
                //  infinity: that NaN sorts above +inf)
                k = __float_as_uint(fabsf(__uint_as_float(raw) - cen)) | 0x80000000u;
                ok = ok && (k <= 0xff800000u);
            }
            key[i] = ok ? k : 0xffffffffu;
            mine += ok ? 1 : 0;
        }
        __builtin_amdgcn_sched_barrier(0);                       // U loads in flight, not KPL
    }
    return mine;
}

template <int TS, int KPL, bool ARR, bool DESC, int BT = 256>
__device__ __forceinline__ int sel_load_keys(const float* cube, int64_t plane_stride, int64_t x_stride, int64_t tile_off,
                                             const uint8_t* marr, int64_t m_plane_stride, int64_t m_x_stride, int64_t m_tile_off,
                                             int rc, int j, int nz, bool col_in, uint32_t kmin, uint32_t span1,
                                             bool use_cen, float cen, uint32_t (&key)[KPL]) {
    // (block-uniform branch; the memory clobbers keep the compiler from hoisting the - identical - loads of both arms above
    //  the branch, where all KPL of them would be in flight at once and spill)
    if (use_cen) {
        asm volatile("; keys of |x - centre|" ::: "memory");
        return sel_load_keys_impl<TS, KPL, ARR, DESC, true, BT>(cube, plane_stride, x_stride, tile_off, marr, m_plane_stride, m_x_stride,
                                                            m_tile_off, rc, j, nz, col_in, kmin, span1, cen, key);
    }
    asm volatile("; keys of x" ::: "memory");
    return sel_load_keys_impl<TS, KPL, ARR, DESC, false, BT>(cube, plane_stride, x_stride, tile_off, marr, m_plane_stride, m_x_stride,
                                                         m_tile_off, rc, j, nz, col_in, kmin, span1, 0.f, key);
}

// LDS scratch of one block of TS rays
template <int TS>
struct SelShared {
    uint32_t hist[3][TS][16];
    uint32_t nvalid[TS], nextkey[TS], ncand[TS], sel_key[TS], sel_below[TS], sel_eq[TS], nlow[TS];
    uint32_t cand[TS][kCandMax];
    int level;                                                  // (SelCache: the pass a descent resumes after)
    int vote[8];                                                // "a ray's bin is too large to rank" after pass p / [7]: at the resume
    int narrow;                                                 // a ray keeps > 3/4 of its samples in one leading digit: no early votes
};

// The histograms an earlier descent over the SAME keys counted in its first four passes (4, 8, 12, 16 key bits), per ray, each with
// the prefix it was counted under.  A later descent for another rank (the clip loop: the median moves by a few ranks per iteration)
// walks them instead of counting - pass p's cached histogram serves as long as the new path's prefix above it is the one it was
// counted under, also when the new rank picks ANOTHER digit from it - and starts counting at the first pass whose cached
// histogram belongs to another bin (block-wide: the earliest of its rays' answers).  `prefix / below / eq / krel`: the walk's state
// after each pass, handed from the one lane per ray that walks to the others.
template <int TS>
struct SelCache {
    uint16_t hist[4][TS][16];
    uint32_t pre[4][TS];
    uint32_t prefix[4][TS], below[4][TS], eq[4][TS], krel[4][TS];
    int first_done;                                             // the pass after which the FIRST descent ranked its candidates (block-wide)
};

// every thread of the block: zero what a descent needs (followed by a barrier at the caller)
template <int TS, int BT = 256>
__device__ __forceinline__ void sel_reset(SelShared<TS>& S) {
    const int t = threadIdx.x;
    if (t < TS) { S.nvalid[t] = 0u; S.nextkey[t] = 0xffffffffu; S.ncand[t] = 0u; S.nlow[t] = 0u; }
    if (t == 0) S.level = 3;
    if (t < 8) S.vote[t] = 0;
    if (t == 8) S.narrow = 0;
    for (int i = t; i < 3 * TS * 16; i += BT) (&S.hist[0][0][0])[i] = 0u;
}

// 16 bits of the key known: few samples are left in the bin.  All rays of the block small enough -> rank them directly
// (k: rank inside the bin; on success prefix / below / eq describe the selected KEY).  Block-uniform result.
template <int TS, int KPL, int BT, class XF>
__device__ __forceinline__ bool sel_rank_candidates(SelShared<TS>& S, const uint32_t (&key)[KPL], const XF& xf, int r, int j, int n, int k,
                                                    uint32_t& prefix, int& below, int& eq, int cshift = 16, int cap = kCandMax, int slot = 7) {
    constexpr int kLanesPerRay = BT / TS;
    // the vote: one flag word per asking point of a descent (zeroed by sel_reset), one barrier
    if ((n > 0) & (eq > cap) & (j == 0)) S.vote[slot] = 1;
    __syncthreads();
    if (S.vote[slot] != 0) return false;
    if (n > 0) {
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const uint32_t ki = xf(key[i]);
            if (((ki ^ prefix) >> cshift) == 0u) {
                const uint32_t slot = atomicAdd(&S.ncand[r], 1u);
                S.cand[r][slot] = ki;
            }
        }
    }
    __syncthreads();
    if (n > 0) {
        for (int idx = j; idx < eq; idx += kLanesPerRay) {
            const uint32_t c = S.cand[r][idx];
            int less = 0, same_before = 0, same = 0;
            for (int m = 0; m < eq; ++m) {
                const uint32_t o = S.cand[r][m];
                less += (o < c) ? 1 : 0;
                same += (o == c) ? 1 : 0;
                same_before += (o == c && m < idx) ? 1 : 0;
            }
            if (less + same_before == k) { S.sel_key[r] = c; S.sel_below[r] = (uint32_t)(below + less); S.sel_eq[r] = (uint32_t)same; }
        }
    }
    __syncthreads();
    if (n > 0) { prefix = S.sel_key[r]; below = (int)S.sel_below[r]; eq = (int)S.sel_eq[r]; }
    return true;
}

// The descent over the registers of the block (all threads call it; barriers inside).  r / j: ray and slice of this
// lane, n: valid samples of the ray, rank0: samples of the key set that sort below them (the clip loop keeps its keys
// and moves a window over them).  Returns the keys of the two order statistics numpy's 'linear' percentile q
// interpolates between and the interpolation fraction.  S must have been reset (sel_reset + barrier).
// C: cache of this key set's descents (filled; consulted when `resume`, block-uniform), or nullptr.
template <int TS, int KPL, int BT = 256, class XF = KeyIdentity>
__device__ __forceinline__ void ray_select(SelShared<TS>& S, const uint32_t (&key)[KPL], const XF& xf, int r, int j, int n, double q,
                                           uint32_t& key_lo, uint32_t& key_hi, double& frac, int max_pass = 8, int rank0 = 0,
                                           SelCache<TS>* C = nullptr, bool resume = false, bool early = true) {
    const double pos = q / 100.0 * (double)(n > 0 ? n - 1 : 0);
    const double fl = floor(pos);
    int k = rank0 + (int)fl;                                     // rank still to be found inside the current prefix
    const int khi = rank0 + min((int)ceil(pos), max(n - 1, 0));
    frac = pos - fl;
    int below = 0;                                               // keys smaller than everything matching the prefix
    uint32_t prefix = 0u;
    int eq = 0;
    bool done = false;                                           // block-uniform
    int start = 0;
    if (C != nullptr && resume) {
        if (j == 0) {                                            // one lane per ray walks the cached histograms
            int lvl = 3;                                         // (rays without samples do not care)
            if (n > 0) {
                lvl = -1;
                uint32_t pf = 0u;
                int bl = 0, kk = k;
                bool live = true;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    live = live && (p == 0 || pf == C->pre[p][r]);
                    if (live) {
                        uint32_t dsel = 15u;
                        int e = 0;
                        bool found = false;
#pragma unroll
                        for (int d = 0; d < 16; ++d) {
                            const int c = (int)C->hist[p][r][d];
                            if (!found) {
                                if (kk < c) { dsel = d; found = true; e = c; }
                                else { kk -= c; bl += c; }
                            }
                        }
                        pf |= dsel << (28 - 4 * p);
                        C->prefix[p][r] = pf; C->below[p][r] = (uint32_t)bl; C->eq[p][r] = (uint32_t)e; C->krel[p][r] = (uint32_t)kk;
                        lvl = p;
                    }
                }
            }
            if (lvl < 3) atomicMin(&S.level, lvl);
        }
        __syncthreads();
        const int sl = S.level;
        if (sl >= 0) {
            prefix = C->prefix[sl][r];
            below = (int)C->below[sl][r];
            eq = (int)C->eq[sl][r];
            k = (int)C->krel[sl][r];
            start = sl + 1;
        }
    }
    // Ranking eq candidates costs a lane eq^2 / (lanes per ray) compares, a pass ~5 slots for each of its KPL keys: before 16 bits
    // are known the vote only passes where ranking is the cheaper of the two - 32 candidates with 16 lanes per ray, 11 with 2.
    constexpr int kL = BT / TS;
    constexpr int kEarlyCap = kL >= 16 ? 32 : (kL >= 8 ? 22 : (kL >= 4 ? 16 : 11));
    if (C != nullptr && !resume && j == 0) {
        // a first descent may stop before its fourth pass: what it does not count must not look like a cached histogram
        C->pre[1][r] = 0xffffffffu; C->pre[2][r] = 0xffffffffu; C->pre[3][r] = 0xffffffffu;
    }
    // A vote that fails costs a barrier: a resumed descent (the clip loop: the same keys, a window that moved by a few ranks) only asks
    // where the first descent of the block was answered - its bins are the same size give or take the clipped samples.
    const int vote_from = (C != nullptr && resume) ? min(C->first_done, 3) : (early ? kSelFirstVote : 3);     // block-uniform
    int done_pass = 3;
    // resumed with enough bits known: the candidates of the bin straight away when every ray's bin is small (no pass runs)
    if (start >= 2 && start - 1 >= vote_from)
        done = sel_rank_candidates<TS, KPL, BT>(S, key, xf, r, j, n, k, prefix, below, eq, 32 - 4 * start, start < 4 ? kEarlyCap : kCandMax);
#pragma unroll 1
    for (int pass = start; pass < max_pass && !done; ++pass) {
        const int b = 28 - 4 * pass;
        unsigned long long accE = 0ull, accO = 0ull;             // even / odd digits, 8 bits each (<= 64 keys per lane)
        // (the first pass has no prefix; `pass` is made opaque so that its digit extraction - which does not depend on
        // anything the loop changes - is not hoisted out of the loop and kept in 64 more registers)
        int popaque = pass;
        asm volatile("" : "+s"(popaque));
        if (popaque == 0) count_keys<KPL, true>(key, prefix, b, xf, accE, accO);
        else count_keys<KPL, false>(key, prefix, b, xf, accE, accO);
        uint32_t* h = S.hist[pass % 3][r];
        uint32_t* hz = S.hist[(pass + 1) % 3][r];
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const uint32_t c0 = (uint32_t)(accE >> (8 * d)) & 0xffu, c1 = (uint32_t)(accO >> (8 * d)) & 0xffu;
            if (c0) atomicAdd(&h[2 * d], c0);
            if (c1) atomicAdd(&h[2 * d + 1], c1);
        }
        if (j == 0) {
#pragma unroll
            for (int d = 0; d < 16; ++d) hz[d] = 0u;              // next pass's buffer (last read two passes ago)
        }
        __syncthreads();
        uint32_t dsel = 15u;
        bool found = false;
        const bool keep = C != nullptr && pass < 4 && j == 0;    // this pass's histogram and the prefix it was counted under
        if (keep) C->pre[pass][r] = prefix;
#pragma unroll
        for (int d = 0; d < 16; ++d) {
            const int c = (int)h[d];
            if (keep) C->hist[pass][r][d] = (uint16_t)c;
            if (!found) {
                if (k < c) { dsel = d; found = true; eq = c; }
                else { k -= c; below += c; }
            }
        }
        prefix |= dsel << b;
        // (a ray that keeps more than 3/4 of its samples in one leading digit - positive data, a narrow relative range - will not have
        //  a small bin two passes later: the early votes of the whole block are dropped.  Written here, read behind the next pass's
        //  barrier.)
        if (pass == 0 && j == 0 && n > 0 && 4 * eq > 3 * n) S.narrow = 1;
        // Few samples are left in the bin: rank its candidates directly when every ray's bin is small, and ask again after every
        // further pass (data in a narrow relative range share their leading bits: their bins get small two passes later).  Round 4:
        // asked from the second pass on - a failed vote costs one barrier, and samples around zero (baseline-subtracted spectra)
        // have few keys per binade near their median: 8 or 12 bits leave <= 32 (median 1024^3: 1.86 -> 1.64 ms).
        if (pass >= vote_from && pass < 7 && (pass >= 3 || S.narrow == 0)) {
            done = sel_rank_candidates<TS, KPL, BT>(S, key, xf, r, j, n, k, prefix, below, eq, 28 - 4 * pass, pass < 3 ? kEarlyCap : kCandMax, pass);
            if (done) done_pass = min(pass, 3);
        }
    }
    if (C != nullptr && !resume && threadIdx.x == 0) C->first_done = done_pass;
    // prefix = the key of rank floor(pos); `eq` samples carry it, `below` are smaller
    key_lo = prefix;
    key_hi = prefix;
    const bool need_next = (n > 0) && (khi >= below + eq);       // ray-uniform
    if (__syncthreads_or(need_next ? 1 : 0)) {
        if (need_next) {
            uint32_t mn = 0xffffffffu;
#pragma unroll
            for (int i = 0; i < KPL; ++i) { const uint32_t ki = xf(key[i]); mn = (ki > prefix) ? min(mn, ki) : mn; }
            atomicMin(&S.nextkey[r], mn);
        }
        __syncthreads();
        if (need_next) key_hi = S.nextkey[r];
    }
}

// numpy's interpolation between the two order statistics (the mean of two for a median), in float64, rounded once
__device__ __forceinline__ float sel_value(uint32_t key_lo, uint32_t key_hi, double frac, double scale, bool median = true) {
    const double a = (double)funkey(key_lo), bb = (double)funkey(key_hi);
    // (np.nanmedian of an odd count is the middle sample itself - also an infinity; np.nanpercentile's lerp a + (b - a) t
    //  between two equal infinities is NaN, and so is it here)
    return (float)(((median && a == bb) ? a : (frac == 0.5 ? 0.5 * (a + bb) : a + (bb - a) * frac)) * scale);
}

// ---- rays with few valid samples (round 5) ---------------------------------------------------------------
// A signal mask (data > n sigma on narrow lines: the SURVEY's mask rule leaves 4 - 5 % of a cube) keeps a few dozen of a
// ray's 1024 samples, yet every digit pass and every statistics sweep walked all KPL key registers of every lane.  When NO
// ray of the block holds more than kCompactKeys x (lanes per ray) valid samples, the valid keys of a ray are packed into LDS -
// in sample order: per-lane counts, an exclusive prefix over the lanes of the ray, every lane writes its keys behind its
// prefix, so the packed order does not depend on scheduling - and dealt out again, kCompactKeys per lane; the descent and the
// clip loop then run on those instead of on KPL registers.  The packed set holds the same keys: the selection is identical, the
// clip loop's float64 sums are taken in another (fixed) order.
constexpr int kCompactKeys = 8;
template <int TS, int BT>
struct SelCompact {
    uint32_t keys[TS][kCompactKeys * (BT / TS)];       // a ray's valid keys in sample order
    uint32_t sorted[TS][kCompactKeys * (BT / TS)];     // ... ascending (clip_packed_waves)
    double ps[TS][BT / TS], pq[TS][BT / TS];           // lane partials of a ray's sums (clip_packed_waves)
    int cnt[TS][BT / TS];
    int tot[TS];
    uint32_t win[TS][2];
    int any_big;
};
template <int KPL, int TS, int BT>
constexpr bool sel_compactable() { return KPL >= 4 * kCompactKeys && (BT / TS) >= 8; }

// all threads of the block; true: ck holds this lane's share of the ray's n valid keys (block-uniform result)
template <int TS, int KPL, int BT>
__device__ __forceinline__ bool sel_compact(SelCompact<TS, BT>& Q, const uint32_t (&key)[KPL], int mine, int r, int j,
                                            uint32_t (&ck)[kCompactKeys], int& n) {
    constexpr int L = BT / TS, CAP = kCompactKeys * L;
    Q.cnt[r][j] = mine;
    if (threadIdx.x == 0) Q.any_big = 0;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll 4
    for (int l = 0; l < L; ++l) {
        const int c = Q.cnt[r][l];
        base += (l < j) ? c : 0;
        tot += c;
    }
    n = tot;
    if (j == 0) Q.tot[r] = tot;
    if (tot > CAP && j == 0) Q.any_big = 1;
    __syncthreads();
    if (Q.any_big) return false;
    int idx = base;
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
        if (key[i] != 0xffffffffu) { Q.keys[r][idx] = key[i]; ++idx; }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kCompactKeys; ++i) {
        const int sidx = j + L * i;
        ck[i] = sidx < tot ? Q.keys[r][sidx] : 0xffffffffu;
    }
    return true;
}

// (LDS traffic between the lanes of ONE wave: the LDS serves a wave's operations in order, the fence keeps the compiler
//  from reordering them)
__device__ __forceinline__ void sel_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

}  // namespace
