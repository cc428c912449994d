// spc_sigma_clip_impl.h - the fused sigma-clip kernel and its 256-thread launch table, shared by spc_sigma_clip.hip (spread = std,
// the entry point) and spc_sigma_clip_mad.hip (spread = mad_std: the 40 instantiations that run a second descent per iteration,
// 60 - 160 KB of code each, in a unit of their own for build time - as the stencils' r65f / r65m units).
//
// Internal linkage, like spc_select_impl.h: the kernels and their argument struct keep their unit-local names, so the one
// call that crosses units (spc_clip_launch_mad below) hands the struct over as bytes.
#pragma once
#include "spc_select_impl.h"

// spc_sigma_clip_mad.hip: clip_launch_base<true> on *args, a ClipRegArgs of the caller's (the same header, the same layout)
void spc_clip_launch_mad(const void* args, hipStream_t st);

namespace {

// ---- sigma clipping with the rays resident in registers -------------------------------------------------
// astropy.stats.sigma_clip(axis=0, masked=False) iterates centre / spread / clip over the cube; built from separate
// kernels every iteration reads it three times and writes it once (ops.sigma_clip_axis0: ~20 passes for the 5
// default iterations).  Here a block loads its TS rays once (the selection kernel's layout), iterates entirely in
// registers - valid count, sum and sum of squares per ray (float64, lane partials added in a fixed order: the result
// does not depend on scheduling), the median through ray_select, the bounds with spc_clip_bounds_f32's arithmetic,
// clipped samples turned into the "excluded" key - until no ray of the block changes or maxiters is reached, and
// writes the clipped rays once.  A ray that has converged recomputes the same bounds and clips nothing, so stopping per
// block equals astropy's global "until nothing changes".
struct ClipRegArgs {
    const float* cube;
    int64_t nz, ny, nx, row_stride, plane_stride;
    MaskDev mask;
    float* out;                 // (nz, ny, nx) C-contiguous
    double lo_s, hi_s;
    int maxiters;               // < 0: until convergence
    int cen_mean;               // centre: 0 median, 1 mean
    int spread_mad;             // spread: 0 std, 1 mad_std
    uint32_t key_min, key_span;            // sel_key_range of the mask's predicate terms (filled by the launcher)
    int xcd_group;              // tiles of a row kept on one XCD (sel_tile_of_block): kXcdGroup
    int compact;                // rays with few valid samples are packed (sel_compact; SPC_SELECT_COMPACT=0: off)
    const int* probe;           // NULL, or the largest valid count among the sampled rays (clip_probe_kernel): which block shape runs
};

// |x - centre| of the samples inside the clip window (the MAD's keys)
struct KeyAbsDevWin {
    float center;
    uint32_t wlo, wspan;
    __device__ __forceinline__ uint32_t operator()(uint32_t k) const {
        const float v = fabsf(funkey(k) - center);
        return ((k - wlo) < wspan && v == v) ? fkey(v) : 0xffffffffu;
    }
};

// the clip loop over one set of resident keys (all KPL registers of the lane, or its share of a packed sparse ray): narrows
// the window [wlo, wlo + wspan) of the keys that are kept
template <int TS, int KPL, bool MAD, int BT>
__device__ __forceinline__ void clip_iterate(const ClipRegArgs& A, SelShared<TS>& S, SelCache<TS>& C, double (*part_s)[BT / TS],
                                             double (*part_q)[BT / TS], uint32_t (&key)[KPL], int r, int j, uint32_t& wlo, uint32_t& wspan) {
    constexpr int kLanesPerRay = BT / TS;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    // The keys stay as loaded.  Clipping v < lo || v > hi removes the two ENDS of a ray's sorted samples, so what is left
    // is a window of keys [wlo, wlo + wspan): an iteration counts and sums the samples inside it, asks the resident key
    // set for the rank (samples below the window) + (n - 1) / 2 - a descent that resumes from the cached bins of the
    // earlier iterations' descents, the median moving by a few ranks only (round 3a re-ran all four passes over keys it
    // had overwritten: 1.9 ms per iteration at 1024^3) - and narrows the window.
    int n_prev = -1;
    bool cached = false;                                         // block-uniform: C holds an earlier iteration's descent
#pragma unroll 1
    for (int it = 0; A.maxiters < 0 || it < A.maxiters; ++it) {
        // (the keys never change, so everything an iteration derives from them alone - 64 floats, doubles, digits - would be
        //  hoisted out of the loop and spilled: they are made opaque once per iteration, which costs no instruction)
#pragma unroll
        for (int i = 0; i < KPL; ++i) asm volatile("" : "+v"(key[i]));
        // ---- valid count, sum, sum of squares of the ray (what spc_stats_axis_f32 gives the unfused path)
        // (the previous iteration's descent ends with lanes reading S.nextkey[r] behind its last barrier: without this barrier a
        //  wave that is already here resets the word under them - the upper of an even count's two middle samples came back as
        //  the "excluded" key in one launch out of four, tools/stress_clip_determinism.py)
        if (it > 0) __syncthreads();
        sel_reset<TS, BT>(S);
        int cnt = 0, low = 0;
        double s = 0.0, ss = 0.0;
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const bool ok = (key[i] - wlo) < wspan;
            const double v = ok ? (double)funkey(key[i]) : 0.0;
            cnt += ok ? 1 : 0;
            low += (key[i] < wlo) ? 1 : 0;
            s += v;
            ss = fma(v, v, ss);
            if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);
        }
        part_s[r][j] = s;
        part_q[r][j] = ss;
        __syncthreads();                                         // (also orders sel_reset before the counts)
        if (cnt) atomicAdd(&S.nvalid[r], (uint32_t)cnt);
        if (low) atomicAdd(&S.nlow[r], (uint32_t)low);
        double sum = 0.0, ssq = 0.0;
#pragma unroll 4
        for (int l = 0; l < kLanesPerRay; ++l) { sum += part_s[r][l]; ssq += part_q[r][l]; }
        __syncthreads();
        const int n = (int)S.nvalid[r], nl = (int)S.nlow[r];
        // (the previous iteration clipped nothing anywhere in the block: astropy stops there)
        if (it > 0 && !__syncthreads_or(n != n_prev ? 1 : 0)) break;
        n_prev = n;
        double mean = nan, sd = nan;
        if (n > 0) {
            mean = sum / (double)n;
            const double var = __dsub_rn(ssq / (double)n, __dmul_rn(mean, mean));
            sd = (var != var) ? nan : sqrt(var > 0.0 ? var : 0.0);
        }
        double cen = mean;
        float med = NAN;
        if (!A.cen_mean || MAD) {
            uint32_t key_lo, key_hi;
            double frac;
            ray_select<TS, KPL, BT>(S, key, KeyIdentity{}, r, j, n, 50.0, key_lo, key_hi, frac, 8, nl, &C, cached);
            cached = true;
            med = n > 0 ? sel_value(key_lo, key_hi, frac, 1.0) : NAN;
            if (!A.cen_mean) cen = (double)med;
        }
        if (MAD) {
            // spread = 1.4826 x the median of |x - median| (astropy mad_std; float32 deviations like numpy's, the scale
            // in float32 like spc_percentile_axis0_f32's argument): a second descent over the transformed keys
            const KeyAbsDevWin xf{med, wlo, wspan};
            __syncthreads();                                     // the first descent's last reads of S
            sel_reset<TS, BT>(S);
            __syncthreads();
            int nm = n;
            if (__syncthreads_or((n > 0 && !(fabsf(med) <= 3.4028234664e38f)) ? 1 : 0)) {
                // an infinite median: inf - inf deviations are NaN and drop out of the ray
                int c = 0;
#pragma unroll
                for (int i = 0; i < KPL; ++i) c += (xf(key[i]) != 0xffffffffu) ? 1 : 0;
                if (c) atomicAdd(&S.nvalid[r], (uint32_t)c);
                __syncthreads();
                nm = (int)S.nvalid[r];
            }
            uint32_t key_lo, key_hi;
            double frac;
            ray_select<TS, KPL, BT>(S, key, xf, r, j, nm, 50.0, key_lo, key_hi, frac, 8, 0, nullptr, false, /*early*/ false);
            const float spread = nm > 0 ? sel_value(key_lo, key_hi, frac, (double)1.482602218505602f) : NAN;
            sd = (double)spread;
            if (A.cen_mean) cen = (double)(float)mean;           // (the loop of separate kernels hands a float32 mean map over)
        }
        const float lo = (float)__dsub_rn(cen, __dmul_rn(A.lo_s, sd));
        const float hi = (float)__dadd_rn(cen, __dmul_rn(A.hi_s, sd));
        // v < lo  <=>  key < key(lo), v > hi  <=>  key > key(hi); a bound of either zero keeps both zeros; NaN bounds clip nothing
        if (wspan != 0u) {
            const uint32_t klo = (lo == lo) ? fkey(lo == 0.f ? -0.f : lo) : 0u;
            const uint32_t khi = (hi == hi) ? fkey(hi == 0.f ? 0.f : hi) : 0xff800000u;
            const uint32_t nlo = max(wlo, klo), nhi = min(wlo + (wspan - 1u), khi);
            wlo = nlo;
            wspan = nhi >= nlo ? nhi - nlo + 1u : 0u;
        }
    }
}

// The clip loop over PACKED rays (sel_compact: no ray of the block holds more than 128 valid samples), every wave on its own:
// what an iteration costs on 8 keys per lane is not arithmetic but the block's rendezvous - ~20 barriers per iteration, three
// LDS histogram rounds per digit pass: 0.75 ms per iteration at 1024^3 whether a lane walks 64 keys or 8.  With 16 lanes per ray
// a wave takes four whole rays instead: it sorts each once (every lane ranks its <= 8 keys against the ray's, ties by sample
// index - n^2 / 16 compares per lane, n ~ 50 under a signal mask), after which the median of any clip window is two LDS reads
// (the window removes the two ends of the sorted keys), counts come from a 16-lane butterfly and the float64 sums from lane
// partials added in a fixed order.  No barrier, no atomics, no descent; a wave stops when none of ITS rays changes.  The
// arithmetic of the bounds is clip_iterate's (astropy's): the same windows up to the order of the float64 additions.
// REPRODUCIBILITY (round-5 advisor): which of the two loops a ray takes depends on ITS BLOCK (every ray of the block sparse) and
// on the 64-ray probe that picks the block shape, so the float64 mean / std of one spectrum can be added up in two different
// (each fixed) orders depending on the cube's width or on how it was sharded: the bounds then differ in their last bits and a
// sample that sits within 1e-16 relative of a bound can be clipped in one run and kept in the other.  Launch-to-launch results
// on the SAME cube are bit-identical (tests/test_gpu_fullsize.py); sigma_clip_spectrally is NOT among the operators whose
// sharded result is bit-identical to the unsharded one (DESIGN section 7 lists them) - like astropy's own result, which
// moves in the same way with numpy's pairwise summation block size.
// (its own function, not inlined: in line, the sort's registers on top of the 64 resident keys made the allocator spill 57 VGPRs and
//  the DENSE loop of the same kernel went from 7.7 to 9.4 ms)
struct ClipScalars { double lo_s, hi_s; int maxiters, cen_mean; };
template <int TS, int BT>
__device__ __attribute__((noinline)) void clip_packed_waves(const ClipScalars A, SelCompact<TS, BT> __attribute__((address_space(3)))* Qp) {
    static_assert(BT / TS == 16, "16 lanes per ray: four rays per wave");
    auto& Q = *Qp;                                                   // (an LDS pointer: ds_read / ds_write, not flat accesses)
    constexpr int KC = kCompactKeys;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rr = 4 * w + (lane >> 4), jl = lane & 15;
    const int n_all = Q.tot[rr];
    const int nmax = max(max(__builtin_amdgcn_readlane(n_all, 0), __builtin_amdgcn_readlane(n_all, 16)),
                         max(__builtin_amdgcn_readlane(n_all, 32), __builtin_amdgcn_readlane(n_all, 48)));
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    // ---- sort: position of a key = keys below it (ties: earlier samples first).  Candidates four at a time (one 16-byte LDS
    // read), two reads in flight; slots past a ray's count compare as the largest key.
    unsigned long long mine64[KC];
    int pos[KC];
#pragma unroll
    for (int i = 0; i < KC; ++i) {
        const int idx = jl + 16 * i;
        const uint32_t k = idx < n_all ? Q.keys[rr][idx] : 0xffffffffu;
        mine64[i] = ((unsigned long long)k << 32) | (unsigned)idx;
        pos[i] = 0;
    }
    const u32x4 __attribute__((address_space(3)))* cand = reinterpret_cast<const u32x4 __attribute__((address_space(3)))*>(&Q.keys[rr][0]);
    for (int m0 = 0; m0 < nmax; m0 += 8) {
        const u32x4 c0 = cand[m0 / 4], c1 = cand[m0 / 4 + 1];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int m = m0 + u;
            const uint32_t raw = u < 4 ? c0[u & 3] : c1[u & 3];
            const uint32_t o = m < n_all ? raw : 0xffffffffu;
            const unsigned long long o64 = ((unsigned long long)o << 32) | (unsigned)m;
#pragma unroll
            for (int i = 0; i < KC; ++i)
                if (16 * i < nmax) pos[i] += (o64 < mine64[i]) ? 1 : 0;      // (wave-uniform guard)
        }
    }
#pragma unroll
    for (int i = 0; i < KC; ++i)
        if (jl + 16 * i < n_all) Q.sorted[rr][pos[i]] = (uint32_t)(mine64[i] >> 32);
    sel_wave_sync();
    uint32_t sk[KC];
#pragma unroll
    for (int i = 0; i < KC; ++i) sk[i] = (jl + 16 * i < n_all) ? Q.sorted[rr][jl + 16 * i] : 0xffffffffu;
    // ---- iterate
    uint32_t wlo = 0u, wspan = 0xff800001u;
    int n_prev = -1;
#pragma unroll 1
    for (int it = 0; A.maxiters < 0 || it < A.maxiters; ++it) {
        int cnt = 0, low = 0;
        double s = 0.0, ss = 0.0;
#pragma unroll
        for (int i = 0; i < KC; ++i) {
            if (16 * i < nmax) {
                const bool ok = (sk[i] - wlo) < wspan;
                const double v = ok ? (double)funkey(sk[i]) : 0.0;
                cnt += ok ? 1 : 0;
                low += (sk[i] < wlo) ? 1 : 0;
                s += v;
                ss = fma(v, v, ss);
            }
        }
        Q.ps[rr][jl] = s;
        Q.pq[rr][jl] = ss;
        int both = cnt | (low << 16);                                   // (<= 128 each)
        both += __builtin_amdgcn_ds_swizzle(both, 0x041f);               // butterfly over the 16 lanes of the ray: xor 1, 2, 4, 8
        both += __builtin_amdgcn_ds_swizzle(both, 0x081f);
        both += __builtin_amdgcn_ds_swizzle(both, 0x101f);
        both += __builtin_amdgcn_ds_swizzle(both, 0x201f);
        sel_wave_sync();
        double sum = 0.0, ssq = 0.0;
#pragma unroll
        for (int l = 0; l < 16; ++l) { sum += Q.ps[rr][l]; ssq += Q.pq[rr][l]; }
        sel_wave_sync();
        const int n = both & 0xffff, nl = both >> 16;
        if (it > 0 && __builtin_amdgcn_ballot_w64(n != n_prev) == 0ull) break;    // none of this wave's rays lost a sample
        n_prev = n;
        double mean = nan, sd = nan;
        if (n > 0) {
            mean = sum / (double)n;
            const double var = __dsub_rn(ssq / (double)n, __dmul_rn(mean, mean));
            sd = (var != var) ? nan : sqrt(var > 0.0 ? var : 0.0);
        }
        double cen = mean;
        if (!A.cen_mean) {
            float med = NAN;
            if (n > 0) {
                const double p = 0.5 * (double)(n - 1), fl = floor(p);
                const uint32_t key_lo = Q.sorted[rr][nl + (int)fl], key_hi = Q.sorted[rr][nl + min((int)ceil(p), n - 1)];
                med = sel_value(key_lo, key_hi, p - fl, 1.0);
            }
            cen = (double)med;
        }
        const float lo = (float)__dsub_rn(cen, __dmul_rn(A.lo_s, sd));
        const float hi = (float)__dadd_rn(cen, __dmul_rn(A.hi_s, sd));
        if (wspan != 0u) {
            const uint32_t klo = (lo == lo) ? fkey(lo == 0.f ? -0.f : lo) : 0u;
            const uint32_t khi = (hi == hi) ? fkey(hi == 0.f ? 0.f : hi) : 0xff800000u;
            const uint32_t nlo = max(wlo, klo), nhi = min(wlo + (wspan - 1u), khi);
            wlo = nlo;
            wspan = nhi >= nlo ? nhi - nlo + 1u : 0u;
        }
    }
    if (jl == 0) { Q.win[rr][0] = wlo; Q.win[rr][1] = wspan; }
}

// Which block shape suits the cube is a property of its mask: packed rays (<= 128 valid samples each) iterate for free, so the
// 512-thread blocks' wider runs per plane win (read + write floor 2.4 against 3.3 ms at 1024^3); rays that stay in the registers
// iterate faster in 256-thread blocks.  The host cannot know without waiting for the device: a probe kernel counts the valid
// samples of 64 rays spread over the map and leaves the largest count in the caller's workspace, BOTH shapes are launched, and
// the blocks of the one the count does not select retire at once (an empty grid of 65536 blocks: ~20 us).
constexpr int kProbeRays = 64, kProbeSparse = 96;

template <int TS, int KPL, bool ARR, bool MAD, bool DESC, int BT = 256>
// (blocks per CU: what the registers of each shape allow, as the compiler reports it - the instantiations that asked for four
//  and reached two or three now say so; the dense-mask shape <16, 64> reaches its four)
__global__ __launch_bounds__(BT, KPL == 128 ? 1 : (MAD ? 2 : (BT != 256 ? 4 : (TS == 128 ? 2 : (TS == 32 ? ((KPL == 64 && !DESC) ? 2 : 3) : 4))))) void sigma_clip_reg_kernel(const ClipRegArgs A) {
    if (A.probe != nullptr && ((*A.probe <= kProbeSparse) != (BT == 512))) return;   // the other block shape runs this cube
    __shared__ SelShared<TS> S;
    __shared__ SelCache<TS> C;
    constexpr int kLanesPerRay = BT / TS;
    __shared__ double part_s[TS][kLanesPerRay], part_q[TS][kLanesPerRay];
    const int t = threadIdx.x;
    const int r = t % TS, j = t / TS;
    const int64_t tiles_x = (A.nx + TS - 1) / TS;
    const int64_t tile = sel_tile_of_block(blockIdx.x, gridDim.x, A.xcd_group);
    const int64_t y = tile / tiles_x, x0 = (tile % tiles_x) * TS;
    const int nz = (int)A.nz;
    const bool col_in = x0 + r < A.nx;
    uint32_t key[KPL];
    const int mine = sel_load_keys<TS, KPL, ARR, DESC, BT>(A.cube, A.plane_stride, 1, y * A.row_stride + x0, A.mask.arr, A.mask.plane_stride, 1,
                                ARR ? y * A.mask.row_stride + x0 : 0, col_in ? r : (int)(A.nx - 1 - x0), j, nz,
                                col_in, A.key_min, A.key_span, false, 0.f, key);
    uint32_t wlo = 0u, wspan = 0xff800001u;                      // every valid key (the excluded one lies above)
    bool packed = false;
    if constexpr (sel_compactable<KPL, TS, BT>()) {
        // (a probe that met a ray of more than 128 valid samples: a dense cube, whose blocks need not even ask)
        if (A.compact && (A.probe == nullptr || *A.probe <= kCompactKeys * (BT / TS))) {
            __shared__ SelCompact<TS, BT> Q;
            uint32_t ck[kCompactKeys];
            int nc = 0;
            packed = sel_compact<TS, KPL, BT>(Q, key, mine, r, j, ck, nc);
            if (packed) {
                if constexpr (!MAD && BT / TS == 16) {
                    if (A.compact >= 2) {
                        clip_packed_waves<TS, BT>(ClipScalars{A.lo_s, A.hi_s, A.maxiters, A.cen_mean}, (SelCompact<TS, BT> __attribute__((address_space(3)))*)&Q);
                        __syncthreads();
                        wlo = Q.win[r][0];
                        wspan = Q.win[r][1];
                    } else {
                        clip_iterate<TS, kCompactKeys, MAD, BT>(A, S, C, part_s, part_q, ck, r, j, wlo, wspan);
                    }
                } else {
                    clip_iterate<TS, kCompactKeys, MAD, BT>(A, S, C, part_s, part_q, ck, r, j, wlo, wspan);
                }
            }
        }
    }
    if (!packed) clip_iterate<TS, KPL, MAD, BT>(A, S, C, part_s, part_q, key, r, j, wlo, wspan);
    (void)mine;
    // ---- the clipped rays, written once
    if (col_in) {
        float* q = A.out + y * A.nx + x0 + r + (int64_t)j * A.ny * A.nx;
        const int64_t qstep = (int64_t)kLanesPerRay * A.ny * A.nx;
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
            const int z = j + kLanesPerRay * i;
            if (z < nz) *q = ((key[i] - wlo) < wspan) ? funkey(key[i]) : NAN;
            q += qstep;
            if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// ---- the 256-thread launch table of sigma_clip_reg_kernel, one spread (MAD) at a time ----------------------------------
// The selection's Base shapes - 32 / 16 / 8 spaxels per block for rays of up to 512 / 1024 / 4096 samples, 16 .. 64 keys per lane,
// 128 for the 2049 .. 4096 samples of 8 spaxels - each with and without a mask array and descriptor loads (SPC_SELECT_DESC, on
// by default here: 10.1 against 10.8 ms at 1024^3, mad_std 28.3 against 31.9 ms): 10 rows, 40 instantiations per spread.
// Four of the rows no ray length reaches - <16, 16>, <16, 32> (513 .. 1024 samples on 16 lanes need 33 .. 64 keys) and <8, 16>,
// <8, 32> (more than 1024 samples on 32 lanes likewise): they are kept because the set of kernels is.
template <bool MAD>
static void clip_launch_base(const ClipRegArgs& A, hipStream_t st) {
    const int64_t nz = A.nz;
    const bool arr = (A.mask.flags & SPC_MASK_ARRAY) != 0;
    const int ts = sel_ts256(nz), kpl = sel_kpl(nz, 256 / ts);
    const bool desc = sel_desc_fits(ts, std::max<int64_t>(A.plane_stride, arr ? A.mask.plane_stride : 0), 1) &&
                      spc_switch("SPC_SELECT_DESC", 1) != 0;
    const dim3 grid((unsigned)(A.ny * ((A.nx + ts - 1) / ts)));
    auto row = [&](auto ts_c, auto kpl_c) {
        constexpr int TS = decltype(ts_c)::value, KPL = decltype(kpl_c)::value;
        sel_with_bool(arr, [&](auto arr_c) {
            sel_with_bool(desc, [&](auto desc_c) {
                hipLaunchKernelGGL((sigma_clip_reg_kernel<TS, KPL, decltype(arr_c)::value, MAD, decltype(desc_c)::value, 256>), grid, dim3(256), 0, st, A);
            });
        });
    };
    auto row_by_kpl = [&](auto ts_c) {                          // 16, 32 or 64 keys per lane
        if (kpl == 16) row(ts_c, SelInt<16>{});
        else if (kpl == 32) row(ts_c, SelInt<32>{});
        else row(ts_c, SelInt<64>{});
    };
    if (kpl == 128) row(SelInt<8>{}, SelInt<128>{});
    else if (ts == 32) row_by_kpl(SelInt<32>{});
    else if (ts == 16) row_by_kpl(SelInt<16>{});
    else row_by_kpl(SelInt<8>{});
}

}  // namespace
