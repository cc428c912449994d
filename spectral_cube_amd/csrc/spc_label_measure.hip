// spc_label_measure.hip - per-label measurements of a cube through the int32 labels of spc_label_u8: the counts, sums,
// extrema with their positions and first / second moments behind scipy.ndimage.sum_labels, mean, variance, minimum,
// maximum, minimum_position, maximum_position, extrema and center_of_mass, which users of the reference run on the host
// on the label array and the cube.  One streaming segmented reduction; only the per-label tables travel.
//
// Rules (include/spcube_hip.h).  A voxel is measured when its label is above 0, the cube's mask includes it and its sample
// is not NaN.  Every sum is float64.  The groups of tables (SUMS, EXTREMA, FIRST, SECOND) are chosen by `want`, and the
// kernel is specialised on it: a sums-only launch of a contiguous cube forms no coordinate at all.
//
// The hot path, lm_kernel, walks like lb_objects_kernel (spc_label.hip).  Lanes run along x; a wave takes 16 to 256 x 64
// CONSECUTIVE voxels a round (the longest walk that still fills the grid).  The label is loaded first: the mask byte and
// the sample are fetched only where it is above 0, and 64 voxels of background cost one ballot.  The labelled voxels of
// one label that follow each other in the walk are a run - a voxel without a label does not end it, it goes with the
// labelled voxel before it and adds nothing, so the rows of a cloud inside one walk are ONE run.  Runs are found with two
// shuffles and two ballots.  The run that is open at the end of 64 voxels is carried, per lane: while the next 64 voxels
// all go on with it, every lane adds its own voxel to its own partial totals and nothing is shuffled at all - the inside
// of a cloud, a label that fills the array.  Where another label begins, the carried partials are reduced over the wave
// and every quantity of the runs that END in these 64 voxels is reduced by a segmented shuffle reduction (six steps, a
// lane adds the lane o above it while that lane is still in its run), so a run costs ONE global atomic per quantity,
// issued by one lane, whatever its length: a label that fills the array costs one atomic per quantity and wave.
//
// Atomics: float64 adds (global_atomic_add_f64) for the sums, 64-bit unsigned minima (global_atomic_umin_x2) for the
// extrema, all relaxed at agent scope, none with a returned value and none in a loop.  The order of the adds is not fixed:
// the sums are reproducible to float64 rounding only (the header says how far); counts, extrema and positions are exact.
// Extrema are minima of order-preserving keys.  float32: the key is the encoded sample in the high half and the linear
// index in the low half (the complemented encoding for the maximum), so one minimum gives the value and its FIRST
// position.  float64: the key is the encoded sample; a second launch of the same kernel (POS) takes the minimum of the
// index over the voxels whose sample equals their label's extreme.  -0.0 is encoded as +0.0: the two compare equal.
//
// Termination.  No workgroup waits for another: no spin, ticket or look-back; every loop has a bound stated where it is.
//
// Bytes per voxel: 4 B of labels for every voxel, plus the sample (4 / 8 B) and the mask byte (1 B, when the mask has an
// array term) of the labelled voxels only, plus 8 - 32 B of origin per labelled voxel that mostly hit L2 (a row per label).
#include "spc_common.h"

namespace {

constexpr int LM_BLOCK = 256;
constexpr int LM_MIN_CHUNKS = 16, LM_MAX_CHUNKS = 256;                // 64-voxel chunks a wave walks through a round
constexpr int64_t LM_MAX_BLOCKS = 2048;
constexpr int64_t LM_MAX_VOXELS = INT32_MAX;
constexpr unsigned LM_ALL = SPC_MEASURE_SUMS | SPC_MEASURE_EXTREMA | SPC_MEASURE_FIRST | SPC_MEASURE_SECOND;
constexpr unsigned LM_COUNTED = SPC_MEASURE_SUMS | SPC_MEASURE_FIRST | SPC_MEASURE_SECOND;    // the groups that are sums
constexpr unsigned long long LM_NONE = ~0ull;                         // a key no sample has; as an int64 position: -1
static_assert(LM_BLOCK % 64 == 0, "a wave's 64 voxels start at a multiple of 64");

// order-preserving keys: a < b as samples <=> enc(a) < enc(b) as unsigned integers.  Neither ~0 (the bits of a NaN) nor 0
// (the bits of another) is the key of a sample that is measured.
__device__ __forceinline__ uint32_t lm_enc(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long lm_enc(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ __forceinline__ float lm_dec32(uint32_t e) {
    return __uint_as_float((e & 0x80000000u) ? (e ^ 0x80000000u) : ~e);
}
__device__ __forceinline__ double lm_dec64(unsigned long long e) {
    return __longlong_as_double((long long)((e >> 63) ? (e ^ (1ull << 63)) : ~e));
}

template <typename T>
struct LmArgs {
    const T* data;                       // the cube, strides rs / ps
    int64_t rs, ps;
    SpcMaskDev<T> M;
    const int32_t* L;
    int64_t n, nlabels;
    uint32_t ny, nx;
    int contig;                          // cube and mask array are C-contiguous: a voxel's offset is its linear index
    int chunks;                          // 64-voxel chunks a wave walks through a round
    const double* origin;                // (nlabels + 1) x 4: v0, z0, y0, x0, or nullptr
    unsigned long long* count;           // SUMS
    double* sums;
    unsigned long long* kmin;            // EXTREMA: the key tables; in the POS launch the position tables
    unsigned long long* kmax;
    const unsigned long long* vmin;      // POS: the key tables of the launch before
    const unsigned long long* vmax;
    double* first;
    double* second;
    uint32_t* bad;
    // the tables lm_finish decodes the keys into
    void* omin;
    void* omax;
    long long* pmin;
    long long* pmax;
};

// what one voxel, one run or the carried run has added up; only the members of the wanted groups are ever touched
template <unsigned W>
struct LmAcc {
    long long c;
    double a1, a2;
    unsigned long long lo, hi;
    double f[4];
    double s[6];
};

template <unsigned W>
__device__ __forceinline__ LmAcc<W> lm_identity() {
    LmAcc<W> a;
    if constexpr (W & LM_COUNTED) a.c = 0;
    if constexpr (W & SPC_MEASURE_SUMS) { a.a1 = 0.0; a.a2 = 0.0; }
    if constexpr (W & SPC_MEASURE_EXTREMA) { a.lo = LM_NONE; a.hi = LM_NONE; }
    if constexpr (W & SPC_MEASURE_FIRST) {
#pragma unroll
        for (int q = 0; q < 4; ++q) a.f[q] = 0.0;
    }
    if constexpr (W & SPC_MEASURE_SECOND) {
#pragma unroll
        for (int q = 0; q < 6; ++q) a.s[q] = 0.0;
    }
    return a;
}

template <unsigned W>
__device__ __forceinline__ void lm_combine(LmAcc<W>& a, const LmAcc<W>& b) {
    if constexpr (W & LM_COUNTED) a.c += b.c;
    if constexpr (W & SPC_MEASURE_SUMS) { a.a1 += b.a1; a.a2 += b.a2; }
    if constexpr (W & SPC_MEASURE_EXTREMA) { a.lo = b.lo < a.lo ? b.lo : a.lo; a.hi = b.hi < a.hi ? b.hi : a.hi; }
    if constexpr (W & SPC_MEASURE_FIRST) {
#pragma unroll
        for (int q = 0; q < 4; ++q) a.f[q] += b.f[q];
    }
    if constexpr (W & SPC_MEASURE_SECOND) {
#pragma unroll
        for (int q = 0; q < 6; ++q) a.s[q] += b.s[q];
    }
}

// S(x): x of another lane
template <unsigned W, typename S>
__device__ __forceinline__ LmAcc<W> lm_moved(const LmAcc<W>& a, S sh) {
    LmAcc<W> t;
    if constexpr (W & LM_COUNTED) t.c = sh(a.c);
    if constexpr (W & SPC_MEASURE_SUMS) { t.a1 = sh(a.a1); t.a2 = sh(a.a2); }
    if constexpr (W & SPC_MEASURE_EXTREMA) { t.lo = sh(a.lo); t.hi = sh(a.hi); }
    if constexpr (W & SPC_MEASURE_FIRST) {
#pragma unroll
        for (int q = 0; q < 4; ++q) t.f[q] = sh(a.f[q]);
    }
    if constexpr (W & SPC_MEASURE_SECOND) {
#pragma unroll
        for (int q = 0; q < 6; ++q) t.s[q] = sh(a.s[q]);
    }
    return t;
}

__device__ __forceinline__ void lm_add(double* p, double v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lm_umin(unsigned long long* p, unsigned long long v) {
    if (v != LM_NONE) __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the totals of one run leave the wave: one atomic per quantity; k < 0 (the background, a label out of range) has no table row
template <typename T, unsigned W>
__device__ __forceinline__ void lm_flush(const LmArgs<T>& A, int32_t k, const LmAcc<W>& a) {
    if (k < 0) return;
    if constexpr (W & SPC_MEASURE_EXTREMA) {                          // (a key of LM_NONE: nothing measured, no atomic)
        lm_umin(A.kmin + k, a.lo);
        lm_umin(A.kmax + k, a.hi);
    }
    if constexpr (W & LM_COUNTED) {
        if (a.c <= 0) return;                                         // nothing measured (masked, NaN): every sum of the run is 0
    }
    if constexpr (W & SPC_MEASURE_SUMS) {
        __hip_atomic_fetch_add(A.count + k, (unsigned long long)a.c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        lm_add(A.sums + 2 * (int64_t)k, a.a1);
        lm_add(A.sums + 2 * (int64_t)k + 1, a.a2);
    }
    if constexpr (W & SPC_MEASURE_FIRST) {
#pragma unroll
        for (int q = 0; q < 4; ++q) lm_add(A.first + 4 * (int64_t)k + q, a.f[q]);
    }
    if constexpr (W & SPC_MEASURE_SECOND) {
#pragma unroll
        for (int q = 0; q < 6; ++q) lm_add(A.second + 6 * (int64_t)k + q, a.s[q]);
    }
}

// what voxel i of label k > 0 adds: the identity when the mask excludes it or its sample is NaN
template <typename T, unsigned W, bool POS>
__device__ __forceinline__ LmAcc<W> lm_voxel(const LmArgs<T>& A, int64_t i, int32_t k) {
    constexpr bool COORD = (W & (SPC_MEASURE_FIRST | SPC_MEASURE_SECOND)) != 0;
    LmAcc<W> a = lm_identity<W>();
    uint32_t z = 0, y = 0, x = 0;
    int64_t off = i, moff = i;
    if (COORD || !A.contig) {
        const uint32_t row = (uint32_t)i / A.nx;
        x = (uint32_t)i - row * A.nx;
        z = row / A.ny;
        y = row - z * A.ny;
        off = (int64_t)z * A.ps + (int64_t)y * A.rs + x;
        moff = (int64_t)z * A.M.plane_stride + (int64_t)y * A.M.row_stride + x;
    }
    if (A.M.arr != nullptr && A.M.arr[moff] == 0) return a;           // the mask byte before the sample
    T v = A.data[off];
    if (!spc_pred_valid(A.M, v)) return a;                            // the predicate terms, and never a NaN
    const double* o = A.origin ? A.origin + 4 * (int64_t)k : nullptr;
    if constexpr (W & LM_COUNTED) a.c = 1;
    if constexpr (W & SPC_MEASURE_SUMS) {
        const double dv = (double)v - (o ? o[0] : 0.0);
        a.a1 = dv;
        a.a2 = dv * dv;
    }
    if constexpr (W & SPC_MEASURE_EXTREMA) {
        if (v == (T)0) v = (T)0;                                      // -0.0 == +0.0: one key for both
        if constexpr (POS) {
            a.lo = lm_enc(v) == A.vmin[k] ? (unsigned long long)i : LM_NONE;
            a.hi = ~lm_enc(v) == A.vmax[k] ? (unsigned long long)i : LM_NONE;
        } else if constexpr (sizeof(T) == 4) {
            const uint32_t e = lm_enc(v);
            a.lo = ((unsigned long long)e << 32) | (uint32_t)i;      // i < 2^31
            a.hi = ((unsigned long long)(~e) << 32) | (uint32_t)i;
        } else {
            a.lo = lm_enc(v);
            a.hi = ~lm_enc(v);
        }
    }
    if constexpr (COORD) {
        const double w = (double)v;
        const double dz = (double)z - (o ? o[1] : 0.0), dy = (double)y - (o ? o[2] : 0.0), dx = (double)x - (o ? o[3] : 0.0);
        if constexpr (W & SPC_MEASURE_FIRST) {
            a.f[0] = w; a.f[1] = w * dz; a.f[2] = w * dy; a.f[3] = w * dx;
        }
        if constexpr (W & SPC_MEASURE_SECOND) {
            const double wz = w * dz, wy = w * dy;
            a.s[0] = wz * dz; a.s[1] = wy * dy; a.s[2] = (w * dx) * dx;
            a.s[3] = wz * dy; a.s[4] = wz * dx; a.s[5] = wy * dx;
        }
    }
    return a;
}

// lane 0: the totals of the whole wave
template <unsigned W>
__device__ __forceinline__ LmAcc<W> lm_wave_total(LmAcc<W> a, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {                                // bound: 6 doublings; after each, a = the sum of [lane, min(lane + 2 o, 64))
        const LmAcc<W> t = lm_moved<W>(a, [o](auto x) { return __shfl_down(x, o); });
        if (lane + o < 64) lm_combine<W>(a, t);
    }
    return a;
}

template <typename T, unsigned W, bool POS>
__global__ __launch_bounds__(LM_BLOCK) void lm_kernel(const LmArgs<T> A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t span = (int64_t)LM_BLOCK * A.chunks;                // voxels per block and round
    bool bad = false;
    int32_t open = -1;                                                // the label of the run that is carried (uniform)
    LmAcc<W> pl = lm_identity<W>();                                   // what every LANE has added to the carried run
    bool live = false;                                                // (uniform) pl holds something
    // bound: b0 grows by a positive stride up to n
    for (int64_t b0 = (int64_t)blockIdx.x * span; b0 < A.n; b0 += (int64_t)gridDim.x * span) {
        const int64_t w0 = b0 + (int64_t)wave * 64 * A.chunks;
#pragma unroll 1
        for (int c = 0; c < A.chunks; ++c) {                          // bound: chunks <= LM_MAX_CHUNKS (uniform over the wave)
            const int64_t c0 = w0 + (int64_t)c * 64;
            if (c0 >= A.n) break;
            const int64_t i = c0 + lane;
            int32_t ks = -1;                                          // the label when it is measured: 1 ... nlabels
            if (i < A.n) {
                const int32_t k = A.L[i];
                if (k < 0 || (int64_t)k > A.nlabels) bad = true;
                else if (k > 0) ks = k;
            }
            // 64 voxels without a label: nothing is fetched, and the carried run stays open (the same label may go on behind)
            const uint64_t any = __ballot(ks >= 0);
            if (any == 0ull) continue;
            // a voxel without a label does not end a run: it goes with the labelled voxel before it (with the carried run
            // when there is none in these 64) and adds nothing, so a label's rows inside a wave's walk are ONE run
            const uint64_t below = any & ((1ull << lane) - 1ull);
            const int32_t kb = __shfl(ks, below ? 63 - __clzll((long long)below) : 0);
            const int32_t ke = ks >= 0 ? ks : (below ? kb : open);
            LmAcc<W> a = lm_identity<W>();
            if (ks >= 0) a = lm_voxel<T, W, POS>(A, i, ks);
            const int32_t kp = __shfl_up(ke, 1);
            const bool head = lane == 0 || ke != kp;
            const uint64_t HK = __ballot(head);
            const int32_t kf = __shfl(ke, 0);
            if (HK == 1ull && kf == open) {                           // (uniform) all 64 go on with the carried run: no shuffle at all
                lm_combine<W>(pl, a);
                live = true;
                continue;
            }
            if (live) {                                               // (uniform) the carried run ends here or goes on in the first run
                const LmAcc<W> r = lm_wave_total<W>(pl, lane);
                if (kf != open) {
                    if (lane == 0) lm_flush<T, W>(A, open, r);
                } else if (lane == 0) {
                    lm_combine<W>(a, r);
                }
            }
            // the first lane past this lane's run
            const uint64_t above = lane == 63 ? 0ull : HK >> (lane + 1);
            const int lim = above ? lane + 1 + __builtin_ctzll(above) : 64;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {                        // bound: 6 doublings; after each, a = the sum of [lane, min(lane + 2 o, lim))
                const LmAcc<W> t = lm_moved<W>(a, [o](auto x) { return __shfl_down(x, o); });
                if (lane + o < lim) lm_combine<W>(a, t);
            }
            const int last = 63 - __clzll((long long)HK);             // the head of the chunk's last run (bit 0 is set)
            if (head && lane != last) lm_flush<T, W>(A, ke, a);       // complete runs; the last stays open, its totals in its head lane
            open = __shfl(ke, last);
            pl = lm_identity<W>();
            if (lane == last) pl = a;
            live = true;
        }
    }
    if (live) {
        const LmAcc<W> r = lm_wave_total<W>(pl, lane);
        if (lane == 0) lm_flush<T, W>(A, open, r);
    }
    if (__ballot(bad) != 0ull && lane == 0) __hip_atomic_fetch_or(A.bad, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// every table of the wanted groups, the key tables and the flag: what the call finds there is never read
template <typename T>
__global__ __launch_bounds__(LM_BLOCK) void lm_init_kernel(const LmArgs<T> A, unsigned want) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *A.bad = 0u;
    // bound: k grows by a positive stride up to nlabels
    for (int64_t k = (int64_t)blockIdx.x * LM_BLOCK + threadIdx.x; k <= A.nlabels; k += (int64_t)gridDim.x * LM_BLOCK) {
        if (want & SPC_MEASURE_SUMS) { A.count[k] = 0ull; A.sums[2 * k] = 0.0; A.sums[2 * k + 1] = 0.0; }
        if (want & SPC_MEASURE_EXTREMA) {
            A.kmin[k] = LM_NONE; A.kmax[k] = LM_NONE;
            if (sizeof(T) == 8) { A.pmin[k] = -1; A.pmax[k] = -1; }   // LM_NONE: the POS launch takes minima of these
        }
        if (want & SPC_MEASURE_FIRST) for (int q = 0; q < 4; ++q) A.first[4 * k + q] = 0.0;       // bound: 4
        if (want & SPC_MEASURE_SECOND) for (int q = 0; q < 6; ++q) A.second[6 * k + q] = 0.0;     // bound: 6
    }
}

// keys -> the extreme samples (and, float32, their positions); a label without a measured voxel: NaN and -1
template <typename T>
__global__ __launch_bounds__(LM_BLOCK) void lm_finish_kernel(const LmArgs<T> A) {
    // bound: k grows by a positive stride up to nlabels
    for (int64_t k = (int64_t)blockIdx.x * LM_BLOCK + threadIdx.x; k <= A.nlabels; k += (int64_t)gridDim.x * LM_BLOCK) {
        const unsigned long long lo = A.kmin[k], hi = A.kmax[k];
        if constexpr (sizeof(T) == 4) {
            float* omin = (float*)A.omin;
            float* omax = (float*)A.omax;
            omin[k] = lo == LM_NONE ? NAN : lm_dec32((uint32_t)(lo >> 32));
            omax[k] = hi == LM_NONE ? NAN : lm_dec32(~(uint32_t)(hi >> 32));
            A.pmin[k] = lo == LM_NONE ? -1 : (long long)(uint32_t)lo;
            A.pmax[k] = hi == LM_NONE ? -1 : (long long)(uint32_t)hi;
        } else {
            double* omin = (double*)A.omin;
            double* omax = (double*)A.omax;
            omin[k] = lo == LM_NONE ? (double)NAN : lm_dec64(lo);
            omax[k] = hi == LM_NONE ? (double)NAN : lm_dec64(~hi);    // (the positions: the POS launch wrote them)
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
int64_t lm_voxels(int64_t nz, int64_t ny, int64_t nx) {               // saturates at INT64_MAX / 4 (the shape is positive)
    const int64_t cap = INT64_MAX / 4;
    if (ny > cap / nz) return cap;
    const int64_t a = nz * ny;
    return nx > cap / a ? cap : a * nx;
}

unsigned lm_grid(int64_t n, int64_t per_block) {
    const int64_t b = (n + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b < LM_MAX_BLOCKS ? b : LM_MAX_BLOCKS));
}

struct LmBuf { const void* p; int64_t bytes; const char* name; };

bool lm_overlap(const LmBuf& a, const LmBuf& b) {
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a0 < b0 + (uintptr_t)b.bytes && b0 < a0 + (uintptr_t)a.bytes;
}

size_t lm_keys_bytes(int64_t nlabels) { return spc_ws_round(sizeof(unsigned long long) * (size_t)(nlabels + 1)); }

template <typename T, unsigned W>
void lm_launch_want(const LmArgs<T>& A, unsigned grid, hipStream_t st) {
    hipLaunchKernelGGL((lm_kernel<T, W, false>), dim3(grid), dim3(LM_BLOCK), 0, st, A);
}

template <typename T>
void lm_launch(unsigned want, const LmArgs<T>& A, unsigned grid, hipStream_t st) {
    switch (want) {                                                   // one kernel per set of groups
#define LM_CASE(w) case w: lm_launch_want<T, w>(A, grid, st); break;
        LM_CASE(1) LM_CASE(2) LM_CASE(3) LM_CASE(4) LM_CASE(5) LM_CASE(6) LM_CASE(7) LM_CASE(8)
        LM_CASE(9) LM_CASE(10) LM_CASE(11) LM_CASE(12) LM_CASE(13) LM_CASE(14) LM_CASE(15)
#undef LM_CASE
        default: break;
    }
}

template <typename T>
int lm_run(int device, void* stream, const typename SpcAbi<T>::cube* cube, const typename SpcAbi<T>::mask* mask,
           const int32_t* d_labels, int64_t nlabels, const double* d_origin, uint32_t want, const spc_label_measure_outputs* out,
           void* d_workspace, size_t workspace_bytes) {
    int rc = spc_check_cube_any_order(cube);
    if (rc) return rc;
    const int64_t nz = cube->nz, ny = cube->ny, nx = cube->nx, n = lm_voxels(nz, ny, nx);
    if (n > LM_MAX_VOXELS) {
        spc_set_error("%lld x %lld x %lld voxels: linear indices are int32, at most 2^31 - 1 voxels are measured", (long long)nz,
                      (long long)ny, (long long)nx);
        return SPC_ERR_UNSUPPORTED;
    }
    SPC_REQUIRE(d_labels != nullptr, "d_labels is NULL");
    SPC_REQUIRE(out != nullptr, "out is NULL");
    SPC_REQUIRE(nlabels >= 0 && nlabels <= LM_MAX_VOXELS, "nlabels must be 0 to 2^31 - 1 (got %lld)", (long long)nlabels);
    SPC_REQUIRE(want != 0u && (want & ~LM_ALL) == 0u, "want must be a non-empty set of SPC_MEASURE_* bits (got 0x%x)", want);
    LmArgs<T> A{};
    rc = spc_mask_to_dev<T>(mask, cube, &A.M);
    if (rc) return rc;
    if (!(A.M.flags & SPC_MASK_ARRAY)) A.M.arr = nullptr;
    const int64_t nt = nlabels + 1, cext = (nz - 1) * cube->plane_stride + (ny - 1) * cube->row_stride + nx;
    // d_labels, 2 + 4 + 1 + 1 tables, the workspace, the cube, the mask array, the origins
    constexpr int LM_MAX_BUFS = 13;
    LmBuf bufs[LM_MAX_BUFS];
    int nb = 0;
    auto push = [&](const void* p, int64_t bytes, const char* name) {          // never past the list: nb is checked below
        if (nb < LM_MAX_BUFS) bufs[nb] = LmBuf{p, bytes, name};
        ++nb;
    };
    push(d_labels, 4 * n, "d_labels");
    const int first_out = nb;
    if (want & SPC_MEASURE_SUMS) {
        SPC_REQUIRE(out->d_count != nullptr && out->d_sums != nullptr, "SPC_MEASURE_SUMS: d_count or d_sums is NULL");
        push(out->d_count, 8 * nt, "d_count");
        push(out->d_sums, 16 * nt, "d_sums");
    }
    if (want & SPC_MEASURE_EXTREMA) {
        SPC_REQUIRE(out->d_min != nullptr && out->d_max != nullptr && out->d_min_pos != nullptr && out->d_max_pos != nullptr,
                    "SPC_MEASURE_EXTREMA: d_min, d_max, d_min_pos or d_max_pos is NULL");
        push(out->d_min, (int64_t)sizeof(T) * nt, "d_min");
        push(out->d_max, (int64_t)sizeof(T) * nt, "d_max");
        push(out->d_min_pos, 8 * nt, "d_min_pos");
        push(out->d_max_pos, 8 * nt, "d_max_pos");
    }
    if (want & SPC_MEASURE_FIRST) {
        SPC_REQUIRE(out->d_first != nullptr, "SPC_MEASURE_FIRST: d_first is NULL");
        push(out->d_first, 32 * nt, "d_first");
    }
    if (want & SPC_MEASURE_SECOND) {
        SPC_REQUIRE(out->d_second != nullptr, "SPC_MEASURE_SECOND: d_second is NULL");
        push(out->d_second, 48 * nt, "d_second");
    }
    const size_t need = spc_label_measure_workspace_bytes(nlabels, want);
    SPC_REQUIRE(d_workspace != nullptr && workspace_bytes >= need,
                "d_workspace too small: this call needs the %zu bytes spc_label_measure_workspace_bytes returns", need);
    SpcWorkspace ws(d_workspace, workspace_bytes);
    SPC_WS_TAKE(d_bad, ws, uint32_t, 1);
    unsigned long long* d_kmin = nullptr;
    unsigned long long* d_kmax = nullptr;
    if (want & SPC_MEASURE_EXTREMA) {
        SPC_WS_TAKE(kmin_, ws, unsigned long long, nt);
        SPC_WS_TAKE(kmax_, ws, unsigned long long, nt);
        d_kmin = kmin_; d_kmax = kmax_;
    }
    push(d_workspace, (int64_t)ws.used, "d_workspace");
    // what is only read: the cube, the mask array (as far as its strides reach), the origins
    const int first_in = nb;
    push(cube->d_data, (int64_t)sizeof(T) * cext, "the cube");
    if (A.M.arr) push(A.M.arr, (nz - 1) * A.M.plane_stride + (ny - 1) * A.M.row_stride + nx, "the mask array");
    if (d_origin) push(d_origin, 32 * nt, "d_origin");
    SPC_REQUIRE(nb <= LM_MAX_BUFS, "internal: %d buffers to check, room for %d", nb, LM_MAX_BUFS);
    // every written buffer against every other buffer
    for (int a = first_out; a < first_in; ++a)                        // bound: nb <= LM_MAX_BUFS
        for (int b = 0; b < nb; ++b)
            SPC_REQUIRE(a == b || !lm_overlap(bufs[a], bufs[b]), "%s overlaps %s", bufs[a].name, bufs[b].name);

    A.data = cube->d_data; A.rs = cube->row_stride; A.ps = cube->plane_stride;
    A.L = d_labels; A.n = n; A.nlabels = nlabels; A.ny = (uint32_t)ny; A.nx = (uint32_t)nx;
    A.contig = A.rs == nx && A.ps == ny * nx && (!A.M.arr || (A.M.row_stride == nx && A.M.plane_stride == ny * nx));
    A.origin = d_origin;
    A.count = reinterpret_cast<unsigned long long*>(out->d_count); A.sums = out->d_sums;
    A.kmin = d_kmin; A.kmax = d_kmax; A.vmin = nullptr; A.vmax = nullptr;
    A.first = out->d_first; A.second = out->d_second; A.bad = d_bad;
    A.omin = out->d_min; A.omax = out->d_max;
    A.pmin = reinterpret_cast<long long*>(out->d_min_pos); A.pmax = reinterpret_cast<long long*>(out->d_max_pos);

    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    // a wave walks chunks x 64 CONSECUTIVE voxels a round: the longer the walk, the more rows of a label it adds up before an
    // atomic leaves it; as long as that still leaves LM_MAX_BLOCKS blocks
    int chunks = LM_MIN_CHUNKS;
    while (chunks < LM_MAX_CHUNKS && n / ((int64_t)LM_BLOCK * chunks * 2) >= LM_MAX_BLOCKS) chunks *= 2;       // bound: 4 doublings
    A.chunks = chunks;
    const unsigned gt = lm_grid(nt, LM_BLOCK), gv = lm_grid(n, (int64_t)LM_BLOCK * chunks);
    hipLaunchKernelGGL(lm_init_kernel<T>, dim3(gt), dim3(LM_BLOCK), 0, st, A, want);
    SPC_LAUNCH_CHECK();
    lm_launch<T>(want, A, gv, st);
    SPC_LAUNCH_CHECK();
    if (want & SPC_MEASURE_EXTREMA) {
        if constexpr (sizeof(T) == 8) {                               // the first voxel that holds its label's extreme
            LmArgs<T> P = A;
            P.vmin = d_kmin; P.vmax = d_kmax;
            P.kmin = reinterpret_cast<unsigned long long*>(out->d_min_pos);
            P.kmax = reinterpret_cast<unsigned long long*>(out->d_max_pos);
            hipLaunchKernelGGL((lm_kernel<T, SPC_MEASURE_EXTREMA, true>), dim3(gv), dim3(LM_BLOCK), 0, st, P);
            SPC_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(lm_finish_kernel<T>, dim3(gt), dim3(LM_BLOCK), 0, st, A);
        SPC_LAUNCH_CHECK();
    }
    uint32_t bad = 0;
    SPC_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, st));
    SPC_HIP(hipStreamSynchronize(st));
    SPC_REQUIRE(bad == 0u, "d_labels holds a label outside 0 ... %lld: those voxels were skipped", (long long)nlabels);
    return SPC_OK;
}

}  // namespace

extern "C" {

size_t spc_label_measure_workspace_bytes(int64_t nlabels, uint32_t want) {
    if (nlabels < 0 || nlabels > LM_MAX_VOXELS) return 0;
    // the flag, the two key tables of the extrema; a slice may start up to 255 bytes into the workspace
    return spc_ws_round(sizeof(uint32_t)) + ((want & SPC_MEASURE_EXTREMA) ? 2 * lm_keys_bytes(nlabels) : 0) + 256;
}

int spc_label_measure_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, const int32_t* d_labels,
                          int64_t nlabels, const double* d_origin, uint32_t want, const spc_label_measure_outputs* out,
                          void* d_workspace, size_t workspace_bytes) {
    return lm_run<float>(device, stream, cube, mask, d_labels, nlabels, d_origin, want, out, d_workspace, workspace_bytes);
}

int spc_label_measure_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, const int32_t* d_labels,
                          int64_t nlabels, const double* d_origin, uint32_t want, const spc_label_measure_outputs* out,
                          void* d_workspace, size_t workspace_bytes) {
    return lm_run<double>(device, stream, cube, mask, d_labels, nlabels, d_origin, want, out, d_workspace, workspace_bytes);
}

}  // extern "C"
