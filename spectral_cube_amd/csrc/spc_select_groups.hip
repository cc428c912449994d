// Order statistics over TWO axes at once: median / percentile / mad_std with axis=(1, 2) (one result per channel: the
// noise spectrum a signal mask is built from) or axis=(0, 2) (one per row index y).  Replaces
// BaseSpectralCube.median / percentile (spectral_cube/spectral_cube.py:1172-1257: apply_numpy_function(np.nanmedian /
// np.nanpercentile, axis=pair)) and mad_std (:730-764, how='slice' with a two-axis tuple), which partition every plane on
// the host.
//
// The whole-cube selection of spc_select.hip (spc_percentile_global_f32), batched: a GROUP is all samples that share the
// index along the kept axis, and every group descends the bytes of its own order-preserving key at once.
//   * count (4 passes, one per key byte): a block takes one piece of ONE group at a time - a run of a contiguous plane, or
//     some of the group's rows - counts the next byte of the samples whose key matches the group's prefix in a 256-bin LDS
//     histogram (16 interleaved copies, as gselect_kernel) and flushes it into hist[group][256] with 64-bit atomics.
//   * walk (after each count): one wave per group walks its 256 counters, updates the group's state on the device
//     (prefix, remaining rank, n, below, eq) and clears the counters for the next pass.  The host never sees a counter.
//   * next key (a fifth pass, always launched): blocks skip every group whose upper order statistic is the selected key
//     itself, so only the groups that interpolate between two different values are read again.
//   * finish: numpy's rule on the two keys, one float32 per group.
// Nothing comes back to the host: the call queues its kernels on the caller's stream and returns (no synchronisation), so
// the median of a mad_std is the centre of its second call without leaving the device.
#include "spc_common.h"
#include <algorithm>

namespace {

// (the key of spc_select.hip: IEEE bits with the sign flipped / all bits of a negative flipped - unsigned order = float order)
__device__ __forceinline__ uint32_t gkey(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float gunkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

typedef float f32x4g __attribute__((ext_vector_type(4)));

// what a group knows about its descent; every field is written by the first walk (nothing is assumed of the workspace)
struct GroupState {
    unsigned long long n, k, khi, below, eq;
    double frac;
    uint32_t prefix, next;
    int need_next, pad;
};

struct GroupArgs {
    const float* cube;
    MaskDev mask;
    int64_t ngroups;
    int64_t gstride, rstride;              // group g, row r of it: cube + g * gstride + r * rstride (mask: m_gstride / m_rstride)
    int64_t m_gstride, m_rstride;
    int64_t nrows, rowlen;                 // rows of a group and their length; a contiguous plane is ONE row of ny * nx
    int64_t nseg, seg;                     // pieces per group; samples (nrows == 1) or rows per piece
    uint32_t pmask;
    int shift;
    const float* center;                   // NULL, or one centre per group
    unsigned long long* hist;              // [ngroups][256]
    GroupState* state;                     // [ngroups]
};

constexpr int kCopies = 16;

// MODE 0: count the key byte at `shift` under the group's prefix; MODE 1: the smallest key above the prefix
template <bool ARR, int MODE>
__global__ __launch_bounds__(256) void group_count_kernel(const GroupArgs A) {
    __shared__ uint32_t lh[256 * kCopies];
    __shared__ uint32_t s_min;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int copy = t & (kCopies - 1);
    if (MODE == 0) {
        for (int i = t; i < 256 * kCopies; i += 256) lh[i] = 0u;
    }
    const int64_t nitems = A.ngroups * A.nseg;
    for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int64_t g = item / A.nseg, s = item - g * A.nseg;
        // (block-uniform: the state was written by the walk before this launch)
        const bool first = MODE == 0 && A.pmask == 0u;
        if (!first && A.state[g].n == 0ull) continue;
        if (MODE == 1 && A.state[g].need_next == 0) continue;
        const uint32_t prefix = first ? 0u : A.state[g].prefix;
        const bool has_center = A.center != nullptr;
        const float center = has_center ? A.center[g] : 0.f;
        if (MODE == 1 && t == 0) s_min = 0xffffffffu;
        __syncthreads();                    // the cleared bins / s_min; the previous item's flush has read its bins
        uint32_t mymin = 0xffffffffu;
        auto take = [&](float v, unsigned mk) {
            bool ok = spc_pred_valid(A.mask, v) & (mk != 0);
            if (has_center) { v = __builtin_fabsf(v - center); ok = ok & (v == v); }      // (inf - inf, a NaN centre: no sample)
            if (!ok) return;
            const uint32_t k = gkey(v);
            if (MODE == 0) {
                if ((k & A.pmask) == prefix) atomicAdd(&lh[((k >> A.shift) & 0xffu) * kCopies + copy], 1u);
            } else {
                if (k > prefix) mymin = min(mymin, k);
            }
        };
        const float* gp = A.cube + g * A.gstride;
        const uint8_t* gm = ARR ? A.mask.arr + g * A.m_gstride : nullptr;
        if (A.nrows == 1) {
            // a piece [a, b) of the group's one run; `seg` is a multiple of 4, so the piece is aligned as the run is
            const int64_t a = s * A.seg, b = spc_min64(a + A.seg, A.rowlen);
            const float* p = gp + a;
            const uint8_t* pm = ARR ? gm + a : nullptr;
            const int64_t len = b - a;
            const bool al = ((((uintptr_t)p) & 15) == 0) && (!ARR || ((((uintptr_t)pm) & 3) == 0));
            const int64_t n4 = al ? len / 4 : 0;
            for (int64_t i = t; i < n4; i += 256) {
                const f32x4g v = __builtin_nontemporal_load(reinterpret_cast<const f32x4g*>(p) + i);
                const uint32_t m = ARR ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(pm) + i) : 0x01010101u;
#pragma unroll
                for (int c = 0; c < 4; ++c) take(v[c], (m >> (8 * c)) & 0xffu);
            }
            for (int64_t j = n4 * 4 + t; j < len; j += 256) take(p[j], ARR ? pm[j] : 1u);
        } else {
            // rows [r0, r1) of the group, a wave per row
            const int64_t r0 = s * A.seg, r1 = spc_min64(r0 + A.seg, A.nrows);
            for (int64_t r = r0 + wave; r < r1; r += 4) {
                const float* p = gp + r * A.rstride;
                const uint8_t* pm = ARR ? gm + r * A.m_rstride : nullptr;
                const bool al = ((((uintptr_t)p) & 15) == 0) && (!ARR || ((((uintptr_t)pm) & 3) == 0));
                const int64_t n4 = al ? A.rowlen / 4 : 0;
                for (int64_t i = lane; i < n4; i += 64) {
                    const f32x4g v = __builtin_nontemporal_load(reinterpret_cast<const f32x4g*>(p) + i);
                    const uint32_t m = ARR ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(pm) + i) : 0x01010101u;
#pragma unroll
                    for (int c = 0; c < 4; ++c) take(v[c], (m >> (8 * c)) & 0xffu);
                }
                for (int64_t j = n4 * 4 + lane; j < A.rowlen; j += 64) take(p[j], ARR ? pm[j] : 1u);
            }
        }
        if (MODE == 0) {
            __syncthreads();
            unsigned long long tot = 0;
#pragma unroll
            for (int c = 0; c < kCopies; ++c) { tot += lh[t * kCopies + c]; lh[t * kCopies + c] = 0u; }     // (cleared for the next item)
            if (tot) atomicAdd(&A.hist[g * 256 + t], tot);
        } else {
            if (mymin != 0xffffffffu) atomicMin(&s_min, mymin);
            __syncthreads();
            if (t == 0 && s_min != 0xffffffffu) atomicMin(&A.state[g].next, s_min);
            __syncthreads();                // s_min is reset by the next item
        }
    }
}

// One wave per group (4 groups per block): lane l owns counters 4 l .. 4 l + 3.  pass 0 also turns the group's total
// into the two ranks of numpy's 'linear' percentile; the last pass decides whether the upper statistic is another key.
__global__ __launch_bounds__(256) void group_walk_kernel(unsigned long long* hist, GroupState* state, int64_t ngroups, int pass, double q) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= ngroups) return;               // (wave-uniform)
    unsigned long long* h = hist + g * 256 + 4 * lane;
    unsigned long long c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = h[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i] = 0ull;          // the next pass counts into cleared bins
    const unsigned long long mine = c[0] + c[1] + c[2] + c[3];
    unsigned long long incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    const unsigned long long total = __shfl(incl, 63, 64);
    GroupState* S = state + g;
    // every lane holds the group's state; ONE lane stores it (no two lanes of the wave write or read-after-write a word)
    GroupState N;
    if (pass == 0) {
        N.n = total; N.k = 0ull; N.khi = 0ull; N.below = 0ull; N.eq = 0ull; N.frac = 0.0;
        N.prefix = 0u; N.next = 0xffffffffu; N.need_next = 0; N.pad = 0;
        if (total == 0ull) {
            if (lane == 0) *S = N;
            return;
        }
        const double pos = q / 100.0 * (double)(total - 1);
        const double fl = floor(pos);
        N.k = (unsigned long long)fl;
        N.khi = min((unsigned long long)ceil(pos), total - 1);
        N.frac = pos - fl;
    } else {
        N = *S;
        if (N.n == 0ull) return;
    }
    // the lane whose four counters hold rank k of the current bin (k < the bin's total: exactly one)
    const unsigned long long excl = incl - mine;
    if (N.k >= excl && N.k < incl) {
        unsigned long long kk = N.k - excl, bl = N.below + excl;
        int d = 0;
        while (d < 3 && kk >= c[d]) { kk -= c[d]; bl += c[d]; ++d; }
        N.prefix |= (uint32_t)(4 * lane + d) << (24 - 8 * pass);
        N.k = kk;
        N.below = bl;
        N.eq = c[d];
        if (pass == 3) N.need_next = (N.khi >= bl + c[d]) ? 1 : 0;         // the upper statistic is the next larger value
        *S = N;
    }
}

__global__ __launch_bounds__(256) void group_finish_kernel(const GroupState* state, int64_t ngroups, double q, float scale, float* out) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= ngroups) return;
    const GroupState S = state[g];
    float res = NAN;
    if (S.n > 0ull) {
        const double a = (double)gunkey(S.prefix), b = (double)gunkey(S.need_next ? S.next : S.prefix);
        // spc_percentile_global_f32's rule (numpy's 'linear': the median of equal values is that value, the mean of two
        // for an even count), the scale as spc_percentile_axis0_f32 applies it, rounded once
        res = (float)(((q == 50.0 && a == b) ? a : (S.frac == 0.5 ? 0.5 * (a + b) : a + (b - a) * S.frac)) * (double)scale);
    }
    out[g] = res;
}

}  // namespace

extern "C" size_t spc_percentile_groups_workspace_bytes(int64_t ngroups) {
    const size_t g = ngroups > 0 ? (size_t)ngroups : 0;
    return spc_ws_round(sizeof(unsigned long long) * 256 * g) + spc_ws_round(sizeof(GroupState) * g) + 256;
}

extern "C" int spc_percentile_groups_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int keep_axis,
                                         double q, const float* d_center, float scale, float* d_out,
                                         void* d_workspace, size_t workspace_bytes) {
    int rc = spc_check_cube(cube);
    if (rc) return rc;
    SPC_REQUIRE(keep_axis == 0 || keep_axis == 1, "keep_axis must be 0 (one result per plane) or 1 (one per row index)");
    SPC_REQUIRE(d_out != nullptr, "d_out is NULL");
    SPC_REQUIRE(q >= 0.0 && q <= 100.0, "Percentiles must be in the range [0, 100]");
    GroupArgs A{};
    rc = spc_mask_to_dev(mask, cube, &A.mask);
    if (rc) return rc;
    const bool arr = (A.mask.flags & SPC_MASK_ARRAY) != 0;
    const int64_t nz = cube->nz, ny = cube->ny, nx = cube->nx;
    A.cube = cube->d_data;
    A.center = d_center;
    A.ngroups = keep_axis == 0 ? nz : ny;
    if (keep_axis == 0) {
        A.gstride = cube->plane_stride; A.rstride = cube->row_stride;
        A.m_gstride = A.mask.plane_stride; A.m_rstride = A.mask.row_stride;
        const bool run = cube->row_stride == nx && (!arr || A.mask.row_stride == nx);      // the plane is one run of ny * nx
        A.nrows = run ? 1 : ny;
        A.rowlen = run ? ny * nx : nx;
    } else {
        A.gstride = cube->row_stride; A.rstride = cube->plane_stride;
        A.m_gstride = A.mask.row_stride; A.m_rstride = A.mask.plane_stride;
        A.nrows = nz;
        A.rowlen = nx;
    }
    // pieces per group: enough blocks to fill the device when the groups are few, at least ~8192 samples each
    const int64_t group_size = A.nrows * A.rowlen;
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>((4096 + A.ngroups - 1) / A.ngroups, (group_size + 8191) / 8192));
    if (A.nrows == 1) {
        A.seg = ((A.rowlen + want - 1) / want + 3) / 4 * 4;
        A.nseg = (A.rowlen + A.seg - 1) / A.seg;
    } else {
        A.seg = (A.nrows + want - 1) / want;
        A.nseg = (A.nrows + A.seg - 1) / A.seg;
    }
    SpcWorkspace ws(d_workspace, workspace_bytes);
    unsigned long long* d_hist = (unsigned long long*)ws.take(sizeof(unsigned long long) * 256 * (size_t)A.ngroups);
    GroupState* d_state = (GroupState*)ws.take(sizeof(GroupState) * (size_t)A.ngroups);
    SPC_REQUIRE(d_hist != nullptr && d_state != nullptr, "d_workspace too small: %lld groups need %zu bytes (spc_percentile_groups_workspace_bytes)",
                (long long)A.ngroups, spc_percentile_groups_workspace_bytes(A.ngroups));
    A.hist = d_hist;
    A.state = d_state;
    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const int64_t nitems = A.ngroups * A.nseg;
    const dim3 grid((unsigned)std::min<int64_t>(nitems, 8192)), wgrid((unsigned)((A.ngroups + 3) / 4));
    // the counters arrive dirty: cleared here once, by every walk afterwards; the state is written by the first walk
    SPC_HIP(hipMemsetAsync(d_hist, 0, sizeof(unsigned long long) * 256 * (size_t)A.ngroups, st));
    for (int pass = 0; pass < 4; ++pass) {
        A.shift = 24 - 8 * pass;
        A.pmask = pass == 0 ? 0u : (0xffffffffu << (A.shift + 8));
        if (arr) hipLaunchKernelGGL((group_count_kernel<true, 0>), grid, dim3(256), 0, st, A);
        else hipLaunchKernelGGL((group_count_kernel<false, 0>), grid, dim3(256), 0, st, A);
        SPC_LAUNCH_CHECK();
        hipLaunchKernelGGL(group_walk_kernel, wgrid, dim3(256), 0, st, d_hist, d_state, A.ngroups, pass, q);
        SPC_LAUNCH_CHECK();
    }
    A.pmask = 0xffffffffu;
    A.shift = 0;
    if (arr) hipLaunchKernelGGL((group_count_kernel<true, 1>), grid, dim3(256), 0, st, A);
    else hipLaunchKernelGGL((group_count_kernel<false, 1>), grid, dim3(256), 0, st, A);
    SPC_LAUNCH_CHECK();
    hipLaunchKernelGGL(group_finish_kernel, dim3((unsigned)((A.ngroups + 255) / 256)), dim3(256), 0, st, d_state, A.ngroups, q, scale, d_out);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}
