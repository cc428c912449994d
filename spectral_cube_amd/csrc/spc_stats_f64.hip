// spc_stats_f64.hip - statistics of a float64 cube (gfx950): spc_stats_global_f64, spc_stats_axis_f64.
//
// statistics() and the nan-reductions of the reference (dask_spectral_cube.py:641-814; nansum_allbadtonan, :54-59) on the
// float64 samples as they are: count, min, max, sum and sum of squares, compared and added in float64 (spc_stats.hip is
// the float32 twin).  HBM streams with the lanes along x: the whole-cube form deals rows to blocks (two samples per lane
// where the layout allows, spc_pairs_ok_f64) and merges the blocks' records in a fixed order; the per-axis forms march z
// or y with one lane per output, or give a wave a row.
#include "spc_wide.h"

#include <algorithm>

namespace {

struct Rec64 { double n, mn, mx, s, q; };
__device__ __forceinline__ void rec_add(Rec64& r, double v) {
    r.n += 1.0; r.mn = fmin(r.mn, v); r.mx = fmax(r.mx, v); r.s += v; r.q = fma(v, v, r.q);
}
__device__ __forceinline__ void rec_merge(Rec64& a, const Rec64& b) {
    a.n += b.n; a.mn = fmin(a.mn, b.mn); a.mx = fmax(a.mx, b.mx); a.s += b.s; a.q += b.q;
}
__device__ __forceinline__ Rec64 rec_empty() { return Rec64{0.0, INFINITY, -INFINITY, 0.0, 0.0}; }
__device__ __forceinline__ Rec64 rec_shfl_down(const Rec64& r, int d) {
    return Rec64{__shfl_down(r.n, d, 64), __shfl_down(r.mn, d, 64), __shfl_down(r.mx, d, 64), __shfl_down(r.s, d, 64), __shfl_down(r.q, d, 64)};
}
// block of 256: lane partials -> one record in thread 0 (fixed order: the result does not depend on scheduling)
__device__ __forceinline__ Rec64 rec_block_reduce(Rec64 r, Rec64* sh) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const Rec64 o = rec_shfl_down(r, d); rec_merge(r, o); }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[w] = r;
    __syncthreads();
    if (threadIdx.x == 0) for (int k = 1; k < (int)(blockDim.x >> 6); ++k) rec_merge(r, sh[k]);
    return r;
}

// rows of the cube (nz * ny of them) dealt to the blocks round robin; partial[b] = the block's record
// VEC = 2: rows of an even length on 16-byte boundaries - a lane asks for two adjacent samples (16 bytes, and 2 mask bytes) per
// request, four requests together: a wave moves 1 KiB per instruction where the one-sample form moves 512 bytes
template <int VEC>
__global__ __launch_bounds__(256) void stats64_global_kernel(const Cube64 C, const MaskDev64 M, Rec64* partial) {
    __shared__ Rec64 sh[4];
    Rec64 r = rec_empty();
    const int64_t nrows = C.nz * C.ny;
    const bool arr = (M.flags & SPC_MASK_ARRAY) != 0;
    constexpr int kIn = 4;                                       // requests together per lane (clamped into the row)
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    for (int64_t row = blockIdx.x; row < nrows; row += gridDim.x) {
        const int64_t z = row / C.ny, y = row - z * C.ny;
        const double* pd = C.p + z * C.plane_stride + y * C.row_stride;
        const uint8_t* pm = arr ? M.arr + z * M.plane_stride + y * M.row_stride : nullptr;
        for (int64_t x0 = (int64_t)threadIdx.x * VEC; x0 < C.nx; x0 += (int64_t)blockDim.x * kIn * VEC) {
            double vv[kIn][VEC];
            unsigned mk[kIn];
#pragma unroll
            for (int q = 0; q < kIn; ++q) {
                const int64_t xc = min(x0 + (int64_t)q * blockDim.x * VEC, C.nx - VEC);
                if (VEC == 2) {
                    const f64x2 t = *reinterpret_cast<const f64x2*>(pd + xc);
                    vv[q][0] = t.x; vv[q][VEC - 1] = t.y;
                    mk[q] = arr ? (unsigned)*reinterpret_cast<const uint16_t*>(pm + xc) : 0x0101u;
                } else {
                    vv[q][0] = pd[xc];
                    mk[q] = arr ? pm[xc] : 1u;
                }
            }
#pragma unroll
            for (int q = 0; q < kIn; ++q) {
                const bool in = x0 + (int64_t)q * blockDim.x * VEC < C.nx;      // (VEC = 2: nx is even, both samples or neither)
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    if (in && spc_pred_valid(M, vv[q][e]) && ((mk[q] >> (8 * e)) & 0xffu) != 0u) rec_add(r, vv[q][e]);
            }
        }
    }
    r = rec_block_reduce(r, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}
__global__ __launch_bounds__(256) void stats64_finish_kernel(const Rec64* partial, int nblocks, double* out) {
    __shared__ Rec64 sh[4];
    Rec64 r = rec_empty();
    for (int k = threadIdx.x; k < nblocks; k += blockDim.x) rec_merge(r, partial[k]);
    r = rec_block_reduce(r, sh);
    if (threadIdx.x == 0) {
        out[0] = r.n; out[1] = r.n > 0 ? r.mn : NAN; out[2] = r.n > 0 ? r.mx : NAN; out[3] = r.s; out[4] = r.q;
    }
}

struct StatOut64 {
    int32_t* count; double* mn; double* mx; double* sum; double* sumsq;
};
__device__ __forceinline__ void stat_store(const StatOut64& O, int64_t o, const Rec64& r) {
    const bool any = r.n > 0;
    if (O.count) O.count[o] = (int32_t)r.n;
    if (O.mn) O.mn[o] = any ? r.mn : NAN;
    if (O.mx) O.mx[o] = any ? r.mx : NAN;
    if (O.sum) O.sum[o] = any ? r.s : NAN;              // nansum_allbadtonan (dask_spectral_cube.py:54-59)
    if (O.sumsq) O.sumsq[o] = any ? r.q : NAN;
}
// AXIS 0: a lane per (y, x), marching z; AXIS 1: a lane per (z, x), marching y - lanes along x either way
template <int AXIS>
__global__ __launch_bounds__(256) void stats64_march_kernel(const Cube64 C, const MaskDev64 M, const StatOut64 O) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nouter = AXIS == 0 ? C.ny : C.nz;
    if (g >= nouter * C.nx) return;
    const int64_t a = g / C.nx, x = g - a * C.nx;
    const int64_t n = AXIS == 0 ? C.nz : C.ny;
    Rec64 r = rec_empty();
    const bool arr = (M.flags & SPC_MASK_ARRAY) != 0;
    const int64_t dstep = AXIS == 0 ? C.plane_stride : C.row_stride, mstep = AXIS == 0 ? M.plane_stride : M.row_stride;
    const double* pd = C.p + (AXIS == 0 ? a * C.row_stride : a * C.plane_stride) + x;
    const uint8_t* pm = arr ? M.arr + (AXIS == 0 ? a * M.row_stride : a * M.plane_stride) + x : nullptr;
    constexpr int kIn = 8;                                       // samples requested together per lane (clamped into the ray)
    for (int64_t k0 = 0; k0 < n; k0 += kIn) {
        double vv[kIn];
        unsigned mk[kIn];
#pragma unroll
        for (int q = 0; q < kIn; ++q) {
            const int64_t kc = min(k0 + q, n - 1);
            vv[q] = pd[kc * dstep];
            mk[q] = arr ? pm[kc * mstep] : 1u;
        }
#pragma unroll
        for (int q = 0; q < kIn; ++q)
            if (k0 + q < n && spc_pred_valid(M, vv[q]) && mk[q] != 0u) rec_add(r, vv[q]);
    }
    stat_store(O, g, r);
}
// AXIS 2: a wave per row (z, y)
__global__ __launch_bounds__(256) void stats64_rows_kernel(const Cube64 C, const MaskDev64 M, const StatOut64 O) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= C.nz * C.ny) return;
    const int64_t z = row / C.ny, y = row - z * C.ny;
    Rec64 r = rec_empty();
    for (int64_t x = threadIdx.x & 63; x < C.nx; x += 64) {
        double v;
        if (inc64(C, M, z, y, x, v)) rec_add(r, v);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const Rec64 o = rec_shfl_down(r, d); rec_merge(r, o); }
    if ((threadIdx.x & 63) == 0) stat_store(O, row, r);
}

}  // namespace

size_t spc_ws_stats_global_f64(void) { return spc_ws_round(sizeof(Rec64) * 4096) + spc_ws_round(5 * sizeof(double)) + 256; }

extern "C" {

int spc_stats_global_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, double* h_stats,
                         void* d_workspace, size_t workspace_bytes) {
    Cube64 C; MaskDev64 M;
    int rc = cube64_args(cube, mask, &C, &M);
    if (rc) return rc;
    SPC_REQUIRE(h_stats != nullptr, "h_stats is NULL");
    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    SpcWorkspace ws(d_workspace, workspace_bytes);
    const int nblocks = (int)std::min<int64_t>(4096, C.nz * C.ny);
    SPC_WS_TAKE(d_partial, ws, Rec64, 4096);
    SPC_WS_TAKE(d_out, ws, double, 5);
    const bool vec2 = spc_pairs_ok_f64(cube, M);
    if (vec2) hipLaunchKernelGGL(stats64_global_kernel<2>, dim3((unsigned)nblocks), dim3(256), 0, st, C, M, d_partial);
    else hipLaunchKernelGGL(stats64_global_kernel<1>, dim3((unsigned)nblocks), dim3(256), 0, st, C, M, d_partial);
    SPC_LAUNCH_CHECK();
    hipLaunchKernelGGL(stats64_finish_kernel, dim3(1), dim3(256), 0, st, d_partial, nblocks, d_out);
    SPC_LAUNCH_CHECK();
    SPC_HIP(hipMemcpyAsync(h_stats, d_out, 5 * sizeof(double), hipMemcpyDeviceToHost, st));
    SPC_HIP(hipStreamSynchronize(st));
    return SPC_OK;
}

int spc_stats_axis_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int axis,
                       const spc_stats_outputs_f64* out) {
    Cube64 C; MaskDev64 M;
    int rc = cube64_args(cube, mask, &C, &M);
    if (rc) return rc;
    SPC_REQUIRE(out != nullptr, "outputs struct is NULL");
    SPC_REQUIRE(axis >= 0 && axis <= 2, "axis must be 0, 1 or 2, got %d", axis);
    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const StatOut64 O{out->d_count, out->d_min, out->d_max, out->d_sum, out->d_sumsq};
    if (axis == 2) {
        const int64_t nb = (C.nz * C.ny + 3) / 4;
        SPC_REQUIRE(nb < (1LL << 31), "too many rows for one launch");
        hipLaunchKernelGGL(stats64_rows_kernel, dim3((unsigned)nb), dim3(256), 0, st, C, M, O);
    } else {
        const int64_t n = (axis == 0 ? C.ny : C.nz) * C.nx, nb = (n + 255) / 256;
        SPC_REQUIRE(nb < (1LL << 31), "map too large for one launch");
        if (axis == 0) hipLaunchKernelGGL(stats64_march_kernel<0>, dim3((unsigned)nb), dim3(256), 0, st, C, M, O);
        else hipLaunchKernelGGL(stats64_march_kernel<1>, dim3((unsigned)nb), dim3(256), 0, st, C, M, O);
    }
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

}  // extern "C"
