// spc_pv_extract.hip - position-velocity diagrams: the spectrum of the filled cube at every point of a path on the sky,
// averaged over parallel lines across the path's width (SpectralCube.to_pvextractor, spectral_cube.py:2506-2513, which hands
// the cube to pvextractor.extract_pv_slice on the host; and the axis-aligned cube[:, j, :]).  The semantics are stated with
// the prototypes in include/spcube_hip.h.
//
// Lanes run along the path: the 64 neighbouring points of a wave fall on few cache lines of a plane, and the stores of a
// channel are coalesced.  A lane's plan for a point of a line - the offsets of its neighbours in the plane and in the mask,
// their weights, whether the point is inside - does not depend on the channel: it is built once per lane when there is
// one line, once per line and batch of channels otherwise (two float64 loads and a dozen operations against PV_ZC x 4
// sample loads).  Blocks split the channels in batches of PV_ZC; a batch reads the mask bytes of all its channels, then
// the samples those include, then does the arithmetic: the loads of a batch are in flight together.  Lines are added in
// index order into one float64 sum per channel held in registers: no atomics, no workspace, no (nz, nlines, npts) array.
// Built with -ffp-contract=off: every product and sum is rounded on its own, so that the result can be restated in numpy.
#include "spc_common.h"

namespace {

constexpr int PV_BLOCK = 128;                 // lanes along the path
constexpr int64_t PV_GRID_LIMIT = 65535;
constexpr int64_t PV_TARGET_BLOCKS = 4096;    // 256 CUs x 16: enough blocks to fill the device from a short path

template <typename T>
struct PvArgs {
    const T* in;
    int64_t nz, ny, nx, rs, ps;
    SpcInclude<T> m;
    T fill;
    int64_t npts, nlines;
    const double* xs;
    const double* ys;
    int respect_nan;
    T* out;
    int64_t ors;
    int32_t* count;
    int64_t crs;
};

template <int NB>
struct PvPlan {
    int64_t off[NB], moff[NB];               // element offsets of the neighbours in a plane of the cube / of the mask
    double w[NB];                            // weights; a neighbour of weight 0 is never addressed
    bool inside;
};

// the plan of point p of line l; NB == 1: order 0, NB == 4: order 1
template <typename T, int NB>
__device__ __forceinline__ void pv_plan(const PvArgs<T>& A, int64_t l, int64_t p, PvPlan<NB>& P) {
    const double x = A.xs[l * A.npts + p], y = A.ys[l * A.npts + p];
    P.inside = (x >= 0.0) & (x <= (double)(A.nx - 1)) & (y >= 0.0) & (y <= (double)(A.ny - 1));     // NaN: outside
#pragma unroll
    for (int n = 0; n < NB; ++n) { P.off[n] = 0; P.moff[n] = 0; P.w[n] = 0.0; }
    if (!P.inside) return;
    if constexpr (NB == 1) {
        const int64_t ix = (int64_t)floor(x + 0.5), iy = (int64_t)floor(y + 0.5);
        P.off[0] = iy * A.rs + ix;
        P.moff[0] = iy * A.m.mrs + ix;
        P.w[0] = 1.0;
    } else {
        const double xf = floor(x), yf = floor(y);
        const double fx = x - xf, fy = y - yf;
        const int64_t x0 = (int64_t)xf, y0 = (int64_t)yf;
        const int64_t x1 = spc_min64(x0 + 1, A.nx - 1), y1 = spc_min64(y0 + 1, A.ny - 1);      // (weight 0 where clamped)
        const double gx = 1.0 - fx, gy = 1.0 - fy;
        const int64_t xx[4] = {x0, x1, x0, x1}, yy[4] = {y0, y0, y1, y1};
        const double ww[4] = {gy * gx, gy * fx, fy * gx, fy * fx};
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            P.off[n] = yy[n] * A.rs + xx[n];
            P.moff[n] = yy[n] * A.m.mrs + xx[n];
            P.w[n] = ww[n];
        }
    }
}

// blockIdx.x: PV_BLOCK points of the path; blockIdx.y, strided by gridDim.y: batches of ZC channels
template <typename T, bool LINEAR>
__global__ __launch_bounds__(PV_BLOCK) void pv_extract_kernel(const PvArgs<T> A) {
    constexpr int NB = LINEAR ? 4 : 1, ZC = LINEAR ? 4 : 8;
    const int64_t p = (int64_t)blockIdx.x * PV_BLOCK + threadIdx.x;
    if (p >= A.npts) return;
    const int64_t nbatch = (A.nz + ZC - 1) / ZC;
    const T nan = std::numeric_limits<T>::quiet_NaN();
    PvPlan<NB> P;
    bool planned = false;
    for (int64_t b = blockIdx.y; b < nbatch; b += gridDim.y) {
        const int64_t z0 = b * ZC;
        const int nc = (int)spc_min64(ZC, A.nz - z0);
        double sum[ZC];
        int cnt[ZC];
        T raw[ZC];
#pragma unroll
        for (int c = 0; c < ZC; ++c) { sum[c] = 0.0; cnt[c] = 0; raw[c] = nan; }
        for (int64_t l = 0; l < A.nlines; ++l) {
            if (!planned || A.nlines > 1) {
                pv_plan<T, NB>(A, l, p, P);
                planned = true;
            }
            if (!P.inside) continue;                                    // NaN in every channel: the line does not count
            uint8_t mb[ZC][NB];
            T v[ZC][NB];
#pragma unroll
            for (int c = 0; c < ZC; ++c) {
#pragma unroll
                for (int n = 0; n < NB; ++n) {
                    mb[c][n] = 1;
                    if (A.m.marr && c < nc && P.w[n] != 0.0) mb[c][n] = A.m.marr[(z0 + c) * A.m.mps + P.moff[n]];
                }
            }
#pragma unroll
            for (int c = 0; c < ZC; ++c) {
#pragma unroll
                for (int n = 0; n < NB; ++n) {
                    v[c][n] = A.fill;
                    if (c < nc && P.w[n] != 0.0 && mb[c][n] != 0) {              // mask first: an excluded sample is not fetched
                        const T s = A.in[(z0 + c) * A.ps + P.off[n]];
                        v[c][n] = spc_include(A.m, s, mb[c][n]) ? s : A.fill;
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < ZC; ++c) {
                double val = 0.0;
                bool hole = false;
#pragma unroll
                for (int n = 0; n < NB; ++n) {
                    if (P.w[n] != 0.0) {
                        if (v[c][n] != v[c][n]) hole = true;
                        else val = val + P.w[n] * (double)v[c][n];
                    }
                }
                if (hole && A.respect_nan) continue;
                sum[c] = cnt[c] ? sum[c] + val : val;
                raw[c] = hole ? (T)0 : v[c][0];
                ++cnt[c];
            }
        }
#pragma unroll
        for (int c = 0; c < ZC; ++c) {
            if (c < nc) {
                T o = nan;
                if (cnt[c]) o = (!LINEAR && A.nlines == 1) ? raw[c] : (T)(sum[c] / (double)cnt[c]);
                A.out[(z0 + c) * A.ors + p] = o;
                if (A.count) A.count[(z0 + c) * A.crs + p] = cnt[c];
            }
        }
    }
}

template <typename T>
int pv_entry(int device, void* stream, const typename SpcAbi<T>::cube* cube, const typename SpcAbi<T>::mask* mask, int nan_excluded,
             T fill, int64_t npts, int64_t nlines, const double* d_xs, const double* d_ys, int order, int respect_nan, T* d_out,
             int64_t out_row_stride, int32_t* d_count, int64_t count_row_stride) {
    int rc = spc_check_cube(cube);
    if (rc) return rc;
    SPC_REQUIRE(npts >= 1, "a path needs at least one point (npts = %lld)", (long long)npts);
    SPC_REQUIRE(nlines >= 1, "a path needs at least one line (nlines = %lld)", (long long)nlines);
    SPC_REQUIRE(npts <= (int64_t)0x7fffffff * PV_BLOCK && nlines <= INT64_MAX / npts, "npts %lld x nlines %lld too large",
                (long long)npts, (long long)nlines);
    SPC_REQUIRE(order == 0 || order == 1, "order %d is not built: 0 (nearest) or 1 (bilinear)", order);
    SPC_REQUIRE(d_xs != nullptr && d_ys != nullptr, "d_xs / d_ys is NULL");
    SPC_REQUIRE(d_out != nullptr, "d_out is NULL");
    PvArgs<T> A{};
    rc = spc_include_from(mask, cube, nan_excluded, &A.m);
    if (rc) return rc;
    A.in = cube->d_data;
    A.nz = cube->nz; A.ny = cube->ny; A.nx = cube->nx; A.rs = cube->row_stride; A.ps = cube->plane_stride;
    A.fill = fill;
    A.npts = npts; A.nlines = nlines;
    A.xs = d_xs; A.ys = d_ys;
    A.respect_nan = respect_nan != 0;
    A.out = d_out;
    A.ors = out_row_stride ? out_row_stride : npts;
    A.count = d_count;
    A.crs = count_row_stride ? count_row_stride : npts;
    SPC_REQUIRE(A.ors >= npts, "out_row_stride %lld < npts %lld", (long long)A.ors, (long long)npts);
    SPC_REQUIRE(!d_count || A.crs >= npts, "count_row_stride %lld < npts %lld", (long long)A.crs, (long long)npts);
    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const int64_t zc = order ? 4 : 8;
    const int64_t nbatch = (A.nz + zc - 1) / zc;
    const int64_t gx = (npts + PV_BLOCK - 1) / PV_BLOCK;
    const int64_t gy = spc_min64(spc_min64(nbatch, PV_GRID_LIMIT), (PV_TARGET_BLOCKS + gx - 1) / gx);
    dim3 grid((unsigned)gx, (unsigned)gy);
    if (order) hipLaunchKernelGGL((pv_extract_kernel<T, true>), grid, dim3(PV_BLOCK), 0, st, A);
    else hipLaunchKernelGGL((pv_extract_kernel<T, false>), grid, dim3(PV_BLOCK), 0, st, A);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

}  // namespace

extern "C" {

int spc_pv_extract_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded, float fill,
                       int64_t npts, int64_t nlines, const double* d_xs, const double* d_ys, int order, int respect_nan,
                       float* d_out, int64_t out_row_stride, int32_t* d_count, int64_t count_row_stride) {
    return pv_entry<float>(device, stream, cube, mask, nan_excluded, fill, npts, nlines, d_xs, d_ys, order, respect_nan, d_out,
                           out_row_stride, d_count, count_row_stride);
}

int spc_pv_extract_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded, double fill,
                       int64_t npts, int64_t nlines, const double* d_xs, const double* d_ys, int order, int respect_nan,
                       double* d_out, int64_t out_row_stride, int32_t* d_count, int64_t count_row_stride) {
    return pv_entry<double>(device, stream, cube, mask, nan_excluded, fill, npts, nlines, d_xs, d_ys, order, respect_nan, d_out,
                            out_row_stride, d_count, count_row_stride);
}

}  // extern "C"
