// spc_stats_m2.hip - the second pass of std: per ray, the sum of squared deviations about the ray's OWN mean.
//
// The single-pass form sumsq / n - mean^2 (spc_stats.hip) loses (mean / sigma)^2 ulps of float64: a cube on a pedestal - a
// 1000 K baseline with mK noise, a BITPIX = 32 image near 2^30 - gets a std of noise or 0 from it.  The reference does not
// compute std that way: nanstd (dask_spectral_cube.py:699-710, spectral_cube.py:667-724) takes the mean first and then the
// deviations.  So does this pass.  It reads the count and sum maps that spc_stats_axis left on the device, takes
// c = sum / count of ITS ray (no cube-wide pivot: every spaxel may sit on a baseline of its own), and accumulates
//   s1 = sum (x - c),  s2 = sum (x - c)^2   ->   m2 = s2 - s1^2 / n        (the corrected two-pass form: s1 is only the
// rounding of c, its term removes what that rounding put into s2).  x - c is exact or within an ulp OF THE DEVIATION, so m2
// is good to about n eps64 whatever the pedestal.  Rays merge on the host with m2 = m2_a + m2_b + delta^2 n_a n_b / n (Chan).
//
// The whole cube at once has ONE mean, known from spc_stats_global before this pass: spc_stats_dev_axis takes it as a number
// and writes s1 and s2 of every ray about it; the host adds the rays and forms s2 - s1^2 / n once (nothing to merge).
//
// Plain HBM streams in the shape of the float64 statistics kernels (spc_stats_f64.hip): a lane per output marching z or y,
// a wave per row along x; one template for both sample widths.  std pays a second read of the cube; sum / mean / max / min
// and statistics() keep their one pass.
#include "spc_common.h"

namespace {

template <class T>
struct M2Args {
    const T* p;
    int64_t nz, ny, nx, row_stride, plane_stride;
    SpcMaskDev<T> m;
    const int32_t* cnt;           // the maps of spc_stats_axis along the same axis, under the same mask;
    const double* sum;            // cnt == nullptr: every ray about `center`, s1 -> s1_out, s2 -> m2
    double* m2;
    double center;
    double* s1_out;
};

struct Dev2 { double s1, s2; };

template <class T>
__device__ __forceinline__ void dev_add(Dev2& a, T v, bool ok, double c) {
    const double d = ok ? (double)v - c : 0.0;
    a.s1 += d;
    a.s2 = fma(d, d, a.s2);
}

// an empty ray: NaN like its sum; an infinite sample: inf - inf = NaN, as nanstd gives
__device__ __forceinline__ double m2_finish(const Dev2& a, int n) {
    if (n <= 0) return NAN;
    const double m2 = a.s2 - a.s1 * a.s1 / (double)n;
    return m2 < 0.0 ? 0.0 : m2;
}

// AXIS 0: a lane per (y, x), marching z; AXIS 1: a lane per (z, x), marching y - lanes along x either way
template <class T, int AXIS>
__global__ __launch_bounds__(256) void m2_march_kernel(const M2Args<T> A) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nouter = AXIS == 0 ? A.ny : A.nz;
    if (g >= nouter * A.nx) return;
    const int64_t a = g / A.nx, x = g - a * A.nx;
    const int64_t n = AXIS == 0 ? A.nz : A.ny;
    const bool own = A.cnt != nullptr;
    const int cnt = own ? A.cnt[g] : 0;
    const double c = own ? A.sum[g] / (double)cnt : A.center;
    const bool arr = (A.m.flags & SPC_MASK_ARRAY) != 0;
    const int64_t dstep = AXIS == 0 ? A.plane_stride : A.row_stride, mstep = AXIS == 0 ? A.m.plane_stride : A.m.row_stride;
    const T* pd = A.p + (AXIS == 0 ? a * A.row_stride : a * A.plane_stride) + x;
    const uint8_t* pm = arr ? A.m.arr + (AXIS == 0 ? a * A.m.row_stride : a * A.m.plane_stride) + x : nullptr;
    Dev2 r{0.0, 0.0};
    constexpr int kIn = 8;                                       // samples requested together per lane (clamped into the ray)
    for (int64_t k0 = 0; k0 < n; k0 += kIn) {
        T vv[kIn];
        unsigned mk[kIn];
#pragma unroll
        for (int q = 0; q < kIn; ++q) {
            const int64_t kc = min(k0 + q, n - 1);
            vv[q] = pd[kc * dstep];
            mk[q] = arr ? pm[kc * mstep] : 1u;
        }
#pragma unroll
        for (int q = 0; q < kIn; ++q) dev_add(r, vv[q], (k0 + q < n) & spc_pred_valid(A.m, vv[q]) & (mk[q] != 0u), c);
    }
    if (own) A.m2[g] = m2_finish(r, cnt);
    else { A.s1_out[g] = r.s1; A.m2[g] = r.s2; }
}

// AXIS 2: a wave per row (z, y)
template <class T>
__global__ __launch_bounds__(256) void m2_rows_kernel(const M2Args<T> A) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= A.nz * A.ny) return;
    const int64_t z = row / A.ny, y = row - z * A.ny;
    const bool own = A.cnt != nullptr;
    const int cnt = own ? A.cnt[row] : 0;
    const double c = own ? A.sum[row] / (double)cnt : A.center;
    const bool arr = (A.m.flags & SPC_MASK_ARRAY) != 0;
    const T* pd = A.p + z * A.plane_stride + y * A.row_stride;
    const uint8_t* pm = arr ? A.m.arr + z * A.m.plane_stride + y * A.m.row_stride : nullptr;
    Dev2 r{0.0, 0.0};
    for (int64_t x = threadIdx.x & 63; x < A.nx; x += 64) {
        const T v = pd[x];
        dev_add(r, v, spc_pred_valid(A.m, v) & (!arr || pm[x] != 0), c);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { r.s1 += __shfl_down(r.s1, d, 64); r.s2 += __shfl_down(r.s2, d, 64); }
    if ((threadIdx.x & 63) == 0) {
        if (own) A.m2[row] = m2_finish(r, cnt);
        else { A.s1_out[row] = r.s1; A.m2[row] = r.s2; }
    }
}

template <class T>
int stats_m2_axis(int device, void* stream, const typename SpcAbi<T>::cube* cube, const typename SpcAbi<T>::mask* mask, int axis,
                  const int32_t* d_count, const double* d_sum, double* d_m2, double center = 0.0, double* d_s1 = nullptr) {
    int rc = spc_check_cube(cube);
    if (rc) return rc;
    M2Args<T> A{};
    rc = spc_mask_to_dev(mask, cube, &A.m);
    if (rc) return rc;
    SPC_REQUIRE(axis >= 0 && axis <= 2, "axis must be 0, 1 or 2, got %d", axis);
    if (d_s1) SPC_REQUIRE(d_m2 != nullptr, "d_s1 / d_s2 is NULL");
    else SPC_REQUIRE(d_count != nullptr && d_sum != nullptr && d_m2 != nullptr, "d_count / d_sum / d_m2 is NULL");
    A.p = cube->d_data; A.nz = cube->nz; A.ny = cube->ny; A.nx = cube->nx;
    A.row_stride = cube->row_stride; A.plane_stride = cube->plane_stride;
    A.cnt = d_count; A.sum = d_sum; A.m2 = d_m2; A.center = center; A.s1_out = d_s1;
    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    if (axis == 2) {
        const int64_t nb = (A.nz * A.ny + 3) / 4;
        SPC_REQUIRE(nb < (1LL << 31), "too many rows for one launch");
        hipLaunchKernelGGL(m2_rows_kernel<T>, dim3((unsigned)nb), dim3(256), 0, st, A);
    } else {
        const int64_t n = (axis == 0 ? A.ny : A.nz) * A.nx, nb = (n + 255) / 256;
        SPC_REQUIRE(nb < (1LL << 31), "map too large for one launch");
        if (axis == 0) hipLaunchKernelGGL((m2_march_kernel<T, 0>), dim3((unsigned)nb), dim3(256), 0, st, A);
        else hipLaunchKernelGGL((m2_march_kernel<T, 1>), dim3((unsigned)nb), dim3(256), 0, st, A);
    }
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

}  // namespace

extern "C" {

int spc_stats_m2_axis_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int axis,
                          const int32_t* d_count, const double* d_sum, double* d_m2) {
    return stats_m2_axis<float>(device, stream, cube, mask, axis, d_count, d_sum, d_m2);
}

int spc_stats_m2_axis_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int axis,
                          const int32_t* d_count, const double* d_sum, double* d_m2) {
    return stats_m2_axis<double>(device, stream, cube, mask, axis, d_count, d_sum, d_m2);
}

int spc_stats_dev_axis_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int axis, double center,
                           double* d_s1, double* d_s2) {
    SPC_REQUIRE(d_s1 != nullptr, "d_s1 / d_s2 is NULL");
    return stats_m2_axis<float>(device, stream, cube, mask, axis, nullptr, nullptr, d_s2, center, d_s1);
}

int spc_stats_dev_axis_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int axis, double center,
                           double* d_s1, double* d_s2) {
    SPC_REQUIRE(d_s1 != nullptr, "d_s1 / d_s2 is NULL");
    return stats_m2_axis<double>(device, stream, cube, mask, axis, nullptr, nullptr, d_s2, center, d_s1);
}

}  // extern "C"
