// spc_convert_f64.hip - three elementwise helpers for float64 cubes (gfx950): spc_scale_f64, spc_narrow_f64_to_f32,
// spc_mask_include_f64.
//
// spc_scale_f64 multiplies in place (the Jy/beam area ratio of convolve_to, dask_spectral_cube.py:1445-1464);
// spc_mask_include_f64 is MaskBase.include (spectral_cube/masks.py:105-116) with the thresholds compared in float64,
// the float64 side of spc_mask_include_u8; spc_narrow_f64_to_f32 has no line of the reference behind it: it makes the
// float32 copy that an operator without a float64 form is given.  One lane per sample, one load and one store each.
#include "spc_wide.h"

#include <algorithm>

namespace {

__global__ __launch_bounds__(256) void scale64_kernel(double* p, int64_t n, double f) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] *= f;
}
__global__ __launch_bounds__(256) void narrow64_kernel(const Cube64 C, float* out, int64_t out_row_stride, int64_t out_plane_stride) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t y = blockIdx.y, z = blockIdx.z;
    if (x >= C.nx) return;
    out[z * out_plane_stride + y * out_row_stride + x] = (float)C.p[z * C.plane_stride + y * C.row_stride + x];
}
__global__ __launch_bounds__(256) void include64_kernel(const Cube64 C, const MaskDev64 M, int nan_excluded, uint8_t* out) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t y = blockIdx.y, z = blockIdx.z;
    if (x >= C.nx) return;
    double v;
    bool ok = inc64(C, M, z, y, x, v);
    if (!nan_excluded && !(M.flags & ~SPC_MASK_ARRAY) && v != v) {
        // (without a predicate a NaN sample is included when its mask byte says so: the mask, not the data, is reported)
        ok = (M.flags & SPC_MASK_ARRAY) ? M.arr[z * M.plane_stride + y * M.row_stride + x] != 0 : true;
    }
    out[(z * C.ny + y) * C.nx + x] = ok ? 1 : 0;
}

}  // namespace

extern "C" {

int spc_scale_f64(int device, void* stream, double* d_data, int64_t n, double factor) {
    SPC_REQUIRE(d_data != nullptr && n >= 0, "NULL pointer / negative count");
    SPC_DEVICE(device);
    const int64_t nb = (n + 255) / 256;
    SPC_REQUIRE(nb < (1LL << 31), "array too large for one launch");
    if (nb) hipLaunchKernelGGL(scale64_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, d_data, n, factor);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

int spc_narrow_f64_to_f32(int device, void* stream, const spc_cube_f64* cube, float* d_out, int64_t out_row_stride,
                          int64_t out_plane_stride) {
    Cube64 C; MaskDev64 M;
    int rc = cube64_args(cube, nullptr, &C, &M);
    if (rc) return rc;
    SPC_REQUIRE(d_out != nullptr, "d_out is NULL");
    SPC_DEVICE(device);
    const int64_t rs = out_row_stride ? out_row_stride : cube->nx, ps = out_plane_stride ? out_plane_stride : cube->ny * rs;
    for (int64_t z0 = 0; z0 < cube->nz; z0 += 65535) {         // blocks of at most 65535 planes x 65535 rows (gridDim.z / .y)
        for (int64_t y0 = 0; y0 < cube->ny; y0 += 65535) {
            Cube64 S = C;
            S.p = C.p + z0 * C.plane_stride + y0 * C.row_stride;
            const dim3 grid((unsigned)((cube->nx + 255) / 256), (unsigned)std::min<int64_t>(65535, cube->ny - y0),
                            (unsigned)std::min<int64_t>(65535, cube->nz - z0));
            hipLaunchKernelGGL(narrow64_kernel, grid, dim3(256), 0, (hipStream_t)stream, S, d_out + z0 * ps + y0 * rs, rs, ps);
            SPC_LAUNCH_CHECK();
        }
    }
    return SPC_OK;
}

int spc_mask_include_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded,
                         uint8_t* d_out) {
    Cube64 C; MaskDev64 M;
    int rc = cube64_args(cube, mask, &C, &M);
    if (rc) return rc;
    SPC_REQUIRE(d_out != nullptr, "d_out is NULL");
    SPC_DEVICE(device);
    const bool arr = (M.flags & SPC_MASK_ARRAY) != 0;
    for (int64_t z0 = 0; z0 < cube->nz; z0 += 65535) {         // blocks of at most 65535 planes x 65535 rows (gridDim.z / .y)
        for (int64_t y0 = 0; y0 < cube->ny; y0 += 65535) {
            Cube64 S = C;                                      // (S.ny stays the row count of an output plane)
            S.p = C.p + z0 * C.plane_stride + y0 * C.row_stride;
            MaskDev64 SM = M;
            if (arr) SM.arr = M.arr + z0 * M.plane_stride + y0 * M.row_stride;
            const dim3 grid((unsigned)((cube->nx + 255) / 256), (unsigned)std::min<int64_t>(65535, cube->ny - y0),
                            (unsigned)std::min<int64_t>(65535, cube->nz - z0));
            hipLaunchKernelGGL(include64_kernel, grid, dim3(256), 0, (hipStream_t)stream, S, SM, nan_excluded,
                               d_out + (z0 * cube->ny + y0) * cube->nx);
            SPC_LAUNCH_CHECK();
        }
    }
    return SPC_OK;
}

}  // extern "C"
