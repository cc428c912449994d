// spc_wide.h - what the float64 translation units share (spc_*_f64.hip): the cube as a kernel argument, the sample fetch
// with its mask, the stencils' quotient, and the host checks every float64 entry point starts with.
//
// The reference keeps a float64 source in float64 through every operator (np.result_type(dtype, 0.0),
// spectral_cube/masks.py:225; the Dask class keeps the chunk dtype, dask_spectral_cube.py:829).  The float64 kernels read and
// write the samples as they are: 8 bytes per voxel, thresholds compared in float64, sums in float64.
//
// Internal linkage throughout: every unit that includes this has its own copy, and a kernel's argument types stay unit-local.
#pragma once
#include "spc_common.h"

namespace {

// The quotient of a stencil window.  With non-negative taps it is a weighted mean of the valid samples and cannot exceed the
// largest of them: a window that holds DBL_MAX alone gives DBL_MAX, but k * max / k can round one step above it, which the
// type writes as inf.  A finite numerator never gives an infinite quotient here (a window with an infinite valid sample has
// an infinite numerator and stays infinite; 0 / 0 stays NaN).  Signed taps whose true quotient lies beyond DBL_MAX come out
// as DBL_MAX too.
__device__ __forceinline__ double quot_top(double num, double den) {
    double q = num / den;
    if (fabs(q) > 1.7976931348623157e308 && fabs(num) <= 1.7976931348623157e308) q = copysign(1.7976931348623157e308, q);
    return q;
}

struct Cube64 {
    const double* p;
    int64_t nz, ny, nx, row_stride, plane_stride;
};

__device__ __forceinline__ bool inc64(const Cube64& c, const MaskDev64& m, int64_t z, int64_t y, int64_t x, double& v) {
    v = c.p[z * c.plane_stride + y * c.row_stride + x];
    bool ok = spc_pred_valid(m, v);
    if (m.flags & SPC_MASK_ARRAY) ok = ok && m.arr[z * m.plane_stride + y * m.row_stride + x] != 0;
    return ok;
}

// Two float64 samples per lane (16-byte loads of the data, 2-byte loads of the mask array): rows of an even length on 16-byte
// boundaries, in the cube and - where the mask has an array term - in the mask
static bool spc_pairs_ok_f64(const spc_cube_f64* c, const MaskDev64& m) {
    const bool arr = (m.flags & SPC_MASK_ARRAY) != 0;
    return (c->nx % 2 == 0) && (c->row_stride % 2 == 0) && (c->plane_stride % 2 == 0) && ((((uintptr_t)c->d_data) & 15) == 0) &&
           (!arr || ((m.row_stride % 2 == 0) && (m.plane_stride % 2 == 0) && ((((uintptr_t)m.arr) & 1) == 0)));
}

// astropy: "The kernel can't be normalized, because its sum is close to zero" (convolve.py; the float32 entry points' check_kernel)
static int check_kernel_sum(const double* k, size_t n) {
    double sum = 0.0;
    for (size_t i = 0; i < n; ++i) sum += k[i];
    SPC_REQUIRE(!(sum < 1e-8 && sum > -1e-8) && sum >= 1.0 / 1e8, "The kernel can't be normalized, because its sum is close to zero");
    return SPC_OK;
}

// The cube and mask checks of a float64 entry point, and the kernels' view of both.  spc_check_nz_f64 is the moment kernel's
// bound (its count and z indices are packed into 21 bits each), not one of these kernels': the entry points that take a
// cube in spectral order have always carried it and keep it - no message moves; any_order (rays along y) never had it.
static int cube64_args(const spc_cube_f64* cube, const spc_mask_f64* mask, Cube64* C, MaskDev64* M, bool any_order = false) {
    int rc = any_order ? spc_check_cube_any_order(cube) : spc_check_cube(cube);
    if (!rc && !any_order) rc = spc_check_nz_f64(cube);
    if (rc) return rc;
    rc = spc_mask_to_dev(mask, cube, M);
    if (rc) return rc;
    C->p = cube->d_data; C->nz = cube->nz; C->ny = cube->ny; C->nx = cube->nx;
    C->row_stride = cube->row_stride; C->plane_stride = cube->plane_stride;
    return SPC_OK;
}

}  // namespace
