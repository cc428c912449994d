// spc_resample_f64.hip - resampling a float64 cube (gfx950): spc_spectral_lerp_f64, spc_resample_bilinear_f64.
//
// The reference's spectral_interpolate (dask_spectral_cube.py:1342-1353: scipy's interp1d, slope form) and the bilinear /
// nearest resampling under reproject (spectral_cube.py:2709-2712 fills the excluded voxels first) on the float64 samples
// as they are: float64 weights, float64 results (spc_resample.hip holds the float32 kernels).  Plain gathers, a lane per
// output spaxel or pixel marching the channels; not tuned like the float32 forms.
#include "spc_wide.h"

#include <algorithm>

namespace {

// ---- spectral_interpolate -------------------------------------------------------------------------------------
struct Lerp64Args {
    Cube64 c;
    MaskDev64 m;
    int64_t nz_out;
    const int32_t* lo; const double* t; const double* inv_dx;
    double fill;
    double* out;
    int64_t out_row_stride, out_plane_stride, jchunk;
};
__global__ __launch_bounds__(256) void spectral_lerp64_kernel(const Lerp64Args A) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= A.c.ny * A.c.nx) return;
    const int64_t y = g / A.c.nx, x = g - y * A.c.nx;
    const int64_t jb = (int64_t)blockIdx.y * A.jchunk, je = min(A.nz_out, jb + A.jchunk);
    int cur = -2;
    double ylo = NAN, yhi = NAN;
    for (int64_t j = jb; j < je; ++j) {
        const int lo = A.lo[j];
        double res = A.fill;
        if (lo >= 0) {
            if (lo != cur) {
                double v;
                if (lo == cur + 1) ylo = yhi; else ylo = inc64(A.c, A.m, lo, y, x, v) ? v : NAN;
                yhi = inc64(A.c, A.m, lo + 1, y, x, v) ? v : NAN;
                cur = lo;
            }
            // scipy: slope = (y_hi - y_lo) / (x_hi - x_lo); y = slope * (x_new - x_lo) + y_lo
            res = (yhi - ylo) * A.inv_dx[j] * A.t[j] + ylo;
        }
        A.out[j * A.out_plane_stride + y * A.out_row_stride + x] = res;
    }
}

// ---- reproject: bilinear / nearest resampling --------------------------------------------------------------------
// bilinear_kernel's semantics (scipy map_coordinates(order = 1 | 0) on the edge-replicated image, NaN outside [-0.5, n - 0.5],
// a NaN neighbour propagates even with weight 0) with float64 samples, float64 weights and a float64 result.  Gather form:
// a lane per output pixel of a compact 16 x 4 tile per wave, marching the channels.
struct Bil64Args {
    Cube64 c;
    MaskDev64 m;
    double fill;
    int64_t ny_out, nx_out;
    const double* xs; const double* ys;
    double* out;
    int64_t out_row_stride, out_plane_stride, zchunk;
    uint8_t* footprint;
    int nearest;
    unsigned int* any_valid;
};
__global__ __launch_bounds__(256) void bilinear64_kernel(const Bil64Args A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tiles_x = (A.nx_out + 63) / 64;
    const int64_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const int64_t xo = bx * 64 + (wave * 16) + (lane & 15), yo = by * 4 + (lane >> 4);
    if (xo >= A.nx_out || yo >= A.ny_out) return;
    const int64_t pix = yo * A.nx_out + xo;
    const double xs = A.xs[pix], ys = A.ys[pix];
    const bool inside = (xs >= -0.5) && (xs <= (double)A.c.nx - 0.5) && (ys >= -0.5) && (ys <= (double)A.c.ny - 0.5);
    if (blockIdx.y == 0 && A.footprint) A.footprint[pix] = inside ? 1 : 0;
    const int64_t zb = (int64_t)blockIdx.y * A.zchunk, ze = min(A.c.nz, zb + A.zchunk);
    double* po = A.out + yo * A.out_row_stride + xo;
    if (!inside) {
        for (int64_t z = zb; z < ze; ++z) po[z * A.out_plane_stride] = NAN;
        return;
    }
    const double xf = A.nearest ? floor(xs + 0.5) : floor(xs), yf = A.nearest ? floor(ys + 0.5) : floor(ys);
    const int64_t x0 = min(max((int64_t)xf, (int64_t)0), A.c.nx - 1), y0 = min(max((int64_t)yf, (int64_t)0), A.c.ny - 1);
    const int64_t x1 = A.nearest ? x0 : min((int64_t)xf + 1, A.c.nx - 1), y1 = A.nearest ? y0 : min((int64_t)yf + 1, A.c.ny - 1);
    const double fx = xs - xf, fy = ys - yf;
    const double w00 = (1.0 - fy) * (1.0 - fx), w01 = (1.0 - fy) * fx, w10 = fy * (1.0 - fx), w11 = fy * fx;
    bool anyv = false;
    for (int64_t z = zb; z < ze; ++z) {
        // excluded voxels are replaced by the cube's fill value (spectral_cube.py:2709-2712); a NaN sample that an array-only
        // mask includes stays what it is (np.where(include, data, fill))
        auto get = [&](int64_t yy, int64_t xx) {
            double v;
            bool ok = inc64(A.c, A.m, z, yy, xx, v);
            if (!ok && v != v && !(A.m.flags & ~SPC_MASK_ARRAY))
                ok = !(A.m.flags & SPC_MASK_ARRAY) || A.m.arr[z * A.m.plane_stride + yy * A.m.row_stride + xx] != 0;
            return (A.m.flags && !ok) ? A.fill : v;
        };
        const double a = get(y0, x0), b = get(y0, x1), c = get(y1, x0), d = get(y1, x1);
        const double r = A.nearest ? a : (a * w00 + b * w01 + c * w10 + d * w11);
        anyv = anyv || (r == r);
        po[z * A.out_plane_stride] = r;
    }
    // (the lanes outside the output or the source have returned: the first lane still here reports, lane 0 may be gone)
    if (A.any_valid && __any(anyv) && lane == __ffsll((long long)__ballot(1)) - 1) atomicOr(A.any_valid, 1u);
}

}  // namespace

extern "C" {

int spc_spectral_lerp_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int64_t nz_out,
                          const int32_t* d_lo, const double* d_t, const double* d_inv_dx, double fill, double* d_out,
                          int64_t out_row_stride, int64_t out_plane_stride) {
    Lerp64Args A{};
    int rc = cube64_args(cube, mask, &A.c, &A.m);
    if (rc) return rc;
    SPC_REQUIRE(nz_out > 0 && d_lo && d_t && d_inv_dx && d_out, "NULL pointer argument / nz_out must be positive");
    SPC_DEVICE(device);
    A.nz_out = nz_out; A.lo = d_lo; A.t = d_t; A.inv_dx = d_inv_dx; A.fill = fill; A.out = d_out;
    A.out_row_stride = out_row_stride ? out_row_stride : cube->nx;
    A.out_plane_stride = out_plane_stride ? out_plane_stride : cube->ny * A.out_row_stride;
    const int64_t nb = (cube->ny * cube->nx + 255) / 256;
    SPC_REQUIRE(nb < (1LL << 31), "map too large for one launch");
    int nsplit = 1;
    if (nb < 2048) nsplit = (int)std::max<int64_t>(1, std::min<int64_t>((2048 + nb - 1) / nb, nz_out / 8));
    A.jchunk = (nz_out + nsplit - 1) / nsplit;
    nsplit = (int)((nz_out + A.jchunk - 1) / A.jchunk);
    hipLaunchKernelGGL(spectral_lerp64_kernel, dim3((unsigned)nb, (unsigned)nsplit), dim3(256), 0, (hipStream_t)stream, A);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

int spc_resample_bilinear_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, double fill,
                              int64_t ny_out, int64_t nx_out, const double* d_xs, const double* d_ys, double* d_out,
                              int64_t out_row_stride, int64_t out_plane_stride, uint8_t* d_footprint, int order,
                              uint32_t* d_any_valid) {
    Bil64Args A{};
    int rc = cube64_args(cube, mask, &A.c, &A.m);
    if (rc) return rc;
    SPC_REQUIRE(ny_out > 0 && nx_out > 0, "output shape must be positive");
    SPC_REQUIRE(d_xs && d_ys && d_out, "NULL pointer argument");
    SPC_REQUIRE(order == 0 || order == 1, "order must be 1 (bilinear) or 0 (nearest neighbour), got %d", order);
    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    A.fill = fill; A.ny_out = ny_out; A.nx_out = nx_out; A.xs = d_xs; A.ys = d_ys; A.out = d_out;
    A.out_row_stride = out_row_stride ? out_row_stride : nx_out;
    A.out_plane_stride = out_plane_stride ? out_plane_stride : ny_out * A.out_row_stride;
    A.footprint = d_footprint; A.nearest = order == 0; A.any_valid = d_any_valid;
    if (d_any_valid) SPC_HIP(hipMemsetAsync(d_any_valid, 0, sizeof(uint32_t), st));
    const int64_t nblocks = ((nx_out + 63) / 64) * ((ny_out + 3) / 4);
    SPC_REQUIRE(nblocks < (1LL << 31), "output map too large for one launch");
    int nsplit = 1;
    if (nblocks < 2048) nsplit = (int)std::max<int64_t>(1, std::min<int64_t>((2048 + nblocks - 1) / nblocks, cube->nz / 8));
    A.zchunk = (cube->nz + nsplit - 1) / nsplit;
    nsplit = (int)((cube->nz + A.zchunk - 1) / A.zchunk);
    hipLaunchKernelGGL(bilinear64_kernel, dim3((unsigned)nblocks, (unsigned)nsplit), dim3(256), 0, st, A);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

}  // extern "C"
