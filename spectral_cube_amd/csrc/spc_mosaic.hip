// spc_mosaic.hip - mosaic_cubes of spectral_cube.cube_utils (cube_utils.py:810-856) in one pass: S cubes, each
// resampled onto one target sky grid (SpectralCube.reproject -> reproject_interp, order 0 | 1) and averaged where they
// overlap.  No reprojected cube is ever written: every source is read where the target reaches it and the mosaic is
// written once.
//
// The reference, per source in list order:  final += nan_to_num(filled data of the reprojected cube)  (float64; NaN -> 0,
// +-inf -> +-DBL_MAX; the reprojected cube keeps the source's fill value, so OUTSIDE its footprint it contributes that fill
// value),  weight += footprint (2-D);  then  final /= weight  (0 / 0 = NaN where no cube reaches).
//
// Gather form, the shape of bilinear_kernel: a lane owns one output pixel of a compact 16 x 4 tile per wave and a run of
// channels.  It reads its source position in every source's pixel map once and notes which sources reach it (the weight);
// then, per group of MOS<T>::ZC channels, it takes the sources in list order with the group's sums in float64 registers,
// divides by the weight and stores each output value once.  No atomics, no second pass: two runs agree bit for bit.
//
// The value one source gives at one output voxel is restated from the resampling kernels so that it has THEIR bits:
// bilinear_kernel (spc_resample.hip) for float32 - float weights, fmaf(w11, d, fmaf(w10, c, fmaf(w01, b, w00 * a))), the
// mask as spc_pred reads it - and bilinear64_kernel (spc_resample_f64.hip) for float64 - double weights, a * w00 + b * w01 +
// c * w10 + d * w11, the mask in the canonical form with the NaN rule of an array-only mask.  Both: scipy's
// map_coordinates on the image padded by one edge-replicated pixel, NaN outside [-0.5, n - 0.5], a NaN neighbour
// propagates even with weight 0; unprojectable map entries (-1e30, or anything not finite) are outside.
#include "spc_common.h"
#include <algorithm>
#include <vector>

namespace {

template <typename T> struct MOS;
template <> struct MOS<float> { static constexpr int ZC = 8; };
template <> struct MOS<double> { static constexpr int ZC = 4; };

template <typename T>
struct MosSrc {                           // one source, as the kernel reads it from the device table
    const T* p;
    int64_t ny, nx, rs, ps;
    SpcMaskDev<T> m;
    T fill;
    double fill_num;                      // nan_to_num((double)fill): what the source adds outside its footprint
    const double* xs;
    const double* ys;
};

template <typename T>
struct MosArgs {
    const MosSrc<T>* src;
    int nsrc, nearest;
    int64_t nz, ny_out, nx_out, tiles_x, ntiles, zchunk;
    T* out;
    int32_t* weight;
};

__device__ __forceinline__ double mos_nan_to_num(double v) {
    const double big = 1.7976931348623157e308;
    if (v != v) return 0.0;
    return v > big ? big : (v < -big ? -big : v);
}

__device__ __forceinline__ bool mos_inside(double xs, double ys, int64_t nx, int64_t ny) {
    return (xs >= -0.5) && (xs <= (double)nx - 0.5) && (ys >= -0.5) && (ys <= (double)ny - 0.5);     // false for NaN
}

// the four neighbours of one source position: offsets into the plane and into the mask plane
struct MosTaps { int64_t o00, o01, o10, o11, m00, m01, m10, m11; };

template <typename T>
__device__ __forceinline__ MosTaps mos_taps(const MosSrc<T>& S, double xs, double ys, bool nearest, double& xf, double& yf) {
    xf = nearest ? floor(xs + 0.5) : floor(xs);
    yf = nearest ? floor(ys + 0.5) : floor(ys);
    const int64_t x0 = min(max((int64_t)xf, (int64_t)0), S.nx - 1), y0 = min(max((int64_t)yf, (int64_t)0), S.ny - 1);
    const int64_t x1 = nearest ? x0 : min((int64_t)xf + 1, S.nx - 1), y1 = nearest ? y0 : min((int64_t)yf + 1, S.ny - 1);
    MosTaps t;
    t.o00 = y0 * S.rs + x0; t.o01 = y0 * S.rs + x1; t.o10 = y1 * S.rs + x0; t.o11 = y1 * S.rs + x1;
    t.m00 = y0 * S.m.row_stride + x0; t.m01 = y0 * S.m.row_stride + x1;
    t.m10 = y1 * S.m.row_stride + x0; t.m11 = y1 * S.m.row_stride + x1;
    return t;
}

// float32: bilinear_kernel's sample.  An excluded voxel is the fill value (spectral_cube.py:2709-2712)
__device__ __forceinline__ float mos_filled(const MosSrc<float>& S, float v, const uint8_t* pm, int64_t moff) {
    if (S.m.flags == 0) return v;
    bool inc = spc_pred(S.m.flags, S.m.thr_lo, S.m.thr_hi, v);
    if (pm) inc = inc && pm[moff];
    return inc ? v : S.fill;
}
// float64: bilinear64_kernel's sample.  A NaN sample that an array-only mask includes stays what it is
__device__ __forceinline__ double mos_filled(const MosSrc<double>& S, double v, const uint8_t* pm, int64_t moff) {
    if (S.m.flags == 0) return v;
    bool ok = spc_pred_valid(S.m, v);
    if (pm) ok = ok && pm[moff] != 0;
    if (!ok && v != v && !(S.m.flags & ~SPC_MASK_ARRAY)) ok = !pm || pm[moff] != 0;
    return ok ? v : S.fill;
}

struct MosW32 { float w00, w01, w10, w11; };
struct MosW64 { double w00, w01, w10, w11; };
__device__ __forceinline__ MosW32 mos_weights(float, double xs, double ys, double xf, double yf) {
    const float fx = (float)(xs - xf), fy = (float)(ys - yf);
    return MosW32{(1.f - fy) * (1.f - fx), (1.f - fy) * fx, fy * (1.f - fx), fy * fx};
}
__device__ __forceinline__ MosW64 mos_weights(double, double xs, double ys, double xf, double yf) {
    const double fx = xs - xf, fy = ys - yf;
    return MosW64{(1.0 - fy) * (1.0 - fx), (1.0 - fy) * fx, fy * (1.0 - fx), fy * fx};
}
// plain weighted sums like scipy: a NaN neighbour propagates even with weight 0
__device__ __forceinline__ float mos_blend(const MosW32& w, float a, float b, float c, float d) {
    return fmaf(w.w11, d, fmaf(w.w10, c, fmaf(w.w01, b, w.w00 * a)));
}
__device__ __forceinline__ double mos_blend(const MosW64& w, double a, double b, double c, double d) {
    return a * w.w00 + b * w.w01 + c * w.w10 + d * w.w11;
}

// grid: x = 64 x 4 pixel tiles (strided when there are more than the grid holds), y = runs of zchunk channels
template <typename T>
__global__ __launch_bounds__(256) void mosaic_kernel(const MosArgs<T> A) {
    constexpr int ZC = MOS<T>::ZC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool nearest = A.nearest != 0;
    const int64_t zb = (int64_t)blockIdx.y * A.zchunk, ze = min(A.nz, zb + A.zchunk);
    for (int64_t tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
        const int64_t bx = tile % A.tiles_x, by = tile / A.tiles_x;
        const int64_t xo = bx * 64 + (wave * 16) + (lane & 15), yo = by * 4 + (lane >> 4);
        if (xo >= A.nx_out || yo >= A.ny_out) continue;
        const int64_t pix = yo * A.nx_out + xo;
        // which sources reach this pixel: the weight, and (for the first 64) a bit each so that the channel groups
        // below do not read the maps of the others again
        int w = 0;
        unsigned long long reach = 0ull;
        bool any_fill = false;
        for (int s = 0; s < A.nsrc; ++s) {
            const MosSrc<T>& S = A.src[s];
            const bool in = mos_inside(S.xs[pix], S.ys[pix], S.nx, S.ny);
            w += in ? 1 : 0;
            if (in && s < 64) reach |= 1ull << s;
            any_fill = any_fill || (!in && S.fill_num != 0.0);
        }
        if (blockIdx.y == 0 && A.weight) A.weight[pix] = w;
        T* po = A.out + yo * A.nx_out + xo;
        const int64_t ops = A.ny_out * A.nx_out;
        if (w == 0 && !any_fill) {                                   // 0 / 0
            for (int64_t z = zb; z < ze; ++z) __builtin_nontemporal_store((T)NAN, po + z * ops);
            continue;
        }
        const double dw = (double)w;
        for (int64_t zq = zb; zq < ze; zq += ZC) {
            double acc[ZC];
#pragma unroll
            for (int u = 0; u < ZC; ++u) acc[u] = 0.0;
            for (int s = 0; s < A.nsrc; ++s) {
                const MosSrc<T>& S = A.src[s];
                bool in = (reach >> (s & 63)) & 1ull;
                double xs = 0.0, ys = 0.0;
                if (s >= 64 || in) {
                    xs = S.xs[pix]; ys = S.ys[pix];
                    in = mos_inside(xs, ys, S.nx, S.ny);
                }
                if (!in) {
                    // outside its footprint the reprojected cube is its fill value (filled_data), NaN -> 0
                    if (S.fill_num != 0.0) {
#pragma unroll
                        for (int u = 0; u < ZC; ++u) acc[u] += S.fill_num;
                    }
                    continue;
                }
                double xf, yf;
                const MosTaps t = mos_taps(S, xs, ys, nearest, xf, yf);
                const auto wt = mos_weights(T(0), xs, ys, xf, yf);
                const bool arr = (S.m.flags & SPC_MASK_ARRAY) != 0;
                T a[ZC], b[ZC], c[ZC], d[ZC];
#pragma unroll
                for (int u = 0; u < ZC; ++u) {                       // the group's samples requested together
                    const int64_t z = min(zq + u, ze - 1);
                    const T* p = S.p + z * S.ps;
                    a[u] = p[t.o00];
                    if (!nearest) { b[u] = p[t.o01]; c[u] = p[t.o10]; d[u] = p[t.o11]; }
                }
#pragma unroll
                for (int u = 0; u < ZC; ++u) {
                    const int64_t z = min(zq + u, ze - 1);
                    const uint8_t* pm = arr ? S.m.arr + z * S.m.plane_stride : nullptr;
                    T r;
                    if (nearest) {
                        r = mos_filled(S, a[u], pm, t.m00);
                    } else {
                        const T aa = mos_filled(S, a[u], pm, t.m00), bb = mos_filled(S, b[u], pm, t.m01);
                        const T cc = mos_filled(S, c[u], pm, t.m10), dd = mos_filled(S, d[u], pm, t.m11);
                        r = mos_blend(wt, aa, bb, cc, dd);
                    }
                    acc[u] += mos_nan_to_num((double)r);
                }
            }
#pragma unroll
            for (int u = 0; u < ZC; ++u) {
                const int64_t z = zq + u;
                if (z < ze) __builtin_nontemporal_store((T)(acc[u] / dw), po + z * ops);
            }
        }
    }
}

template <typename T> struct MosAbi;
template <> struct MosAbi<float> { typedef spc_mosaic_source_f32 source; };
template <> struct MosAbi<double> { typedef spc_mosaic_source_f64 source; };

static inline double mos_nan_to_num_host(double v) {
    const double big = std::numeric_limits<double>::max();
    if (v != v) return 0.0;
    return v > big ? big : (v < -big ? -big : v);
}

template <typename T>
int mos_entry(int device, void* stream, int nsrc, const typename MosAbi<T>::source* h_sources, int64_t nz, int64_t ny_out,
              int64_t nx_out, int order, T* d_out, int32_t* d_weight, void* d_workspace, size_t workspace_bytes) {
    SPC_REQUIRE(nsrc >= 1, "mosaic needs at least one source (got %d)", nsrc);
    SPC_REQUIRE(h_sources != nullptr, "h_sources is NULL");
    SPC_REQUIRE(nz > 0 && ny_out > 0 && nx_out > 0, "output shape must be positive");
    SPC_REQUIRE(d_out != nullptr, "d_out is NULL");
    SPC_REQUIRE(order == 0 || order == 1, "order must be 1 (bilinear) or 0 (nearest neighbour), got %d", order);
    SpcWorkspace ws(d_workspace, workspace_bytes);
    SPC_WS_TAKE(d_src, ws, MosSrc<T>, nsrc);
    std::vector<MosSrc<T>> tab((size_t)nsrc);
    for (int s = 0; s < nsrc; ++s) {
        const auto& H = h_sources[s];
        int rc = spc_check_cube(&H.cube);
        if (rc) return rc;
        SPC_REQUIRE(H.cube.nz == nz, "source %d has %lld channels, the mosaic %lld", s, (long long)H.cube.nz, (long long)nz);
        SPC_REQUIRE(H.d_xs && H.d_ys, "source %d: NULL pixel map", s);
        MosSrc<T>& D = tab[s];
        rc = spc_mask_to_dev<T>(&H.mask, &H.cube, &D.m);
        if (rc) return rc;
        D.p = H.cube.d_data; D.ny = H.cube.ny; D.nx = H.cube.nx; D.rs = H.cube.row_stride; D.ps = H.cube.plane_stride;
        D.fill = H.fill; D.fill_num = mos_nan_to_num_host((double)H.fill);
        D.xs = H.d_xs; D.ys = H.d_ys;
    }
    MosArgs<T> A{};
    A.src = d_src; A.nsrc = nsrc; A.nearest = order == 0;
    A.nz = nz; A.ny_out = ny_out; A.nx_out = nx_out; A.out = d_out; A.weight = d_weight;
    A.tiles_x = (nx_out + 63) / 64;
    A.ntiles = A.tiles_x * ((ny_out + 3) / 4);
    constexpr int ZC = MOS<T>::ZC;
    int64_t nsplit = 1;
    if (A.ntiles < 2048) nsplit = std::max<int64_t>(1, std::min<int64_t>((2048 + A.ntiles - 1) / A.ntiles, nz / ZC));
    // runs of at most 64 channels: more, shorter blocks even out the tail (a pixel that no source reaches costs nothing)
    A.zchunk = std::min<int64_t>((nz + nsplit - 1) / nsplit, 64);
    A.zchunk = ((A.zchunk + ZC - 1) / ZC) * ZC;
    nsplit = (nz + A.zchunk - 1) / A.zchunk;
    if (nsplit > 65535) {                                            // gridDim.y
        A.zchunk = (((nz + 65534) / 65535 + ZC - 1) / ZC) * ZC;
        nsplit = (nz + A.zchunk - 1) / A.zchunk;
    }
    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    SPC_HIP(spc_table_upload(d_src, tab.data(), sizeof(MosSrc<T>) * (size_t)nsrc, st));
    const unsigned gx = (unsigned)std::min<int64_t>(A.ntiles, 0x7fffffffLL);
    hipLaunchKernelGGL(mosaic_kernel<T>, dim3(gx, (unsigned)nsplit), dim3(256), 0, st, A);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

}  // namespace

extern "C" {

size_t spc_mosaic_workspace_bytes(int nsrc) {
    const size_t per = std::max(sizeof(MosSrc<float>), sizeof(MosSrc<double>));
    return spc_ws_round(per * (size_t)(nsrc < 1 ? 1 : nsrc)) + 256;
}

int spc_mosaic_f32(int device, void* stream, int nsrc, const spc_mosaic_source_f32* h_sources, int64_t nz, int64_t ny_out,
                   int64_t nx_out, int order, float* d_out, int32_t* d_weight, void* d_workspace, size_t workspace_bytes) {
    return mos_entry<float>(device, stream, nsrc, h_sources, nz, ny_out, nx_out, order, d_out, d_weight, d_workspace, workspace_bytes);
}

int spc_mosaic_f64(int device, void* stream, int nsrc, const spc_mosaic_source_f64* h_sources, int64_t nz, int64_t ny_out,
                   int64_t nx_out, int order, double* d_out, int32_t* d_weight, void* d_workspace, size_t workspace_bytes) {
    return mos_entry<double>(device, stream, nsrc, h_sources, nz, ny_out, nx_out, order, d_out, d_weight, d_workspace, workspace_bytes);
}

}  // extern "C"
