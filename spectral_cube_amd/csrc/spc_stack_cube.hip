// spc_stack_cube.hip - stack_cube of spectral_cube.analysis_utilities (analysis_utilities.py:321-432) in one pass: the
// spectral slabs of S lines of one cube, each linearly interpolated onto the velocity grid of the first
// (DaskSpectralCubeMixin.spectral_interpolate, dask_spectral_cube.py:1291-1373) and averaged over the lines.  No cutout is
// ever written: the slabs are read once and the (n0, ny, nx) stack is written once.
//
// The host hands over, per source s and output channel j, the plan of ops.lerp_plan in absolute channels of the cube:
// lo[s][j] (-1 = outside the slab), t[s][j] and inv_dx[s][j]; output sample = a + (b - a) * (inv_dx * t) with a, b the
// samples lo and lo + 1 (excluded ones NaN), a NaN result replaced by the fill value - the filled data of the
// interpolated slab, whose mask is ~isnan.  A source flagged exact (the reference slab) contributes its filled sample lo
// as it is.  Everything is float64 in source order, rounded once at the store; every output voxel is owned by one lane.
//
// Lanes run along x (16-byte loads and stores when the rows allow it).  A lane owns SKC_JC consecutive output channels of
// its spaxels and keeps their sums and counts in registers; it takes the sources one after the other and marches along j
// with the two bracketing samples in registers (lo[] only ever steps forward along j), so a cube sample is fetched once
// per source and chunk.  The tables are indexed by block and loop counters alone: scalar loads, uniform across a wave.
#include "spc_common.h"

namespace {

constexpr int SKC_BLOCK = 256;
constexpr int SKC_JC = 4;
constexpr int64_t SKC_GRID_LIMIT = 65535;

template <typename T>
struct SkcArgs {
    const T* in;
    int64_t ny, nx, rs, ps;
    SpcInclude<T> m;
    T fill;
    int nsrc, mode;
    int64_t n0;
    const int32_t* lo;                    // [nsrc][n0]
    const double* t;
    const double* inv_dx;
    const int32_t* exact;                 // [nsrc]
    T* out;                               // (n0, ny, nx), C-contiguous
};

template <typename T, int VEC> struct SkcVec;
template <> struct SkcVec<float, 4> { typedef float4 type; };
template <> struct SkcVec<double, 2> { typedef double2 type; };

template <typename T, int VEC>
__device__ __forceinline__ void skc_load(const T* p, T (&v)[VEC]) {
    if constexpr (VEC == 1) {
        v[0] = *p;
    } else {
        const typename SkcVec<T, VEC>::type q = *reinterpret_cast<const typename SkcVec<T, VEC>::type*>(p);
        const T* e = reinterpret_cast<const T*>(&q);
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = e[i];
    }
}

template <typename T, int VEC>
__device__ __forceinline__ void skc_store(T* p, const T (&v)[VEC]) {
    if constexpr (VEC == 1) {
        *p = v[0];
    } else {
        typename SkcVec<T, VEC>::type q;
        T* e = reinterpret_cast<T*>(&q);
#pragma unroll
        for (int i = 0; i < VEC; ++i) e[i] = v[i];
        *reinterpret_cast<typename SkcVec<T, VEC>::type*>(p) = q;
    }
}

template <int VEC>
__device__ __forceinline__ void skc_load_mask(const uint8_t* p, uint8_t (&mb)[VEC]) {
    if constexpr (VEC == 4) {
        const uint32_t q = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) mb[i] = (uint8_t)(q >> (8 * i));
    } else if constexpr (VEC == 2) {
        const uint16_t q = *reinterpret_cast<const uint16_t*>(p);
        mb[0] = (uint8_t)q; mb[1] = (uint8_t)(q >> 8);
    } else {
        mb[0] = *p;
    }
}

// the samples of plane z at this lane's spaxels, as float64: excluded ones NaN, or (filled) the fill value
template <typename T, int VEC>
__device__ __forceinline__ void skc_plane(const SkcArgs<T>& A, const T* p, const uint8_t* pm, int64_t z, bool filled, double (&r)[VEC]) {
    T v[VEC];
    uint8_t mb[VEC];
    skc_load<T, VEC>(p + z * A.ps, v);
    if (pm) {
        skc_load_mask<VEC>(pm + z * A.m.mps, mb);
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) mb[i] = 1;
    }
    const double out = filled ? (double)A.fill : (double)NAN;
#pragma unroll
    for (int i = 0; i < VEC; ++i) r[i] = spc_include(A.m, v[i], mb[i]) ? (double)v[i] : out;
}

// grid: x = tiles of SKC_BLOCK * VEC samples of a row, y = rows (of this launch's slab of rows), z = chunks of SKC_JC channels
template <typename T, int VEC>
__global__ __launch_bounds__(SKC_BLOCK) void stack_cube_kernel(const SkcArgs<T> A) {
    const int64_t x = ((int64_t)blockIdx.x * SKC_BLOCK + threadIdx.x) * VEC;
    if (x >= A.nx) return;                                   // (the vector form is launched only when VEC divides nx)
    const int64_t y = blockIdx.y;
    const T* p = A.in + y * A.rs + x;
    const uint8_t* pm = A.m.marr ? A.m.marr + y * A.m.mrs + x : nullptr;
    const int64_t nchunks = (A.n0 + SKC_JC - 1) / SKC_JC;
    for (int64_t chunk = blockIdx.z; chunk < nchunks; chunk += gridDim.z) {
        const int64_t j0 = chunk * SKC_JC;
        double acc[SKC_JC][VEC];
        int nfin[SKC_JC][VEC];                           // (the sources that are NaN there: nsrc - nfin)
#pragma unroll
        for (int u = 0; u < SKC_JC; ++u) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) { acc[u][i] = 0.0; nfin[u][i] = 0; }
        }
        for (int s = 0; s < A.nsrc; ++s) {
            const int64_t row = (int64_t)s * A.n0;
            const bool exact = A.exact[s] != 0;              // (wave-uniform, like every table entry below)
            int cur = -2;
            double ylo[VEC], yhi[VEC];
#pragma unroll
            for (int u = 0; u < SKC_JC; ++u) {
                const int64_t j = j0 + u;
                if (j < A.n0) {
                    const int lo = A.lo[row + j];
                    double r[VEC];
                    if (lo < 0) {
#pragma unroll
                        for (int i = 0; i < VEC; ++i) r[i] = (double)A.fill;
                    } else if (exact) {
                        skc_plane<T, VEC>(A, p, pm, lo, true, r);
                    } else {
                        if (lo != cur) {
                            if (lo == cur + 1) {
#pragma unroll
                                for (int i = 0; i < VEC; ++i) ylo[i] = yhi[i];
                            } else {
                                skc_plane<T, VEC>(A, p, pm, lo, false, ylo);
                            }
                            skc_plane<T, VEC>(A, p, pm, (int64_t)lo + 1, false, yhi);
                            cur = lo;
                        }
                        // scipy: slope = (y_hi - y_lo) / (x_hi - x_lo); y = slope * (x_new - x_lo) + y_lo
                        const double w = A.inv_dx[row + j] * A.t[row + j];
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            const double v = (yhi[i] - ylo[i]) * w + ylo[i];
                            r[i] = (v == v) ? v : (double)A.fill;     // the interpolated slab's mask is ~isnan: filled
                        }
                    }
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        const bool fin = r[i] == r[i];
                        acc[u][i] += fin ? r[i] : 0.0;
                        nfin[u][i] += fin ? 1 : 0;
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < SKC_JC; ++u) {
            const int64_t j = j0 + u;
            if (j < A.n0) {
                T o[VEC];
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    double v = acc[u][i];
                    if (A.mode == SPC_STACK_CUBE_NANMEAN) v = nfin[u][i] > 0 ? v / (double)nfin[u][i] : (double)NAN;
                    else if (A.mode == SPC_STACK_CUBE_MEAN) v = nfin[u][i] < A.nsrc ? (double)NAN : v / (double)A.nsrc;
                    else if (A.mode == SPC_STACK_CUBE_SUM) v = nfin[u][i] < A.nsrc ? (double)NAN : v;
                    o[i] = (T)v;
                }
                skc_store<T, VEC>(A.out + (j * A.ny + y) * A.nx + x, o);
            }
        }
    }
}

template <typename T>
int skc_entry(int device, void* stream, const typename SpcAbi<T>::cube* cube, const typename SpcAbi<T>::mask* mask, int nan_excluded,
              T fill, int nsrc, const int32_t* h_lo, const double* h_t, const double* h_inv_dx, const int32_t* h_exact, int mode,
              int64_t n0, T* d_out, void* d_workspace, size_t workspace_bytes) {
    int rc = spc_check_cube(cube);
    if (rc) return rc;
    SpcInclude<T> M;
    rc = spc_include_from(mask, cube, nan_excluded, &M);
    if (rc) return rc;
    SPC_REQUIRE(nsrc >= 1, "stack_cube needs at least one source (got %d)", nsrc);
    SPC_REQUIRE(h_lo && h_t && h_inv_dx && h_exact, "NULL table pointer");
    SPC_REQUIRE(d_out != nullptr, "d_out is NULL");
    if (nsrc > SPC_STACK_CUBE_MAX_LINES) {
        spc_set_error("%d sources are above the built limit of %d (SPC_STACK_CUBE_MAX_LINES)", nsrc, SPC_STACK_CUBE_MAX_LINES);
        return SPC_ERR_UNSUPPORTED;
    }
    SPC_REQUIRE(n0 >= 2, "the output grid needs at least 2 channels (got %lld)", (long long)n0);
    SPC_REQUIRE(n0 <= cube->nz, "the output grid (%lld channels) is longer than the cube (%lld)", (long long)n0, (long long)cube->nz);
    SPC_REQUIRE(mode >= SPC_STACK_CUBE_NANMEAN && mode <= SPC_STACK_CUBE_SUM, "unknown mode %d", mode);
    for (int s = 0; s < nsrc; ++s) {
        const int64_t top = h_exact[s] ? cube->nz - 1 : cube->nz - 2;       // an interpolated entry also reads channel lo + 1
        for (int64_t j = 0; j < n0; ++j) {
            const int64_t lo = h_lo[(int64_t)s * n0 + j];
            SPC_REQUIRE(lo == -1 || (lo >= 0 && lo <= top), "source %d, channel %lld: lower index %lld outside 0 .. %lld (-1 = out of range)",
                        s, (long long)j, (long long)lo, (long long)top);
        }
    }
    const size_t cells = (size_t)nsrc * (size_t)n0;
    SpcWorkspace ws(d_workspace, workspace_bytes);
    SPC_WS_TAKE(d_lo, ws, int32_t, cells);
    SPC_WS_TAKE(d_t, ws, double, cells);
    SPC_WS_TAKE(d_inv, ws, double, cells);
    SPC_WS_TAKE(d_exact, ws, int32_t, nsrc);

    SkcArgs<T> A{};
    A.in = cube->d_data; A.ny = cube->ny; A.nx = cube->nx; A.rs = cube->row_stride; A.ps = cube->plane_stride;
    A.m = M; A.fill = fill; A.nsrc = nsrc; A.mode = mode; A.n0 = n0;
    A.lo = d_lo; A.t = d_t; A.inv_dx = d_inv; A.exact = d_exact; A.out = d_out;
    constexpr int V = (int)(16 / sizeof(T));
    const int64_t e = (int64_t)sizeof(T);
    bool vec = cube->nx % V == 0 && spc_aligned(A.in, 16) && (A.rs * e) % 16 == 0 && (A.ps * e) % 16 == 0 && spc_aligned(A.out, 16);
    if (M.marr) vec = vec && spc_aligned(M.marr, V) && M.mrs % V == 0 && M.mps % V == 0;

    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    SPC_HIP(spc_table_upload(d_lo, h_lo, cells * sizeof(int32_t), st));
    SPC_HIP(spc_table_upload(d_t, h_t, cells * sizeof(double), st));
    SPC_HIP(spc_table_upload(d_inv, h_inv_dx, cells * sizeof(double), st));
    SPC_HIP(spc_table_upload(d_exact, h_exact, (size_t)nsrc * sizeof(int32_t), st));
    const int64_t per_block = (int64_t)SKC_BLOCK * (vec ? V : 1);
    const unsigned gx = (unsigned)((cube->nx + per_block - 1) / per_block);
    const unsigned gz = (unsigned)spc_min64((n0 + SKC_JC - 1) / SKC_JC, SKC_GRID_LIMIT);
    for (int64_t y0 = 0; y0 < cube->ny; y0 += SKC_GRID_LIMIT) {       // slabs of at most 65535 rows (gridDim.y)
        SkcArgs<T> S = A;
        const int64_t rows = spc_min64(SKC_GRID_LIMIT, cube->ny - y0);
        S.in = A.in + y0 * A.rs;
        if (S.m.marr) S.m.marr = A.m.marr + y0 * A.m.mrs;
        S.out = A.out + y0 * A.nx;
        dim3 grid(gx, (unsigned)rows, gz);
        if (vec) hipLaunchKernelGGL((stack_cube_kernel<T, V>), grid, dim3(SKC_BLOCK), 0, st, S);
        else hipLaunchKernelGGL((stack_cube_kernel<T, 1>), grid, dim3(SKC_BLOCK), 0, st, S);
        SPC_LAUNCH_CHECK();
    }
    return SPC_OK;
}

}  // namespace

extern "C" {

size_t spc_stack_cube_workspace_bytes(int nsrc, int64_t n0) {
    if (nsrc < 1 || n0 < 1) return 256;
    const size_t cells = (size_t)nsrc * (size_t)n0;
    return spc_ws_round(cells * sizeof(int32_t)) + 2 * spc_ws_round(cells * sizeof(double)) + spc_ws_round((size_t)nsrc * sizeof(int32_t)) + 256;
}

int spc_stack_cube_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded, float fill,
                       int nsrc, const int32_t* h_lo, const double* h_t, const double* h_inv_dx, const int32_t* h_exact, int mode,
                       int64_t n0, float* d_out, void* d_workspace, size_t workspace_bytes) {
    return skc_entry<float>(device, stream, cube, mask, nan_excluded, fill, nsrc, h_lo, h_t, h_inv_dx, h_exact, mode, n0, d_out,
                            d_workspace, workspace_bytes);
}

int spc_stack_cube_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded, double fill,
                       int nsrc, const int32_t* h_lo, const double* h_t, const double* h_inv_dx, const int32_t* h_exact, int mode,
                       int64_t n0, double* d_out, void* d_workspace, size_t workspace_bytes) {
    return skc_entry<double>(device, stream, cube, mask, nan_excluded, fill, nsrc, h_lo, h_t, h_inv_dx, h_exact, mode, n0, d_out,
                             d_workspace, workspace_bytes);
}

}  // extern "C"
