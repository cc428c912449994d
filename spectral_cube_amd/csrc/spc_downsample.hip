// spc_downsample.hip - block downsampling of a cube along one axis (SpectralCube.downsample_axis,
// spectral_cube.py:3421-3557, the in-memory form): estimator over every run of `factor` filled samples, plus the
// any(include) mask of the run, in one pass that reads every input byte once.
//
// Axes 0 and 1: a lane owns 4 consecutive x (one 16-byte load per sample row, 4 bytes of mask) and walks the factor
// planes / rows of its run itself; no cross-lane work, the 4 outputs and 4 mask bytes go out as one store each.
// Axis 2: the runs lie along the contiguous axis.  A block stages a row tile (whole runs, 16-byte loads) in LDS, filled
// and with its include bytes, and a thread reduces one run from there; runs too long for a tile (factor > 512) get a
// block each, reduced across the block.
#include "spc_common.h"

namespace {

enum { K_SUM = 0, K_MAX = 1, K_MIN = 2 };
constexpr int DS_BLOCK = 256;
constexpr int DS_TILE = 2048;             // samples of a row tile in LDS (axis 2)
constexpr int DS_TILE_MAX_FACTOR = DS_TILE / 4;

template <typename T>
struct DsArgs {
    const T* in;
    int64_t nz, ny, nx, rs, ps;           // input view, strides in elements
    SpcInclude<T> m;                      // which samples count; the others enter as fill
    T fill;
    int64_t f, n_ax;                      // factor, input length along the axis
    int64_t nzo, nyo, nxo;                // output shape
    T* out;
    uint8_t* omask;                       // may be nullptr
    int64_t ors, ops;                     // output strides (elements), shared by out and omask
    int nan_skip, mean;                   // estimator: skip NaN samples (nan*), divide by the count (mean)
};

template <typename T, int KIND>
struct Acc {
    double s;
    T m;
    int n;
    bool nan, any;
    __device__ __forceinline__ void init() {
        s = 0.0;
        m = KIND == K_MAX ? (T)-INFINITY : (T)INFINITY;
        n = 0;
        nan = false;
        any = false;
    }
    __device__ __forceinline__ void add(T v) {
        if (v == v) {
            if (KIND == K_MAX) m = v > m ? v : m;
            else if (KIND == K_MIN) m = v < m ? v : m;
            else s += (double)v;
            ++n;
        } else {
            nan = true;
        }
    }
    __device__ __forceinline__ void merge(const Acc& o) {
        s += o.s;
        if (KIND == K_MAX) m = o.m > m ? o.m : m;
        if (KIND == K_MIN) m = o.m < m ? o.m : m;
        n += o.n;
        nan |= o.nan;
        any |= o.any;
    }
    __device__ __forceinline__ T result(int nan_skip, int mean) const {
        if (!nan_skip && nan) return (T)NAN;
        if (KIND != K_SUM) return n ? m : (T)NAN;
        if (mean) return n ? (T)(s / (double)n) : (T)NAN;
        return (T)s;
    }
};

// 4 consecutive samples (nv <= 4 of them real); one 16-byte load (two for float64) when VEC and all 4 are there
template <bool VEC>
__device__ __forceinline__ void load4(const float* p, int nv, float (&v)[4]) {
    if (VEC && nv == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < nv ? p[j] : 0.f;
    }
}

template <bool VEC>
__device__ __forceinline__ void load4(const double* p, int nv, double (&v)[4]) {
    if (VEC && nv == 4) {
        const double2 a = *reinterpret_cast<const double2*>(p);
        const double2 b = *reinterpret_cast<const double2*>(p + 2);
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < nv ? p[j] : 0.0;
    }
}

template <bool VEC>
__device__ __forceinline__ void loadm4(const uint8_t* p, int nv, uint8_t (&m)[4]) {
    if (!p) {
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = 1;
    } else if (VEC && nv == 4) {
        const uint32_t q = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = (uint8_t)(q >> (8 * j));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = j < nv ? p[j] : 0;
    }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* p, int nv, const float (&v)[4]) {
    if (VEC && nv == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < nv; ++j) p[j] = v[j];
    }
}

template <bool VEC>
__device__ __forceinline__ void store4(double* p, int nv, const double (&v)[4]) {
    if (VEC && nv == 4) {
        *reinterpret_cast<double2*>(p) = make_double2(v[0], v[1]);
        *reinterpret_cast<double2*>(p + 2) = make_double2(v[2], v[3]);
    } else {
        for (int j = 0; j < nv; ++j) p[j] = v[j];
    }
}

template <bool VEC>
__device__ __forceinline__ void storem4(uint8_t* p, int nv, const uint8_t (&m)[4]) {
    if (VEC && nv == 4) {
        *reinterpret_cast<uint32_t*>(p) = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24);
    } else {
        for (int j = 0; j < nv; ++j) p[j] = m[j];
    }
}

// axes 0 and 1.  blockIdx.y = a, the loop index b: axis 0 -> input row y = a, output plane b, run of planes b*f ...;
// axis 1 -> output row a, plane z = b, run of rows a*f ...  Either way the output sample is (plane b, row a).
template <typename T, int KIND, bool VEC>
__global__ __launch_bounds__(DS_BLOCK) void ds_axis01_kernel(const DsArgs<T> A, int axis) {
    const int64_t x0 = ((int64_t)blockIdx.x * DS_BLOCK + threadIdx.x) * 4;
    if (x0 >= A.nx) return;
    const int nv = (int)spc_min64(4, A.nx - x0);
    const int64_t a = blockIdx.y;
    const int64_t nb = axis == 0 ? A.nzo : A.nz;
    const int64_t step = axis == 0 ? A.ps : A.rs, mstep = axis == 0 ? A.m.mps : A.m.mrs;
    for (int64_t b = blockIdx.z; b < nb; b += gridDim.z) {
        const int64_t z0 = axis == 0 ? b * A.f : b, y0 = axis == 0 ? a : a * A.f;
        const int64_t cnt = spc_min64(A.f, A.n_ax - (axis == 0 ? z0 : y0));       // real samples of the run
        const T* p = A.in + z0 * A.ps + y0 * A.rs + x0;
        const uint8_t* mp = A.m.marr ? A.m.marr + z0 * A.m.mps + y0 * A.m.mrs + x0 : nullptr;
        Acc<T, KIND> acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j].init();
#pragma unroll 4
        for (int64_t k = 0; k < cnt; ++k) {
            T v[4];
            uint8_t mb[4];
            load4<VEC>(p + k * step, nv, v);
            loadm4<VEC>(mp ? mp + k * mstep : nullptr, nv, mb);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool inc = spc_include(A.m, v[j], mb[j]);
                acc[j].any |= inc;
                acc[j].add(inc ? v[j] : A.fill);
            }
        }
        T r[4];
        uint8_t rm[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (cnt < A.f) acc[j].nan = true;                  // the NaN padding of a short last run
            r[j] = acc[j].result(A.nan_skip, A.mean);
            rm[j] = acc[j].any ? 1 : 0;
        }
        const int64_t o = b * A.ops + a * A.ors + x0;
        store4<VEC>(A.out + o, nv, r);
        if (A.omask) storem4<VEC>(A.omask + o, nv, rm);
    }
}

// axis 2, factor <= DS_TILE_MAX_FACTOR: blockIdx.x = tile of `nout_tile` runs of row (blockIdx.z.., blockIdx.y)
template <typename T, int KIND, bool VEC>
__global__ __launch_bounds__(DS_BLOCK) void ds_axis2_tile_kernel(const DsArgs<T> A, int nout_tile) {
    __shared__ T sv[DS_TILE];
    __shared__ uint8_t sm[DS_TILE];
    const int f = (int)A.f;
    const int64_t y = blockIdx.y;
    const int64_t xo0 = (int64_t)blockIdx.x * nout_tile;
    const int nout = (int)spc_min64(nout_tile, A.nxo - xo0);
    const int64_t xs = xo0 * f;
    const int span = (int)(spc_min64(A.nx, (xo0 + nout) * f) - xs);           // real samples of the tile
    for (int64_t z = blockIdx.z; z < A.nz; z += gridDim.z) {
        const T* p = A.in + z * A.ps + y * A.rs + xs;
        const uint8_t* mp = A.m.marr ? A.m.marr + z * A.m.mps + y * A.m.mrs + xs : nullptr;
        for (int i = threadIdx.x * 4; i < span; i += DS_BLOCK * 4) {
            const int nv = span - i < 4 ? span - i : 4;
            T v[4];
            uint8_t mb[4];
            load4<VEC>(p + i, nv, v);
            loadm4<VEC>(mp ? mp + i : nullptr, nv, mb);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < nv) {
                    const bool inc = spc_include(A.m, v[j], mb[j]);
                    sv[i + j] = inc ? v[j] : A.fill;
                    sm[i + j] = inc ? 1 : 0;
                }
            }
        }
        __syncthreads();
        for (int j = threadIdx.x; j < nout; j += DS_BLOCK) {
            const int b0 = j * f;
            const int cnt = span - b0 < f ? span - b0 : f;
            Acc<T, KIND> acc;
            acc.init();
            // start each run at a different offset (j mod f): neighbouring lanes then hit different LDS banks for any f
            int k = cnt ? j % cnt : 0;
            for (int t = 0; t < cnt; ++t) {
                acc.add(sv[b0 + k]);
                acc.any |= sm[b0 + k] != 0;
                k = (k + 1 == cnt) ? 0 : k + 1;
            }
            if (cnt < f) acc.nan = true;
            const int64_t o = z * A.ops + y * A.ors + xo0 + j;
            A.out[o] = acc.result(A.nan_skip, A.mean);
            if (A.omask) A.omask[o] = acc.any ? 1 : 0;
        }
        __syncthreads();
    }
}

// axis 2, factor > DS_TILE_MAX_FACTOR: one block per run (blockIdx.x), reduced across the block through LDS
template <typename T, int KIND, bool VEC>
__global__ __launch_bounds__(DS_BLOCK) void ds_axis2_run_kernel(const DsArgs<T> A) {
    __shared__ double ss[DS_BLOCK];
    __shared__ T smv[DS_BLOCK];
    __shared__ int sn[DS_BLOCK];
    __shared__ uint8_t sfl[DS_BLOCK];
    const int64_t xo = blockIdx.x, y = blockIdx.y;
    const int64_t xs = xo * A.f;
    const int64_t span = spc_min64(A.nx, xs + A.f) - xs;
    const int tid = threadIdx.x;
    for (int64_t z = blockIdx.z; z < A.nz; z += gridDim.z) {
        const T* p = A.in + z * A.ps + y * A.rs + xs;
        const uint8_t* mp = A.m.marr ? A.m.marr + z * A.m.mps + y * A.m.mrs + xs : nullptr;
        Acc<T, KIND> acc;
        acc.init();
        for (int64_t i = (int64_t)tid * 4; i < span; i += DS_BLOCK * 4) {
            const int nv = (int)spc_min64(4, span - i);
            T v[4];
            uint8_t mb[4];
            load4<VEC>(p + i, nv, v);
            loadm4<VEC>(mp ? mp + i : nullptr, nv, mb);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < nv) {
                    const bool inc = spc_include(A.m, v[j], mb[j]);
                    acc.any |= inc;
                    acc.add(inc ? v[j] : A.fill);
                }
            }
        }
        ss[tid] = acc.s; smv[tid] = acc.m; sn[tid] = acc.n;
        sfl[tid] = (acc.nan ? 1 : 0) | (acc.any ? 2 : 0);
        __syncthreads();
        for (int w = DS_BLOCK / 2; w > 0; w >>= 1) {
            if (tid < w) {
                Acc<T, KIND> o;
                o.s = ss[tid + w]; o.m = smv[tid + w]; o.n = sn[tid + w];
                o.nan = sfl[tid + w] & 1; o.any = (sfl[tid + w] & 2) != 0;
                acc.merge(o);
                ss[tid] = acc.s; smv[tid] = acc.m; sn[tid] = acc.n;
                sfl[tid] = (acc.nan ? 1 : 0) | (acc.any ? 2 : 0);
            }
            __syncthreads();
        }
        if (tid == 0) {
            if (span < A.f) acc.nan = true;
            const int64_t o = z * A.ops + y * A.ors + xo;
            A.out[o] = acc.result(A.nan_skip, A.mean);
            if (A.omask) A.omask[o] = acc.any ? 1 : 0;
        }
        __syncthreads();
    }
}

template <typename T, int KIND, bool VEC>
void ds_launch_kind(const DsArgs<T>& A, int axis, hipStream_t st) {
    const unsigned gz = (unsigned)spc_min64(axis == 0 ? A.nzo : A.nz, 65535);
    if (axis < 2) {
        const int64_t lanes = (A.nx + 3) / 4;
        dim3 grid((unsigned)((lanes + DS_BLOCK - 1) / DS_BLOCK), (unsigned)(axis == 0 ? A.ny : A.nyo), gz);
        hipLaunchKernelGGL((ds_axis01_kernel<T, KIND, VEC>), grid, dim3(DS_BLOCK), 0, st, A, axis);
    } else if (A.f <= DS_TILE_MAX_FACTOR) {
        const int nout_tile = (DS_TILE / (int)A.f) & ~3;         // whole runs, a multiple of 4 runs: tiles start 16-byte aligned
        dim3 grid((unsigned)((A.nxo + nout_tile - 1) / nout_tile), (unsigned)A.ny, gz);
        hipLaunchKernelGGL((ds_axis2_tile_kernel<T, KIND, VEC>), grid, dim3(DS_BLOCK), 0, st, A, nout_tile);
    } else {
        dim3 grid((unsigned)A.nxo, (unsigned)A.ny, gz);
        hipLaunchKernelGGL((ds_axis2_run_kernel<T, KIND, VEC>), grid, dim3(DS_BLOCK), 0, st, A);
    }
}

template <typename T, bool VEC>
void ds_launch_vec(const DsArgs<T>& A, int axis, int kind, hipStream_t st) {
    if (kind == K_SUM) ds_launch_kind<T, K_SUM, VEC>(A, axis, st);
    else if (kind == K_MAX) ds_launch_kind<T, K_MAX, VEC>(A, axis, st);
    else ds_launch_kind<T, K_MIN, VEC>(A, axis, st);
}

// shape, strides and output checks shared by both sample types; fills the geometry of A
template <typename T>
int ds_setup(DsArgs<T>& A, int axis, int64_t factor, int truncate, int estimator, T* d_out, int64_t ors, int64_t ops,
             uint8_t* d_out_mask) {
    SPC_REQUIRE(axis >= 0 && axis <= 2, "axis must be 0, 1 or 2 (got %d)", axis);
    SPC_REQUIRE(factor >= 1 && factor <= 0x7fffffff, "factor must be an integer >= 1 (got %lld)", (long long)factor);
    SPC_REQUIRE(estimator >= SPC_DS_NANMEAN && estimator <= SPC_DS_MIN, "unknown estimator %d", estimator);
    SPC_REQUIRE(d_out != nullptr, "d_out is NULL");
    const int64_t n = axis == 0 ? A.nz : (axis == 1 ? A.ny : A.nx);
    const int64_t nout = truncate ? n / factor : (n + factor - 1) / factor;
    SPC_REQUIRE(nout >= 1, "truncating %lld samples by a factor of %lld leaves nothing", (long long)n, (long long)factor);
    A.f = factor;
    A.n_ax = n;
    A.nzo = axis == 0 ? nout : A.nz;
    A.nyo = axis == 1 ? nout : A.ny;
    A.nxo = axis == 2 ? nout : A.nx;
    A.ors = ors ? ors : A.nxo;
    A.ops = ops ? ops : A.nyo * A.ors;
    SPC_REQUIRE(A.ors >= A.nxo && A.ops >= A.ors * (A.nyo - 1) + A.nxo, "output strides too small for (%lld, %lld, %lld)",
                (long long)A.nzo, (long long)A.nyo, (long long)A.nxo);
    A.out = d_out;
    A.omask = d_out_mask;
    A.nan_skip = estimator < SPC_DS_MEAN;
    A.mean = (estimator & 3) == 0;
    return SPC_OK;
}

// 16-byte loads need every row and plane of the input to start 16-byte aligned (4-byte for the mask array); the runs of
// the axis-2 forms start on a multiple of 4 samples only when factor allows.  The stores of axes 0 / 1 are 16-byte (4-byte
// for the mask) as well, those of axis 2 one sample per lane: only axes 0 / 1 ask the same of the outputs
template <typename T>
bool ds_vec_ok(const DsArgs<T>& A, int axis) {
    const size_t e = sizeof(T);
    bool ok = spc_aligned(A.in, 16) && (A.rs * e) % 16 == 0 && (A.ps * e) % 16 == 0;
    if (A.m.marr) ok = ok && spc_aligned(A.m.marr, 4) && A.m.mrs % 4 == 0 && A.m.mps % 4 == 0;
    if (axis < 2) {
        ok = ok && spc_aligned(A.out, 16) && A.ors % 4 == 0 && A.ops % 4 == 0 && (A.ors * e) % 16 == 0 && (A.ops * e) % 16 == 0;
        if (A.omask) ok = ok && spc_aligned(A.omask, 4);
    }
    if (axis == 2 && A.f > DS_TILE_MAX_FACTOR) ok = ok && A.f % 4 == 0;
    return ok;
}

template <typename T>
int ds_run(int device, void* stream, const DsArgs<T>& A, int axis, int estimator) {
    SPC_DEVICE(device);
    const int kind = (estimator & 3) < 2 ? K_SUM : ((estimator & 3) == 2 ? K_MAX : K_MIN);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = ds_vec_ok(A, axis);             // (row offsets below keep every alignment it checks)
    const int64_t rows = axis == 1 ? A.nyo : A.ny;   // blockIdx.y: output rows along y, input rows otherwise
    for (int64_t r0 = 0; r0 < rows; r0 += 65535) {   // slabs of at most 65535 rows (gridDim.y)
        DsArgs<T> S = A;
        const int64_t n = spc_min64(65535, rows - r0), in_r0 = axis == 1 ? r0 * A.f : r0;
        S.in = A.in + in_r0 * A.rs;
        if (S.m.marr) S.m.marr = A.m.marr + in_r0 * A.m.mrs;
        S.out = A.out + r0 * A.ors;
        if (S.omask) S.omask = A.omask + r0 * A.ors;
        if (axis == 1) {
            S.n_ax = A.n_ax - in_r0;
            S.nyo = n;
            S.ny = spc_min64(S.n_ax, n * A.f);
        } else {
            S.ny = S.nyo = n;
        }
        if (vec) ds_launch_vec<T, true>(S, axis, kind, st);
        else ds_launch_vec<T, false>(S, axis, kind, st);
        SPC_LAUNCH_CHECK();
    }
    return SPC_OK;
}

template <typename T>
int ds_entry(int device, void* stream, const typename SpcAbi<T>::cube* cube, const typename SpcAbi<T>::mask* mask, int nan_excluded,
             T fill, int axis, int64_t factor, int truncate, int estimator, T* d_out, int64_t out_row_stride,
             int64_t out_plane_stride, uint8_t* d_out_mask) {
    int rc = spc_check_cube(cube);
    if (rc) return rc;
    if constexpr (sizeof(T) == 8) {                  // inherited from the float64 moment kernel's cube check; nothing here needs it
        rc = spc_check_nz_f64(cube);
        if (rc) return rc;
    }
    DsArgs<T> A{};
    rc = spc_include_from(mask, cube, nan_excluded, &A.m);
    if (rc) return rc;
    A.in = cube->d_data; A.nz = cube->nz; A.ny = cube->ny; A.nx = cube->nx;
    A.rs = cube->row_stride; A.ps = cube->plane_stride;
    A.fill = fill;
    rc = ds_setup(A, axis, factor, truncate, estimator, d_out, out_row_stride, out_plane_stride, d_out_mask);
    if (rc) return rc;
    return ds_run(device, stream, A, axis, estimator);
}

}  // namespace

extern "C" {

int spc_downsample_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded,
                       float fill, int axis, int64_t factor, int truncate, int estimator,
                       float* d_out, int64_t out_row_stride, int64_t out_plane_stride, uint8_t* d_out_mask) {
    return ds_entry<float>(device, stream, cube, mask, nan_excluded, fill, axis, factor, truncate, estimator, d_out, out_row_stride,
                           out_plane_stride, d_out_mask);
}

int spc_downsample_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded,
                       double fill, int axis, int64_t factor, int truncate, int estimator,
                       double* d_out, int64_t out_row_stride, int64_t out_plane_stride, uint8_t* d_out_mask) {
    return ds_entry<double>(device, stream, cube, mask, nan_excluded, fill, axis, factor, truncate, estimator, d_out, out_row_stride,
                            out_plane_stride, d_out_mask);
}

}  // extern "C"
