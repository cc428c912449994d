// spc_subcube.hip - cutting a cube on the device: the gather behind SpectralCube.__getitem__ / spectral_slab / subcube
// (spectral_cube.py:1308-1381, 1823-1879, 1947-2036) and the bounding box of a mask behind minimal_subcube /
// subcube_slices_from_mask (:1881-1945).
//
// Gather: output sample (k, j, i) is parent sample (z0 + k * sz, y0 + j * sy, x0 + i * sx); data and the include byte of the
// parent's lowered mask leave in one pass, and only the selected rows are ever addressed.  With sx == 1 and every selected
// source row, the output rows and the mask rows 16-byte (4-byte) aligned a lane owns 4 consecutive x (one 16-byte load, one
// 16-byte store); otherwise a lane owns one sample per row (consecutive lanes = consecutive samples, one load each).
// Bounding box: every lane keeps the extremes of the (z, y, x) of its included voxels, a wave folds them with
// cross-lane shuffles, the block's waves meet in LDS, and lane 0 issues one atomicMin / atomicMax per bound.
#include "spc_common.h"

namespace {

constexpr int SC_BLOCK = 256;
constexpr int SC_WAVES = SC_BLOCK / 64;
constexpr int64_t SC_GRID_LIMIT = 65535;

__host__ __device__ __forceinline__ int64_t sc_max(int64_t a, int64_t b) { return a > b ? a : b; }

template <typename T>
struct ScArgs {
    const T* in;                          // parent sample (z0, y0, x0): the start offsets are folded into the pointers
    int64_t sz, sy, sx;                   // element offset between selected planes / rows / samples (step * stride, signed)
    SpcInclude<T> m;                          // marr likewise at (z0, y0, x0); mrs / mps already multiplied by the steps
    int64_t msx;
    int64_t nzo, nyo, nxo;
    T* out;
    uint8_t* omask;                       // may be nullptr
    int64_t ors, ops;
    int filled;
    T fill;
};

__device__ __forceinline__ void sc_load4(const float* p, float (&v)[4]) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
__device__ __forceinline__ void sc_load4(const double* p, double (&v)[4]) {
    const double2 a = *reinterpret_cast<const double2*>(p);
    const double2 b = *reinterpret_cast<const double2*>(p + 2);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
}
__device__ __forceinline__ void sc_store4(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void sc_store4(double* p, const double (&v)[4]) {
    *reinterpret_cast<double2*>(p) = make_double2(v[0], v[1]);
    *reinterpret_cast<double2*>(p + 2) = make_double2(v[2], v[3]);
}

// sx == 1, everything aligned: blockIdx.y = output row, blockIdx.z.. = output planes, a lane owns 4 consecutive x
template <typename T>
__global__ __launch_bounds__(SC_BLOCK) void sc_gather_vec_kernel(const ScArgs<T> A) {
    const int64_t x = ((int64_t)blockIdx.x * SC_BLOCK + threadIdx.x) * 4;
    if (x >= A.nxo) return;
    const int nv = (int)spc_min64(4, A.nxo - x);
    const int64_t j = blockIdx.y;
    for (int64_t k = blockIdx.z; k < A.nzo; k += gridDim.z) {
        const T* p = A.in + k * A.sz + j * A.sy + x;
        const uint8_t* mp = A.m.marr ? A.m.marr + k * A.m.mps + j * A.m.mrs + x : nullptr;
        const int64_t o = k * A.ops + j * A.ors + x;
        T v[4];
        uint8_t mb[4] = {1, 1, 1, 1};
        if (nv == 4) {
            sc_load4(p, v);
            if (mp) {
                const uint32_t q = *reinterpret_cast<const uint32_t*>(mp);
#pragma unroll
                for (int t = 0; t < 4; ++t) mb[t] = (uint8_t)(q >> (8 * t));
            }
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                v[t] = t < nv ? p[t] : (T)0;
                if (mp) mb[t] = t < nv ? mp[t] : 0;
            }
        }
        uint32_t packed = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool inc = spc_include(A.m, v[t], mb[t]);
            packed |= (inc ? 1u : 0u) << (8 * t);
            if (A.filled) v[t] = inc ? v[t] : A.fill;
        }
        if (nv == 4) {
            sc_store4(A.out + o, v);
            if (A.omask) *reinterpret_cast<uint32_t*>(A.omask + o) = packed;
        } else {
            for (int t = 0; t < nv; ++t) {
                A.out[o + t] = v[t];
                if (A.omask) A.omask[o + t] = (uint8_t)(packed >> (8 * t));
            }
        }
    }
}

// any step, any alignment: a lane owns one output sample per row
template <typename T>
__global__ __launch_bounds__(SC_BLOCK) void sc_gather_kernel(const ScArgs<T> A) {
    const int64_t i = (int64_t)blockIdx.x * SC_BLOCK + threadIdx.x;
    if (i >= A.nxo) return;
    const int64_t j = blockIdx.y;
    for (int64_t k = blockIdx.z; k < A.nzo; k += gridDim.z) {
        T v = A.in[k * A.sz + j * A.sy + i * A.sx];
        const uint8_t mb = A.m.marr ? A.m.marr[k * A.m.mps + j * A.m.mrs + i * A.msx] : (uint8_t)1;
        const bool inc = spc_include(A.m, v, mb);
        if (A.filled) v = inc ? v : A.fill;
        const int64_t o = k * A.ops + j * A.ors + i;
        A.out[o] = v;
        if (A.omask) A.omask[o] = inc ? 1 : 0;
    }
}

// ---- bounding box -------------------------------------------------------------------------------------------------
template <typename T>
struct BbArgs {
    const T* in;
    int64_t nz, ny, nx, rs, ps;
    SpcInclude<T> m;
    long long* box;                       // {zmin, zmax, ymin, ymax, xmin, xmax}
};

__global__ void bb_init_kernel(long long* box) {
    const int t = threadIdx.x;
    if (t < 6) box[t] = (t & 1) ? -1LL : 0x7fffffffffffffffLL;
}

__device__ __forceinline__ int64_t bb_wave_min(int64_t v) {
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) v = spc_min64(v, (int64_t)__shfl_xor((long long)v, w));
    return v;
}
__device__ __forceinline__ int64_t bb_wave_max(int64_t v) {
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) v = sc_max(v, (int64_t)__shfl_xor((long long)v, w));
    return v;
}

// blockIdx.x = tile of 4 * SC_BLOCK samples of a row (VEC) or SC_BLOCK samples; rows and planes are strided over
// gridDim.y / gridDim.z.  DATA: a term needs the samples (predicate or nan_excluded); otherwise only mask bytes are read.
template <typename T, bool VEC, bool DATA>
__global__ __launch_bounds__(SC_BLOCK) void bb_kernel(const BbArgs<T> A) {
    constexpr int W = VEC ? 4 : 1;
    __shared__ int64_t sred[6][SC_WAVES];
    const int64_t x = ((int64_t)blockIdx.x * SC_BLOCK + threadIdx.x) * W;
    const int64_t big = 0x7fffffffffffffffLL;
    int64_t zmin = big, zmax = -1, ymin = big, ymax = -1;
    uint32_t hits = 0;                                        // bit t: sample x + t included somewhere
    if (x < A.nx) {
        const int nv = (int)spc_min64(W, A.nx - x);
        for (int64_t z = blockIdx.z; z < A.nz; z += gridDim.z) {
            uint32_t hz = 0;
#pragma unroll 4
            for (int64_t y = blockIdx.y; y < A.ny; y += gridDim.y) {
                T v[4] = {(T)0, (T)0, (T)0, (T)0};
                uint8_t mb[4] = {1, 1, 1, 1};
                if (VEC && nv == 4) {
                    if (DATA) sc_load4(A.in + z * A.ps + y * A.rs + x, v);
                    if (A.m.marr) {
                        const uint32_t q = *reinterpret_cast<const uint32_t*>(A.m.marr + z * A.m.mps + y * A.m.mrs + x);
#pragma unroll
                        for (int t = 0; t < 4; ++t) mb[t] = (uint8_t)(q >> (8 * t));
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < W; ++t) {
                        if (t < nv) {
                            if (DATA) v[t] = A.in[z * A.ps + y * A.rs + x + t];
                            if (A.m.marr) mb[t] = A.m.marr[z * A.m.mps + y * A.m.mrs + x + t];
                        } else {
                            mb[t] = 0;
                        }
                    }
                }
                uint32_t h = 0;
#pragma unroll
                for (int t = 0; t < W; ++t) {
                    const bool inc = DATA ? spc_include(A.m, v[t], mb[t]) : (mb[t] != 0);
                    h |= (inc ? 1u : 0u) << t;
                }
                if (h) {
                    ymin = spc_min64(ymin, y);
                    ymax = sc_max(ymax, y);
                }
                hz |= h;
            }
            if (hz) {
                zmin = spc_min64(zmin, z);
                zmax = sc_max(zmax, z);
            }
            hits |= hz;
        }
    }
    int64_t xmin = big, xmax = -1;
    if (hits) {
        xmin = x + (__ffs((int)hits) - 1);
        xmax = x + (31 - __clz((int)hits));
    }
    // wave, then block, then one atomic per bound and block (none when the block saw nothing)
    int64_t r[6] = {bb_wave_min(zmin), bb_wave_max(zmax), bb_wave_min(ymin), bb_wave_max(ymax), bb_wave_min(xmin), bb_wave_max(xmax)};
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 6; ++q) sred[q][wave] = r[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            int64_t a = sred[q][0];
            for (int w = 1; w < SC_WAVES; ++w) a = (q & 1) ? sc_max(a, sred[q][w]) : spc_min64(a, sred[q][w]);
            r[q] = a;
        }
        if (r[1] >= 0) {
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                if (q & 1) atomicMax(A.box + q, (long long)r[q]);
                else atomicMin(A.box + q, (long long)r[q]);
            }
        }
    }
}

template <typename T>
int sc_run(int device, void* stream, const T* in, int64_t nz, int64_t ny, int64_t nx, int64_t rs, int64_t ps, SpcInclude<T> M,
           const int64_t* start, const int64_t* step, int64_t nzo, int64_t nyo, int64_t nxo, T* d_out, int64_t ors, int64_t ops,
           uint8_t* d_out_mask, int filled, T fill) {
    SPC_REQUIRE(start != nullptr && step != nullptr, "start / step is NULL");
    SPC_REQUIRE(d_out != nullptr, "d_out is NULL");
    const int64_t n_in[3] = {nz, ny, nx}, n_out[3] = {nzo, nyo, nxo};
    for (int a = 0; a < 3; ++a) {
        SPC_REQUIRE(step[a] != 0, "step of axis %d is 0", a);
        SPC_REQUIRE(n_out[a] >= 1, "empty selection along axis %d (output length %lld)", a, (long long)n_out[a]);
        SPC_REQUIRE(n_out[a] <= n_in[a], "output longer than the parent along axis %d", a);
        const int64_t last = start[a] + (n_out[a] - 1) * step[a];
        SPC_REQUIRE(start[a] >= 0 && start[a] < n_in[a] && last >= 0 && last < n_in[a],
                    "axis %d: samples %lld .. %lld (step %lld) leave the parent's 0 .. %lld", a, (long long)start[a], (long long)last,
                    (long long)step[a], (long long)n_in[a] - 1);
    }
    ScArgs<T> A{};
    A.nzo = nzo; A.nyo = nyo; A.nxo = nxo;
    A.ors = ors ? ors : nxo;
    A.ops = ops ? ops : nyo * A.ors;
    SPC_REQUIRE(A.ors >= nxo && A.ops >= A.ors * (nyo - 1) + nxo, "output strides too small for (%lld, %lld, %lld)",
                (long long)nzo, (long long)nyo, (long long)nxo);
    A.in = in + start[0] * ps + start[1] * rs + start[2];
    A.sz = step[0] * ps; A.sy = step[1] * rs; A.sx = step[2];
    A.m = M;
    if (M.marr) {
        A.m.marr = M.marr + start[0] * M.mps + start[1] * M.mrs + start[2];
        A.m.mps = step[0] * M.mps; A.m.mrs = step[1] * M.mrs;
    }
    A.msx = step[2];
    A.out = d_out; A.omask = d_out_mask;
    A.filled = filled != 0; A.fill = fill;
    const size_t e = sizeof(T);
    bool vec = step[2] == 1 && spc_aligned(A.in, 16) && (A.sz * (int64_t)e) % 16 == 0 && (A.sy * (int64_t)e) % 16 == 0 &&
               spc_aligned(A.out, 16) && (A.ors * e) % 16 == 0 && (A.ops * e) % 16 == 0;
    if (A.m.marr) vec = vec && spc_aligned(A.m.marr, 4) && A.m.mrs % 4 == 0 && A.m.mps % 4 == 0;
    if (A.omask) vec = vec && spc_aligned(A.omask, 4) && A.ors % 4 == 0 && A.ops % 4 == 0;
    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const unsigned gz = (unsigned)spc_min64(nzo, SC_GRID_LIMIT);
    const int64_t per_block = vec ? 4 * SC_BLOCK : SC_BLOCK;
    const unsigned gx = (unsigned)((nxo + per_block - 1) / per_block);
    for (int64_t j0 = 0; j0 < nyo; j0 += SC_GRID_LIMIT) {      // slabs of at most 65535 output rows (gridDim.y)
        ScArgs<T> S = A;
        S.nyo = spc_min64(SC_GRID_LIMIT, nyo - j0);
        S.in = A.in + j0 * A.sy;
        if (S.m.marr) S.m.marr = A.m.marr + j0 * A.m.mrs;
        S.out = A.out + j0 * A.ors;
        if (S.omask) S.omask = A.omask + j0 * A.ors;
        dim3 grid(gx, (unsigned)S.nyo, gz);
        if (vec) hipLaunchKernelGGL((sc_gather_vec_kernel<T>), grid, dim3(SC_BLOCK), 0, st, S);
        else hipLaunchKernelGGL((sc_gather_kernel<T>), grid, dim3(SC_BLOCK), 0, st, S);
        SPC_LAUNCH_CHECK();
    }
    return SPC_OK;
}

template <typename T>
int bb_run(int device, void* stream, const T* in, int64_t nz, int64_t ny, int64_t nx, int64_t rs, int64_t ps, SpcInclude<T> M,
           int64_t* d_box) {
    SPC_REQUIRE(d_box != nullptr, "d_box is NULL");
    SPC_REQUIRE(spc_aligned(d_box, 8), "d_box must be 8-byte aligned");
    BbArgs<T> A{};
    A.in = in; A.nz = nz; A.ny = ny; A.nx = nx; A.rs = rs; A.ps = ps;
    A.m = M;
    A.box = reinterpret_cast<long long*>(d_box);
    const bool data = M.pred || M.nan_excluded;
    const size_t e = sizeof(T);
    bool vec = true;
    if (data) vec = vec && spc_aligned(in, 16) && (rs * e) % 16 == 0 && (ps * e) % 16 == 0;
    if (M.marr) vec = vec && spc_aligned(M.marr, 4) && M.mrs % 4 == 0 && M.mps % 4 == 0;
    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bb_init_kernel, dim3(1), dim3(64), 0, st, A.box);
    SPC_LAUNCH_CHECK();
    // about 4096 row-blocks per x tile: every block walks many rows, so the reductions and atomics stay rare
    const int64_t per_block = vec ? 4 * SC_BLOCK : SC_BLOCK;
    const unsigned gx = (unsigned)((nx + per_block - 1) / per_block);
    const int64_t gz = spc_min64(nz, 4096), gy = spc_min64(ny, sc_max(1, 4096 / gz));
    dim3 grid(gx, (unsigned)gy, (unsigned)gz);
    if (vec) {
        if (data) hipLaunchKernelGGL((bb_kernel<T, true, true>), grid, dim3(SC_BLOCK), 0, st, A);
        else hipLaunchKernelGGL((bb_kernel<T, true, false>), grid, dim3(SC_BLOCK), 0, st, A);
    } else {
        if (data) hipLaunchKernelGGL((bb_kernel<T, false, true>), grid, dim3(SC_BLOCK), 0, st, A);
        else hipLaunchKernelGGL((bb_kernel<T, false, false>), grid, dim3(SC_BLOCK), 0, st, A);
    }
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

template <typename T>
int sc_entry(int device, void* stream, const typename SpcAbi<T>::cube* cube, const typename SpcAbi<T>::mask* mask, int nan_excluded,
             const int64_t* start, const int64_t* step, int64_t nz_out, int64_t ny_out, int64_t nx_out, T* d_out,
             int64_t out_row_stride, int64_t out_plane_stride, uint8_t* d_out_mask, int filled, T fill) {
    int rc = spc_check_cube(cube);
    if (rc) return rc;
    SpcInclude<T> M;
    rc = spc_include_from(mask, cube, nan_excluded, &M);
    if (rc) return rc;
    return sc_run<T>(device, stream, cube->d_data, cube->nz, cube->ny, cube->nx, cube->row_stride, cube->plane_stride, M,
                     start, step, nz_out, ny_out, nx_out, d_out, out_row_stride, out_plane_stride, d_out_mask, filled, fill);
}

template <typename T>
int bb_entry(int device, void* stream, const typename SpcAbi<T>::cube* cube, const typename SpcAbi<T>::mask* mask, int nan_excluded,
             int64_t* d_box) {
    int rc = spc_check_cube(cube);
    if (rc) return rc;
    SpcInclude<T> M;
    rc = spc_include_from(mask, cube, nan_excluded, &M);
    if (rc) return rc;
    return bb_run<T>(device, stream, cube->d_data, cube->nz, cube->ny, cube->nx, cube->row_stride, cube->plane_stride, M, d_box);
}

}  // namespace

extern "C" {

int spc_subcube_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded,
                    const int64_t* start, const int64_t* step, int64_t nz_out, int64_t ny_out, int64_t nx_out,
                    float* d_out, int64_t out_row_stride, int64_t out_plane_stride, uint8_t* d_out_mask,
                    int filled, float fill) {
    return sc_entry<float>(device, stream, cube, mask, nan_excluded, start, step, nz_out, ny_out, nx_out, d_out, out_row_stride,
                           out_plane_stride, d_out_mask, filled, fill);
}

int spc_subcube_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded,
                    const int64_t* start, const int64_t* step, int64_t nz_out, int64_t ny_out, int64_t nx_out,
                    double* d_out, int64_t out_row_stride, int64_t out_plane_stride, uint8_t* d_out_mask,
                    int filled, double fill) {
    return sc_entry<double>(device, stream, cube, mask, nan_excluded, start, step, nz_out, ny_out, nx_out, d_out, out_row_stride,
                            out_plane_stride, d_out_mask, filled, fill);
}

int spc_mask_bbox_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded,
                      int64_t* d_box) {
    return bb_entry<float>(device, stream, cube, mask, nan_excluded, d_box);
}

int spc_mask_bbox_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded,
                      int64_t* d_box) {
    return bb_entry<double>(device, stream, cube, mask, nan_excluded, d_box);
}

}  // extern "C"
