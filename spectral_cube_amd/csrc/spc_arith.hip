// spc_arith.hip - cube arithmetic: SpectralCube.__add__ / __sub__ / __mul__ / __truediv__ / __pow__ (spectral_cube.py:2237-2361,
// _apply_everywhere :912-942, _cube_on_cube_operation :944-1003), a chain of up to SPC_ARITH_MAX_STEPS operators in one pass.
//
// Per voxel: a = sample, inc = include(a, mask) once on the source sample, v = a; every step first refills (v = inc ? v : fill,
// the filled_data an _apply_everywhere starts from) when its flag says so, then v = op(v, b); one store.  The steps travel as
// kernel arguments (wave-uniform: the step loop and the opcode switch do not diverge).
// A lane owns 4 consecutive x of one row, placed so that the chunks of the SOURCE row start on 16-byte (float) / 32-byte
// (double) boundaries: chunk g of a row covers x = 4 g - pad ... 4 g - pad + 3 with pad = (element address of the row) mod 4,
// so a misaligned row has a short first chunk (the head) and any row a short last one (the tail).  A whole chunk moves with
// 16-byte loads and stores when the output row, the mask row and every row operand sit at the same phase (decided per row, on
// the scalar unit); otherwise, and in head and tail, sample by sample.  An operand that is broadcast along x is one load per
// row and lane.  blockIdx.y / blockIdx.z stride over rows and planes (about 8192 blocks, each walking several rows): no axis
// length meets a grid limit.
//
// Exactness: + - * / x*x sqrt 1/x must be numpy's correctly rounded single operations, so nothing in this unit may contract
// a multiply and an add into an FMA (the Makefile's default is -ffp-contract=on), and division and sqrt are the IEEE ones.
#include "spc_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int AR_BLOCK = 256;
constexpr int64_t AR_GRID_LIMIT = 65535;
constexpr int64_t AR_BLOCKS_TARGET = 8192;                 // 256 CUs x 8 blocks x 4 rounds

enum { AR_SCALAR = 0, AR_ROW_CONST = 1, AR_ROW = 2 };     // operand: scalar / array broadcast along x / array with stride_x 1

template <typename T>
struct ArStep {
    int op, refill, kind;
    T s;
    const T* p;
    int64_t sz, sy;
};

template <typename T>
struct ArArgs {
    const T* in;
    int64_t nz, ny, nx, rs, ps;
    SpcInclude<T> m;
    T fill;
    int n;
    ArStep<T> st[SPC_ARITH_MAX_STEPS];
    T* out;
    int64_t ors, ops;
};

__device__ __forceinline__ void ar_load4(const float* p, float (&v)[4]) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
__device__ __forceinline__ void ar_load4(const double* p, double (&v)[4]) {
    const double2 a = *reinterpret_cast<const double2*>(p);
    const double2 b = *reinterpret_cast<const double2*>(p + 2);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
}
__device__ __forceinline__ void ar_store4(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void ar_store4(double* p, const double (&v)[4]) {
    *reinterpret_cast<double2*>(p) = make_double2(v[0], v[1]);
    *reinterpret_cast<double2*>(p + 2) = make_double2(v[2], v[3]);
}
__device__ __forceinline__ float ar_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double ar_sqrt(double v) { return sqrt(v); }
__device__ __forceinline__ float ar_pow(float v, float b) { return powf(v, b); }
__device__ __forceinline__ double ar_pow(double v, double b) { return pow(v, b); }

template <typename T>
__device__ __forceinline__ T ar_apply(int op, T v, T b) {
    switch (op) {
        case SPC_AOP_ADD: return v + b;
        case SPC_AOP_SUB: return v - b;
        case SPC_AOP_MUL: return v * b;
        case SPC_AOP_DIV: return v / b;
        case SPC_AOP_POW: return ar_pow(v, b);
        case SPC_AOP_SQUARE: return v * v;
        case SPC_AOP_SQRT: return ar_sqrt(v);
        case SPC_AOP_RECIP: return (T)1 / v;
        default: return (T)1;                                 // SPC_AOP_ONE
    }
}

// element address of a pointer, modulo 4 (the pointers are element-aligned: checked by the host)
template <typename T>
__device__ __forceinline__ int64_t ar_phase(const T* p) { return (int64_t)((uintptr_t)p / sizeof(T)) & 3; }

template <typename T>
__global__ __launch_bounds__(AR_BLOCK) void ar_kernel(const ArArgs<T> A) {
    const int64_t g = (int64_t)blockIdx.x * AR_BLOCK + threadIdx.x;
    for (int64_t z = blockIdx.z; z < A.nz; z += gridDim.z) {
        for (int64_t y = blockIdx.y; y < A.ny; y += gridDim.y) {
            const T* row = A.in + z * A.ps + y * A.rs;
            T* orow = A.out + z * A.ops + y * A.ors;
            const uint8_t* mrow = A.m.marr ? A.m.marr + z * A.m.mps + y * A.m.mrs : nullptr;
            const int64_t pad = ar_phase(row);
            // every array of this row at the phase of the source row: whole chunks are aligned in all of them
            bool ok = ar_phase(orow) == pad;
            if (mrow) ok = ok && ((int64_t)((uintptr_t)mrow & 3) == pad);
            // (formed for every step, whatever its kind - a scalar step has p == nullptr and strides 0 and never reads it:
            // a pointer that is a kernel argument plus an offset on every path stays a global one, a select with nullptr
            // made every operand load a flat load)
            const T* brow[SPC_ARITH_MAX_STEPS];
#pragma unroll
            for (int s = 0; s < SPC_ARITH_MAX_STEPS; ++s) {
                brow[s] = A.st[s].p + z * A.st[s].sz + y * A.st[s].sy;
                if (s < A.n && A.st[s].kind == AR_ROW) ok = ok && ar_phase(brow[s]) == pad;
            }
            const int64_t x0 = 4 * g - pad;
            if (x0 >= A.nx) continue;
            const bool whole = ok && x0 >= 0 && x0 + 4 <= A.nx;
            T v[4], b[SPC_ARITH_MAX_STEPS][4];
            uint8_t mb[4] = {1, 1, 1, 1};
            bool live[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) live[t] = whole || (x0 + t >= 0 && x0 + t < A.nx);
            if (whole) {
                ar_load4(row + x0, v);
                if (mrow) {
                    const uint32_t q = *reinterpret_cast<const uint32_t*>(mrow + x0);
#pragma unroll
                    for (int t = 0; t < 4; ++t) mb[t] = (uint8_t)(q >> (8 * t));
                }
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    v[t] = live[t] ? row[x0 + t] : (T)0;
                    if (mrow) mb[t] = live[t] ? mrow[x0 + t] : (uint8_t)0;
                }
            }
            // every operand is fetched before the first operation: the loads of a chain are in flight together
#pragma unroll
            for (int s = 0; s < SPC_ARITH_MAX_STEPS; ++s) {
                if (s >= A.n) continue;
                if (A.st[s].kind == AR_ROW) {
                    if (whole) {
                        ar_load4(brow[s] + x0, b[s]);
                    } else {
#pragma unroll
                        for (int t = 0; t < 4; ++t) b[s][t] = live[t] ? brow[s][x0 + t] : (T)0;
                    }
                } else {
                    const T c = A.st[s].kind == AR_ROW_CONST ? brow[s][0] : A.st[s].s;
#pragma unroll
                    for (int t = 0; t < 4; ++t) b[s][t] = c;
                }
            }
            bool inc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) inc[t] = spc_include(A.m, v[t], mb[t]);
#pragma unroll
            for (int s = 0; s < SPC_ARITH_MAX_STEPS; ++s) {
                if (s >= A.n) continue;
                const int op = A.st[s].op;
                const bool refill = A.st[s].refill != 0;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (refill) v[t] = inc[t] ? v[t] : A.fill;
                    v[t] = ar_apply(op, v[t], b[s][t]);
                }
            }
            if (whole) {
                ar_store4(orow + x0, v);
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (live[t]) orow[x0 + t] = v[t];
            }
        }
    }
}

struct ArSpan { uintptr_t lo, hi; };                         // bytes [lo, hi)
static inline ArSpan ar_span(const void* p, int64_t nz, int64_t ny, int64_t nx, int64_t sz, int64_t sy, int64_t sx, size_t e) {
    const uintptr_t lo = (uintptr_t)p;
    return ArSpan{lo, lo + (uintptr_t)((nz - 1) * sz + (ny - 1) * sy + (nx - 1) * sx + 1) * e};
}
static inline bool ar_overlap(ArSpan a, ArSpan b) { return a.lo < b.hi && b.lo < a.hi; }

template <typename T>
int ar_entry(int device, void* stream, const typename SpcAbi<T>::cube* cube, const typename SpcAbi<T>::mask* mask, int nan_excluded,
             T fill, const spc_arith_program* prog, T* d_out, int64_t out_row_stride, int64_t out_plane_stride) {
    int rc = spc_check_cube(cube);
    if (rc) return rc;
    SPC_REQUIRE(prog != nullptr, "prog is NULL");
    SPC_REQUIRE(d_out != nullptr, "d_out is NULL");
    SPC_REQUIRE(prog->n_steps >= 1, "an arithmetic program needs at least one step (got %d)", (int)prog->n_steps);
    SPC_REQUIRE(prog->n_steps <= SPC_ARITH_MAX_STEPS, "an arithmetic program holds at most %d steps (got %d)", SPC_ARITH_MAX_STEPS,
                (int)prog->n_steps);
    ArArgs<T> A{};
    A.in = cube->d_data;
    A.nz = cube->nz; A.ny = cube->ny; A.nx = cube->nx; A.rs = cube->row_stride; A.ps = cube->plane_stride;
    rc = spc_include_from<T>(mask, cube, nan_excluded, &A.m);
    if (rc) return rc;
    A.fill = fill;
    A.n = prog->n_steps;
    A.out = d_out;
    A.ors = out_row_stride ? out_row_stride : A.nx;
    A.ops = out_plane_stride ? out_plane_stride : A.ny * A.ors;
    SPC_REQUIRE(A.ors >= A.nx && A.ops >= A.ors * (A.ny - 1) + A.nx, "output strides too small for (%lld, %lld, %lld)",
                (long long)A.nz, (long long)A.ny, (long long)A.nx);
    const size_t e = sizeof(T);
    SPC_REQUIRE(spc_aligned(A.in, e) && spc_aligned(d_out, e), "cube / d_out not aligned to the sample size");
    const ArSpan out = ar_span(d_out, A.nz, A.ny, A.nx, A.ops, A.ors, 1, e);
    SPC_REQUIRE(!ar_overlap(out, ar_span(A.in, A.nz, A.ny, A.nx, A.ps, A.rs, 1, e)), "d_out overlaps the cube: arithmetic is not in place");
    if (A.m.marr)
        SPC_REQUIRE(!ar_overlap(out, ar_span(A.m.marr, A.nz, A.ny, A.nx, A.m.mps, A.m.mrs, 1, 1)), "d_out overlaps the mask array");
    for (int s = 0; s < A.n; ++s) {
        const spc_arith_step& S = prog->steps[s];
        ArStep<T>& D = A.st[s];
        SPC_REQUIRE(S.opcode >= SPC_AOP_ADD && S.opcode <= SPC_AOP_ONE, "step %d: unknown opcode %d", s, (int)S.opcode);
        D.op = S.opcode;
        D.refill = S.refill != 0;
        if (S.is_scalar) {
            SPC_REQUIRE(S.d_data == nullptr, "step %d: is_scalar is set but d_data is not NULL", s);
            D.kind = AR_SCALAR;
            D.s = (T)S.scalar;
            continue;
        }
        SPC_REQUIRE(S.d_data != nullptr, "step %d: an array operand with a NULL d_data", s);
        SPC_REQUIRE(S.opcode <= SPC_AOP_POW, "step %d: opcode %d takes no operand", s, (int)S.opcode);
        SPC_REQUIRE(S.stride_z >= 0 && S.stride_y >= 0 && (S.stride_x == 0 || S.stride_x == 1),
                    "step %d: operand strides (%lld, %lld, %lld): each >= 0 and stride_x 0 or 1", s, (long long)S.stride_z,
                    (long long)S.stride_y, (long long)S.stride_x);
        SPC_REQUIRE(spc_aligned(S.d_data, e), "step %d: operand not aligned to the sample size", s);
        SPC_REQUIRE(!ar_overlap(out, ar_span(S.d_data, A.nz, A.ny, A.nx, S.stride_z, S.stride_y, S.stride_x, e)),
                    "step %d: d_out overlaps the operand", s);
        D.kind = S.stride_x ? AR_ROW : AR_ROW_CONST;
        D.p = (const T*)S.d_data;
        D.sz = S.stride_z; D.sy = S.stride_y;
    }
    // the chunks of a row start up to 3 samples early unless every source row starts on a 4-sample boundary
    const bool rows_aligned = ((uintptr_t)A.in / e) % 4 == 0 && A.rs % 4 == 0 && A.ps % 4 == 0;
    const int64_t gx = (A.nx + (rows_aligned ? 0 : 3) + 4 * AR_BLOCK - 1) / (4 * AR_BLOCK);
    SPC_REQUIRE(gx <= 0x7fffffffLL, "nx too large (%lld)", (long long)A.nx);
    // about AR_BLOCKS_TARGET blocks, each walking several rows (neighbouring blocks take neighbouring rows): a block per row
    // of a 1024^3 cube is a million blocks of one 16-byte access per lane, and the time was the waves' prologues
    int64_t gz = spc_min64(A.nz, AR_GRID_LIMIT), gy = spc_min64(A.ny, AR_GRID_LIMIT);
    if (gx * gy * gz > AR_BLOCKS_TARGET) {
        gy = spc_min64(gy, (AR_BLOCKS_TARGET + gx * gz - 1) / (gx * gz));
        if (gx * gy * gz > AR_BLOCKS_TARGET) gz = spc_min64(gz, (AR_BLOCKS_TARGET + gx * gy - 1) / (gx * gy));
    }
    SPC_DEVICE(device);
    dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)gz);
    hipLaunchKernelGGL((ar_kernel<T>), grid, dim3(AR_BLOCK), 0, (hipStream_t)stream, A);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

}  // namespace

extern "C" {

int spc_arith_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded, float fill,
                  const spc_arith_program* prog, float* d_out, int64_t out_row_stride, int64_t out_plane_stride) {
    return ar_entry<float>(device, stream, cube, mask, nan_excluded, fill, prog, d_out, out_row_stride, out_plane_stride);
}

int spc_arith_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded, double fill,
                  const spc_arith_program* prog, double* d_out, int64_t out_row_stride, int64_t out_plane_stride) {
    return ar_entry<double>(device, stream, cube, mask, nan_excluded, fill, prog, d_out, out_row_stride, out_plane_stride);
}

}  // extern "C"
