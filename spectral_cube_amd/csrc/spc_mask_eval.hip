// spc_mask_eval.hip - a mask expression evaluated once on the device: the composition rules of the reference's mask tree
// (masks.py:239-250, 399-455: and / or / xor / not) over comparison terms (masks.py:670-758) whose threshold is a
// scalar, a spectrum, a map or a cube, np.isfinite terms and boolean arrays, on up to four cubes.
//
// The host compiles the tree into a postfix program (spc_mask_program, include/spcube_hip.h) that travels as kernel
// arguments: every lane of a launch runs the same instructions, so the interpreter loop is scalar control flow.  A lane
// owns 4 consecutive x of one row.  An include value per voxel is one bit, the 4 bits of a lane make one stack entry
// and the whole stack (8 entries) is ONE 32-bit register: push = shift left by 4, pop = shift right, the top is the low
// nibble - no indexed register array, no scratch.  Every data slot is loaded once per lane before the program runs,
// whatever the number of terms that name it; operands are loaded by the instruction that names them.
// The 4-voxel groups are laid out from the OUTPUT row's 4-byte alignment (the first group of a row may start before
// x = 0), so that every full group leaves in one aligned 4-byte store; a slot row whose groups then fall on 16-byte
// boundaries is read with 16-byte loads, any other row - and the partial groups at both ends - sample by sample.
#include "spc_common.h"

namespace {

constexpr int ME_BLOCK = 256;
constexpr int ME_W = 4;                               // consecutive x per lane = bits per stack entry
constexpr uint32_t ME_TOP = (1u << ME_W) - 1u;
constexpr int64_t ME_GRID_LIMIT = 65535;
static_assert(ME_W * SPC_MASK_PROG_MAX_STACK <= 32, "the stack of a lane is one 32-bit register");

struct MeArgs {
    spc_mask_program p;                               // strides resolved; pointers at the first row of this launch
    int64_t nz, nx;
    uint8_t* out;
    int64_t ors, ops;
};

__device__ __forceinline__ void me_load4(const float* p, float (&v)[4]) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
__device__ __forceinline__ void me_load4(const double* p, double (&v)[4]) {
    const double2 a = *reinterpret_cast<const double2*>(p);
    const double2 b = *reinterpret_cast<const double2*>(p + 2);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
}
__device__ __forceinline__ void me_load4(const uint8_t* p, uint8_t (&v)[4]) {
    const uint32_t q = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = (uint8_t)(q >> (8 * t));
}
// the widest load of 4 elements: 16 bytes (two of them for double), 4 bytes for uint8
template <typename E> __device__ __forceinline__ bool me_aligned4(const E* p) {
    return ((uintptr_t)p & (sizeof(E) * 4 > 16 ? 15 : sizeof(E) * 4 - 1)) == 0;
}

// 4 values of a row starting at sample x0 (x0 < 0 / x0 + 4 > nx at the ends of a row: *valid* has the bits of the
// samples inside it, the others read nothing and come out as 0), element stride sx: 0 = one value for the row
template <typename E>
__device__ __forceinline__ void me_row4(const E* row, int64_t x0, int64_t sx, uint32_t valid, E (&v)[4]) {
    if (sx == 0) {
        const E a = row[0];
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = a;
    } else if (sx == 1 && valid == ME_TOP && me_aligned4(row + x0)) {
        me_load4(row + x0, v);
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = ((valid >> t) & 1u) ? row[(x0 + t) * sx] : (E)0;
    }
}

template <typename E>
__device__ __forceinline__ void me_operand4(const spc_mask_operand& O, int64_t k, int64_t j, int64_t x0, uint32_t valid,
                                            double (&th)[4]) {
    E v[4];
    me_row4(reinterpret_cast<const E*>(O.d_data) + k * O.stride_z + j * O.stride_y, x0, O.stride_x, valid, v);
#pragma unroll
    for (int t = 0; t < 4; ++t) th[t] = (double)v[t];
}

__device__ __forceinline__ uint32_t me_compare(int cmp, const double (&x)[4], const double (&th)[4]) {
    uint32_t b = 0;
    switch (cmp) {                                    // uniform: one compare per voxel whichever it is
    case SPC_CMP_GT:
#pragma unroll
        for (int t = 0; t < 4; ++t) b |= (x[t] > th[t] ? 1u : 0u) << t;
        break;
    case SPC_CMP_GE:
#pragma unroll
        for (int t = 0; t < 4; ++t) b |= (x[t] >= th[t] ? 1u : 0u) << t;
        break;
    case SPC_CMP_LT:
#pragma unroll
        for (int t = 0; t < 4; ++t) b |= (x[t] < th[t] ? 1u : 0u) << t;
        break;
    case SPC_CMP_LE:
#pragma unroll
        for (int t = 0; t < 4; ++t) b |= (x[t] <= th[t] ? 1u : 0u) << t;
        break;
    case SPC_CMP_EQ:
#pragma unroll
        for (int t = 0; t < 4; ++t) b |= (x[t] == th[t] ? 1u : 0u) << t;
        break;
    default:                                          // SPC_CMP_NE: true when either side is NaN
#pragma unroll
        for (int t = 0; t < 4; ++t) b |= (x[t] != th[t] ? 1u : 0u) << t;
        break;
    }
    return b;
}

// blockIdx.x = tile of ME_BLOCK groups of 4 samples of a row, blockIdx.y = row, planes strided over gridDim.z
template <typename T>
__global__ __launch_bounds__(ME_BLOCK) void spc_mask_eval_kernel(const MeArgs A) {
    const int64_t j = blockIdx.y;
    const int64_t g = (int64_t)blockIdx.x * ME_BLOCK + threadIdx.x;
    for (int64_t k = blockIdx.z; k < A.nz; k += gridDim.z) {
        uint8_t* orow = A.out + k * A.ops + j * A.ors;
        const int shift = (int)((uintptr_t)orow & 3u);              // group g covers x = 4 g - shift ... + 3
        const int64_t x0 = g * ME_W - shift;
        if (x0 >= A.nx) continue;
        uint32_t valid = 0;
#pragma unroll
        for (int t = 0; t < ME_W; ++t) valid |= ((x0 + t >= 0 && x0 + t < A.nx) ? 1u : 0u) << t;

        T v[SPC_MASK_PROG_MAX_SLOTS][4];
#pragma unroll
        for (int s = 0; s < SPC_MASK_PROG_MAX_SLOTS; ++s) {
            if (s < A.p.n_slots) {
                me_row4(reinterpret_cast<const T*>(A.p.slots[s].d_data) + k * A.p.slots[s].plane_stride + j * A.p.slots[s].row_stride,
                        x0, (int64_t)1, valid, v[s]);
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) v[s][t] = (T)0;
            }
        }

        uint32_t stk = 0;
        for (int i = 0; i < A.p.n_instr; ++i) {
            const int op = A.p.instr[i].opcode;
            if (op == SPC_MOP_CMP || op == SPC_MOP_FINITE) {
                const int slot = A.p.instr[i].slot;
                double x[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {                       // a uniform select: v is never indexed at run time
                    T a = v[0][t];
#pragma unroll
                    for (int s = 1; s < SPC_MASK_PROG_MAX_SLOTS; ++s) a = (slot == s) ? v[s][t] : a;
                    x[t] = (double)a;
                }
                uint32_t b = 0;
                if (op == SPC_MOP_FINITE) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) b |= (fabs(x[t]) <= 1.7976931348623157e308 ? 1u : 0u) << t;
                } else {
                    const int oi = A.p.instr[i].operand;
                    double th[4];
                    if (oi < 0) {
                        const double imm = A.p.instr[i].imm;
#pragma unroll
                        for (int t = 0; t < 4; ++t) th[t] = imm;
                    } else {
                        const spc_mask_operand& O = A.p.operands[oi];
                        if (O.elem == SPC_ELEM_F32) me_operand4<float>(O, k, j, x0, valid, th);
                        else me_operand4<double>(O, k, j, x0, valid, th);
                    }
                    b = me_compare(A.p.instr[i].cmp, x, th);
                }
                stk = (stk << ME_W) | b;
            } else if (op == SPC_MOP_LOAD) {
                const spc_mask_operand& O = A.p.operands[A.p.instr[i].operand];
                uint8_t m[4];
                me_row4(reinterpret_cast<const uint8_t*>(O.d_data) + k * O.stride_z + j * O.stride_y, x0, O.stride_x, valid, m);
                uint32_t b = 0;
#pragma unroll
                for (int t = 0; t < 4; ++t) b |= (m[t] != 0 ? 1u : 0u) << t;
                stk = (stk << ME_W) | b;
            } else if (op == SPC_MOP_NOT) {
                stk ^= ME_TOP;
            } else {
                const uint32_t top = stk & ME_TOP, rest = stk >> ME_W;       // rest's low nibble is the other operand
                if (op == SPC_MOP_AND) stk = rest & (top | ~ME_TOP);
                else if (op == SPC_MOP_OR) stk = rest | top;
                else stk = rest ^ top;
            }
        }

        const uint32_t r = stk & ME_TOP;
        if (valid == ME_TOP) {
            *reinterpret_cast<uint32_t*>(orow + x0) = (r & 1u) | ((r & 2u) << 7) | ((r & 4u) << 14) | ((r & 8u) << 21);
        } else {
#pragma unroll
            for (int t = 0; t < ME_W; ++t)
                if ((valid >> t) & 1u) orow[x0 + t] = (uint8_t)((r >> t) & 1u);
        }
    }
}

// everything that can be wrong with a program, before any device work
int me_check(const spc_mask_program* p, int64_t nz, int64_t ny, int64_t nx, const uint8_t* d_out) {
    SPC_REQUIRE(p != nullptr, "program pointer is NULL");
    SPC_REQUIRE(d_out != nullptr, "d_out is NULL");
    SPC_REQUIRE(nz > 0 && ny > 0 && nx > 0, "cube shape must be positive (got %lld,%lld,%lld)", (long long)nz, (long long)ny,
                (long long)nx);
    SPC_REQUIRE(p->n_slots >= 0 && p->n_slots <= SPC_MASK_PROG_MAX_SLOTS, "%d data slots: at most %d", p->n_slots,
                SPC_MASK_PROG_MAX_SLOTS);
    SPC_REQUIRE(p->n_operands >= 0 && p->n_operands <= SPC_MASK_PROG_MAX_OPERANDS, "%d operands: at most %d", p->n_operands,
                SPC_MASK_PROG_MAX_OPERANDS);
    SPC_REQUIRE(p->n_instr >= 1 && p->n_instr <= SPC_MASK_PROG_MAX_INSTR, "%d instructions: 1 to %d", p->n_instr,
                SPC_MASK_PROG_MAX_INSTR);
    for (int s = 0; s < p->n_slots; ++s) {
        const spc_mask_slot& S = p->slots[s];
        SPC_REQUIRE(S.d_data != nullptr, "data slot %d: pointer is NULL", s);
        const int64_t rs = S.row_stride ? S.row_stride : nx, ps = S.plane_stride ? S.plane_stride : ny * rs;
        SPC_REQUIRE(rs >= nx && ps >= nx, "data slot %d: row / plane stride smaller than nx", s);
        SPC_REQUIRE(ps >= rs * (ny - 1) + nx || rs >= ps * (nz - 1) + nx, "data slot %d: overlapping rows and planes", s);
    }
    for (int o = 0; o < p->n_operands; ++o) {
        const spc_mask_operand& O = p->operands[o];
        SPC_REQUIRE(O.d_data != nullptr, "operand %d: pointer is NULL", o);
        SPC_REQUIRE(O.elem == SPC_ELEM_F32 || O.elem == SPC_ELEM_F64 || O.elem == SPC_ELEM_U8, "operand %d: unknown element type %d",
                    o, O.elem);
        SPC_REQUIRE(O.stride_z >= 0 && O.stride_y >= 0 && O.stride_x >= 0, "operand %d: negative stride", o);
    }
    int depth = 0;
    for (int i = 0; i < p->n_instr; ++i) {
        const spc_mask_instr& I = p->instr[i];
        switch (I.opcode) {
        case SPC_MOP_CMP:
            SPC_REQUIRE(I.cmp >= SPC_CMP_GT && I.cmp <= SPC_CMP_NE, "instruction %d: unknown comparison %d", i, I.cmp);
            SPC_REQUIRE(I.operand >= -1 && I.operand < p->n_operands, "instruction %d: operand %d out of range (%d operands)", i,
                        I.operand, p->n_operands);
            SPC_REQUIRE(I.operand < 0 || p->operands[I.operand].elem != SPC_ELEM_U8,
                        "instruction %d: CMP needs a float32 / float64 operand, operand %d is uint8", i, I.operand);
            [[fallthrough]];
        case SPC_MOP_FINITE:
            SPC_REQUIRE(I.slot >= 0 && I.slot < p->n_slots, "instruction %d: data slot %d out of range (%d slots)", i, I.slot,
                        p->n_slots);
            ++depth;
            break;
        case SPC_MOP_LOAD:
            SPC_REQUIRE(I.operand >= 0 && I.operand < p->n_operands, "instruction %d: operand %d out of range (%d operands)", i,
                        I.operand, p->n_operands);
            SPC_REQUIRE(p->operands[I.operand].elem == SPC_ELEM_U8, "instruction %d: LOAD needs a uint8 operand, operand %d is not", i,
                        I.operand);
            ++depth;
            break;
        case SPC_MOP_NOT:
            SPC_REQUIRE(depth >= 1, "instruction %d: NOT on an empty stack", i);
            break;
        case SPC_MOP_AND:
        case SPC_MOP_OR:
        case SPC_MOP_XOR:
            SPC_REQUIRE(depth >= 2, "instruction %d: stack underflow (%d value(s) for a binary operator)", i, depth);
            --depth;
            break;
        default:
            SPC_REQUIRE(false, "instruction %d: unknown opcode %d", i, I.opcode);
        }
        SPC_REQUIRE(depth <= SPC_MASK_PROG_MAX_STACK, "instruction %d: stack deeper than %d", i, SPC_MASK_PROG_MAX_STACK);
    }
    SPC_REQUIRE(depth == 1, "the program leaves %d values on the stack, not 1", depth);
    return SPC_OK;
}

template <typename T>
int me_run(int device, void* stream, int64_t nz, int64_t ny, int64_t nx, const spc_mask_program* prog, uint8_t* d_out,
           int64_t ors, int64_t ops) {
    const int rc = me_check(prog, nz, ny, nx, d_out);
    if (rc) return rc;
    MeArgs A{};
    A.p = *prog;
    A.nz = nz; A.nx = nx;
    A.out = d_out;
    A.ors = ors ? ors : nx;
    A.ops = ops ? ops : ny * A.ors;
    SPC_REQUIRE(A.ors >= nx && A.ops >= nx && (A.ops >= A.ors * (ny - 1) + nx || A.ors >= A.ops * (nz - 1) + nx),
                "output strides too small for (%lld, %lld, %lld)", (long long)nz, (long long)ny, (long long)nx);
    for (int s = 0; s < A.p.n_slots; ++s) {
        spc_mask_slot& S = A.p.slots[s];
        if (!S.row_stride) S.row_stride = nx;
        if (!S.plane_stride) S.plane_stride = ny * S.row_stride;
    }
    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    // a row holds at most (nx + 3) / 4 + 1 groups: the first one may start up to 3 samples before x = 0
    const int64_t groups = (nx + 3 + ME_W - 1) / ME_W;
    const unsigned gx = (unsigned)((groups + ME_BLOCK - 1) / ME_BLOCK);
    const unsigned gz = (unsigned)(nz < ME_GRID_LIMIT ? nz : ME_GRID_LIMIT);
    for (int64_t j0 = 0; j0 < ny; j0 += ME_GRID_LIMIT) {         // slabs of at most 65535 rows (gridDim.y)
        MeArgs S = A;
        const int64_t rows = ny - j0 < ME_GRID_LIMIT ? ny - j0 : ME_GRID_LIMIT;
        S.out = A.out + j0 * A.ors;
        for (int s = 0; s < S.p.n_slots; ++s)
            S.p.slots[s].d_data = reinterpret_cast<const T*>(A.p.slots[s].d_data) + j0 * A.p.slots[s].row_stride;
        for (int o = 0; o < S.p.n_operands; ++o) {
            const spc_mask_operand& O = A.p.operands[o];
            const size_t e = O.elem == SPC_ELEM_F64 ? 8 : (O.elem == SPC_ELEM_F32 ? 4 : 1);
            S.p.operands[o].d_data = reinterpret_cast<const char*>(O.d_data) + (size_t)(j0 * O.stride_y) * e;
        }
        hipLaunchKernelGGL((spc_mask_eval_kernel<T>), dim3(gx, (unsigned)rows, gz), dim3(ME_BLOCK), 0, st, S);
        SPC_LAUNCH_CHECK();
    }
    return SPC_OK;
}

}  // namespace

extern "C" {

int spc_mask_eval_f32(int device, void* stream, int64_t nz, int64_t ny, int64_t nx, const spc_mask_program* prog,
                      uint8_t* d_out, int64_t out_row_stride, int64_t out_plane_stride) {
    return me_run<float>(device, stream, nz, ny, nx, prog, d_out, out_row_stride, out_plane_stride);
}

int spc_mask_eval_f64(int device, void* stream, int64_t nz, int64_t ny, int64_t nx, const spc_mask_program* prog,
                      uint8_t* d_out, int64_t out_row_stride, int64_t out_plane_stride) {
    return me_run<double>(device, stream, nz, ny, nx, prog, d_out, out_row_stride, out_plane_stride);
}

}  // extern "C"
