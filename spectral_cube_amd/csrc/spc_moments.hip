// Fused masked moment 0/1/2 (+argmax/argmin/max/min/count) along the spectral
// axis of a (nz, ny, nx) float32 cube, for gfx950.
//
// Replaces (see include/spcube_hip.h for the full list):
//   spectral_cube/dask_spectral_cube.py:1083-1104, :54-59
//   spectral_cube/_moments.py:30-193, spectral_cube/np_compat.py:3-27
//   spectral_cube/spectral_cube.py:793-819 (argmax/argmin)
//
// Mapping: x is the fastest axis, so one lane owns VEC consecutive spaxels and
// marches over z; a wave reads 64*VEC*4 B contiguous per plane (1 KiB for
// VEC=4).  All sums are carried in fp64 registers (the reference computes in
// fp64; one-pass moment 2 from raw sums needs it).  The cube is read at most
// once: 4 B/voxel (+1 B/voxel with a uint8 mask array).
//
// Parallelism: blockDim = (64, ZW): the ZW waves of a block take interleaved
// planes of the same 64*VEC columns and are combined through LDS; gridDim.y
// splits z further when the map is too small to fill 256 CUs, with a second
// tiny combine kernel over fp64 partial sums.
//
// Issue budget (round 4, tools/micro/read_patterns.hip): this march reads 6.7 - 7.1 TB/s when nothing is
// computed, so the instructions per voxel decide whether the kernel is bound by HBM or by issue.  The mask
// predicate is therefore a template parameter in the canonical form of spc_canonical_pred (one compare when
// the mask has no threshold term, three otherwise - never the five flag-guarded compares of spc_pred), the
// valid count is only carried when it is asked for (otherwise one scalar "any valid" bit per column), the
// include select happens in float32 before the widening, the channel coordinate of a plane is a scalar load
// (the wave index goes through readfirstlane, so a plane's address and coordinate are provably uniform).
// 27.7 -> 12.4 instructions per voxel; the kernel now runs within 2 - 7 % of the same two streams read with no
// arithmetic at all (tools/micro/mask_patterns.hip), which is what is left of the 8 TB/s in this access pattern
// (profiles/r04_moments_issue.log).  SPC_MOMENTS_XCD=1 hands the blocks of one XCD neighbouring column groups
// (+3 % on the bare read, nothing on the kernel: off).
#include "spc_common.h"
#include <algorithm>
#include <cstdlib>

namespace {

constexpr int kLanes = 64;
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct MomArgs {
    const float* cube;
    int64_t nz, ny, nx, row_stride, plane_stride;
    MaskDev mask;
    const double* cen;
    double dv, m1_add;
    spc_moment_outputs out;
    int64_t out_row_stride;
    int64_t groups_per_row;  // nx / VEC
    int64_t ngroups;         // ny * groups_per_row
    int nsplit;              // gridDim.y
    int64_t zchunk;          // planes per split
    double* ws;              // partial sums workspace (nsplit > 1)
    float lim, lo, hi;       // the mask predicate in canonical form: |v| <= lim && !(v <= lo) && !(v >= hi)
    int xcd_group;           // blocks of one XCD take neighbouring column groups
    // the LIST forms only (include/spcube_hip.h, spc_moments_list_*): the entry rows of the included lane segments
    const f32x4* list_samples;      // [rows][64] the lane's four samples
    const uint32_t* list_meta;      // [rows][64] z | nibble << 28
    const uint64_t* list_off;       // [nblocks * nsplit * ZW] first entry row of a sublist
    const uint32_t* list_len;       // [nblocks * nsplit * ZW] its entry rows
    uint64_t list_rows;             // rows the two arrays hold
    // the VOXEL-LIST forms (LIST = 2, spc_moments_vlist_*) read the same fields, so that the arguments of every other form
    // keep their layout: list_samples is the entry array ([rows][64] of 8 bytes), list_off / list_len / list_rows are
    // voff / vlen / the voxel list's rows, list_meta is not read
};

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));   // an entry of the voxel list: { bits of v, meta }

// per-column running state
struct Acc {
    double s0, s1, s2;
    int n;
    bool any;                // EXT == 0: "a valid sample was met" instead of the count (a lane mask in scalar registers)
    float bmax, bmin;
    int imax, imin;
};

// EXT: 0 = the three sums (+ any-valid bit), 1 = + valid count, 2 = + extrema and their channels
constexpr int kSums = 0, kCount = 1, kExtrema = 2;

__device__ __forceinline__ void acc_init(Acc& a, int z0) {
    a.s0 = a.s1 = a.s2 = 0.0;
    a.n = 0;
    a.any = false;
    a.bmax = -INFINITY; a.bmin = INFINITY;
    a.imax = z0; a.imin = z0;
}

// PRED 0: |v| <= lim (lim = +inf: not NaN; FLT_MAX: finite), 1: the full canonical form
template <int PRED>
__device__ __forceinline__ bool mom_pred(float v, float lim, float lo, float hi) {
    bool ok = fabsf(v) <= lim;
    if (PRED) ok = ok && !(v <= lo) && !(v >= hi);
    return ok;
}

// ok already holds every term of the mask and rejects NaN
template <int EXT>
__device__ __forceinline__ void acc_add(Acc& a, float v, bool ok, double c, double c2, int z) {
    float w = ok ? v : 0.f;                  // select in float32 (one v_cndmask), then widen:
    asm volatile("" : "+v"(w));              // left alone LLVM widens first and selects both halves
    const double wd = (double)w;
    a.s0 += wd;
    a.s1 = fma(wd, c, a.s1);
    a.s2 = fma(wd, c2, a.s2);
    if (EXT >= kCount) a.n += ok ? 1 : 0;
    else a.any = a.any || ok;
    if (EXT == kExtrema) {
        const float hi = ok ? v : -INFINITY;
        const float lo = ok ? v : INFINITY;
        if (hi > a.bmax) { a.bmax = hi; a.imax = z; }
        if (lo < a.bmin) { a.bmin = lo; a.imin = z; }
    }
}

// merge b into a; ties keep the smaller channel index (first-index rule)
template <int EXT>
__device__ __forceinline__ void acc_merge(Acc& a, const Acc& b) {
    a.s0 += b.s0; a.s1 += b.s1; a.s2 += b.s2; a.n += b.n;
    if (EXT == kExtrema) {
        if (b.bmax > a.bmax || (b.bmax == a.bmax && b.imax < a.imax)) { a.bmax = b.bmax; a.imax = b.imax; }
        if (b.bmin < a.bmin || (b.bmin == a.bmin && b.imin < a.imin)) { a.bmin = b.bmin; a.imin = b.imin; }
    }
}

__device__ __forceinline__ void finalize(const MomArgs& A, const Acc& a, int64_t y, int64_t x) {
    const int64_t o = y * A.out_row_stride + x;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double mu = a.s1 / a.s0;  // 0/0 -> NaN for empty rays, like the reference
    if (A.out.d_m0) A.out.d_m0[o] = a.n > 0 ? A.dv * a.s0 : nan;
    if (A.out.d_m1) A.out.d_m1[o] = mu + A.m1_add;
    if (A.out.d_m2) A.out.d_m2[o] = a.s2 / a.s0 - mu * mu;
    if (A.out.d_mu) A.out.d_mu[o] = mu;
    if (A.out.d_s0) A.out.d_s0[o] = a.s0;
    if (A.out.d_argmax) A.out.d_argmax[o] = a.n > 0 ? (int64_t)a.imax : 0;
    if (A.out.d_argmin) A.out.d_argmin[o] = a.n > 0 ? (int64_t)a.imin : 0;
    if (A.out.d_vmax) A.out.d_vmax[o] = a.n > 0 ? a.bmax : NAN;
    if (A.out.d_vmin) A.out.d_vmin[o] = a.n > 0 ? a.bmin : NAN;
    if (A.out.d_nvalid) A.out.d_nvalid[o] = a.n;
}

// workspace layout for nsplit > 1: [split][field][column], 8 fields of 8 bytes
constexpr int kWsFields = 6;
__device__ __forceinline__ void ws_store(const MomArgs& A, const Acc& a, int split, int64_t col, int64_t ncols) {
    double* base = A.ws + (int64_t)split * kWsFields * ncols + col;
    base[0 * ncols] = a.s0;
    base[1 * ncols] = a.s1;
    base[2 * ncols] = a.s2;
    base[3 * ncols] = __longlong_as_double((long long)a.n);
    base[4 * ncols] = __longlong_as_double(((long long)__float_as_int(a.bmax) << 32) | (unsigned int)a.imax);
    base[5 * ncols] = __longlong_as_double(((long long)__float_as_int(a.bmin) << 32) | (unsigned int)a.imin);
}
__device__ __forceinline__ void ws_load(const MomArgs& A, Acc& a, int split, int64_t col, int64_t ncols) {
    const double* base = A.ws + (int64_t)split * kWsFields * ncols + col;
    a.s0 = base[0 * ncols];
    a.s1 = base[1 * ncols];
    a.s2 = base[2 * ncols];
    a.n = (int)__double_as_longlong(base[3 * ncols]);
    long long p = __double_as_longlong(base[4 * ncols]);
    a.bmax = __int_as_float((int)(p >> 32)); a.imax = (int)(p & 0xffffffffLL);
    p = __double_as_longlong(base[5 * ncols]);
    a.bmin = __int_as_float((int)(p >> 32)); a.imin = (int)(p & 0xffffffffLL);
}

template <int VEC> struct VecT;
template <> struct VecT<4> { using F = f32x4; using M = uint32_t; };   // 4 mask bytes in one dword
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <> struct VecT<2> { using F = f32x2; using M = uint16_t; };
template <> struct VecT<1> { using F = float; using M = unsigned char; };

__device__ __forceinline__ float vget(const f32x4& v, int i) { return v[i]; }
__device__ __forceinline__ float vget(const f32x2& v, int i) { return v[i]; }
__device__ __forceinline__ float vget(const float& v, int) { return v; }
__device__ __forceinline__ unsigned vget(const uint16_t& v, int i) { return (v >> (8 * i)) & 0xffu; }
__device__ __forceinline__ unsigned vget(const uint32_t& v, int i) { return (v >> (8 * i)) & 0xffu; }
__device__ __forceinline__ unsigned vget(const unsigned char& v, int) { return v; }

// MF (mask first; ARR and VEC = 4 only, SPC_MOMENTS_MASK_FIRST=0 turns it off): the mask dwords of a batch of U planes are
// loaded one batch ahead, and a lane issues the 16-byte load of its four samples only where its mask dword is not zero; the
// other lanes hold 0.f, which acc_add would have selected anyway (ok is false there whatever the sample is).  A 128-byte
// line of the cube in which the mask includes nothing is then never requested.  Everything after the loads is the same
// code in the same order, so the maps are bit-identical for every input, NaN and Inf under excluded voxels included.
//
// BITS (MF only): the mask of a plane is the lane's nibble of the packed form (layout: include/spcube_hip.h, spc_mask_pack_bits)
// instead of its four mask bytes: one unsigned-byte load from bits + (blk * nz + z) * 32 + (lane >> 1), an eighth of the mask's
// bytes.  "Nothing included" is nibble == 0 and voxel i is bit i; the batch of masks one ahead, the wait for all of them, the
// carried pointers, the tail, acc_add and the combine are the same statements, so the maps are those of the byte form bit for bit.
//
// LIST (BITS only): the loader alone differs.  The wave walks the entry rows of its sublist (layout: include/spcube_hip.h,
// spc_moments_list_*): U rows in flight, the metas and the samples of a batch back to back, all coalesced and unconditional.
// An entry is a plane of the lane that the bits include, with its nibble; the planes a lane's sublist leaves out are those for
// which the march adds +0.0 to every sum with ok false, which changes neither a sum (they start at +0.0 and round-to-nearest
// never makes -0.0 of these additions) nor the count, the any-valid bit or the extrema; a lane's entries keep the order of the
// march, and padding entries (meta 0, samples 0) are excluded planes.  So the maps are those of the march bit for bit.  The
// channel coordinate is a per-lane load (the lanes of a row hold different planes); cen is nz doubles and stays in the caches.
//
// LIST = 2, the voxel list (layout: include/spcube_hip.h, spc_moments_vlist_*): again the loader alone differs.  An entry is ONE
// included voxel of the lane - its sample, its plane and its place col in the lane's segment - and a row costs one 8-byte load
// per lane, so U = 16 rows in flight hold 32 registers where the list form holds 40 at U = 8.  Every entry goes through acc_add
// for all four columns with ok = mom_pred(v) && "an entry" && col == i.  Why the maps are the march's bit for bit: column i
// receives its included voxels in the order of the march (a lane's entries follow the list's order, which is the march's, and
// ascending col within a plane never reorders ONE column), each with the v, c, c2 and z the march passes; and every other call
// of acc_add for column i has ok false, which is exactly the call the march makes for an excluded voxel: w = 0.f, so s0 += +0.0
// and two fma(+0.0, c, s) with c the coordinate of a plane the march also adds at with ok false or true - they leave every sum as
// it is (no sum is ever -0.0: they start at +0.0 and round-to-nearest makes -0.0 only of (-0.0) + (-0.0)), and with ok false
// neither the count, the any-valid bit nor the extrema move.  Padding entries (all zero, bit 30 clear) are ok false in every
// column.  The columns' additions the march makes and this form leaves out are +0.0 additions of the same kind.
template <int VEC, int ZW, int U, bool ARR, int EXT, int PRED, bool MF = false, bool BITS = false, int LIST = 0>
__global__ __launch_bounds__(kLanes * ZW) void moments_kernel(const MomArgs A) {
    static_assert(!MF || (ARR && VEC == 4), "mask-first is the 16-byte lane form with a mask array");
    static_assert(!BITS || MF, "the packed mask is read by the mask-first forms only");
    static_assert(!LIST || BITS, "the list holds what the packed mask includes");
    using F = typename VecT<VEC>::F;
    using M = typename VecT<VEC>::M;
    const int lane = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.y);   // blockDim.x = 64: one wave per y
    // the hardware hands consecutive blocks to consecutive XCDs: give the blocks of one XCD one contiguous range of
    // column groups (their 1-KiB row segments then follow each other in that XCD's L2 channels and DRAM pages)
    int64_t blk = blockIdx.x;
    if (A.xcd_group) {
        const int64_t nb = gridDim.x, q = nb >> 3, r = nb & 7, k = blk & 7;
        blk = k * q + (k < r ? k : r) + (blk >> 3);
    }
    const int64_t g = blk * kLanes + lane;
    const bool live = g < A.ngroups;
    const int64_t gg = live ? g : 0;
    const int64_t y = gg / A.groups_per_row;
    const int64_t x = (gg - y * A.groups_per_row) * VEC;
    const int split = blockIdx.y;
    const int64_t zb = (int64_t)split * A.zchunk;
    const int64_t ze = min(A.nz, zb + A.zchunk);

    const float* p = A.cube + y * A.row_stride + x;
    const uint8_t* pm = ARR ? A.mask.arr + y * A.mask.row_stride + x : nullptr;
    const float lim = A.lim, lo = A.lo, hi = A.hi;
    // the channel coordinates through the constant address space: a uniform index is then ALWAYS a scalar load (left in the
    // global address space the ZW = 8 instantiation fell back to eight per-lane loads per iteration - the no-clobber analysis
    // that licenses a scalar load of global memory gives up on the larger kernel)
    typedef const double __attribute__((address_space(4))) cdouble;
    cdouble* cenp = (cdouble*)A.cen;

    Acc acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc_init(acc[i], (int)min(zb + w, ze - 1));

    if (live) {
        int64_t z = zb + w;
        // main loop: U planes (stride ZW) in flight per lane
        if constexpr (LIST == 2) {
            // one voxel of a lane into the column it belongs to; the other three columns add +0.0 (see above the kernel)
            auto add_voxel = [&](const u32x2& e) {
                const uint32_t mt = e.y;
                const float val = __uint_as_float(e.x);
                const int zz = (int)min((int64_t)(mt & 0x0fffffffu), A.nz - 1);
                const double c = A.cen[zz];
                const double c2 = c * c;
                const bool in = mom_pred<PRED>(val, lim, lo, hi) && ((mt >> 30) & 1u) != 0;
                const uint32_t col = (mt >> 28) & 3u;
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc_add<EXT>(acc[i], val, in && col == (uint32_t)i, c, c2, zz);
            };
            // the sublist of this wave: wave-uniform indices, scalar loads
            typedef const uint64_t __attribute__((address_space(4))) cu64;
            typedef const uint32_t __attribute__((address_space(4))) cu32;
            const int64_t sub = (blk * A.nsplit + split) * ZW + w;
            const uint64_t row = ((cu64*)A.list_off)[sub];
            uint32_t n = ((cu32*)A.list_len)[sub];
            if (row > A.list_rows || n > A.list_rows - row) n = 0;   // never past the array, whatever voff and vlen hold
            typedef const u32x2 __attribute__((address_space(1))) GE;
            GE* pe = (GE*)A.list_samples + row * kLanes + lane;
            uint32_t k = 0;
            for (; k + U <= n; k += U, pe += U * kLanes) {
                u32x2 e[U];
#pragma unroll
                for (int u = 0; u < U; ++u) e[u] = __builtin_nontemporal_load(pe + u * kLanes);
#pragma unroll
                for (int u = 0; u < U; ++u) add_voxel(e[u]);
            }
            for (; k < n; ++k, pe += kLanes) {
                const u32x2 e = *pe;
                add_voxel(e);
            }
        } else if constexpr (LIST) {
            // one entry of a lane: add_plane of the march below, with the lane's own plane number and coordinate (a plane number
            // past the cube, which no filled list holds, reads the last coordinate instead of memory that is not cen's)
            auto add_entry = [&](const F& v, uint32_t mt) {
                const int zz = (int)min((int64_t)(mt & 0x0fffffffu), A.nz - 1);
                const uint32_t m = mt >> 28;
                const double c = A.cen[zz];
                const double c2 = c * c;
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    const float val = vget(v, i);
                    bool ok = mom_pred<PRED>(val, lim, lo, hi);
                    ok = ok && ((m >> i) & 1u) != 0;
                    acc_add<EXT>(acc[i], val, ok, c, c2, zz);
                }
            };
            // the sublist of this wave: wave-uniform indices, scalar loads
            typedef const uint64_t __attribute__((address_space(4))) cu64;
            typedef const uint32_t __attribute__((address_space(4))) cu32;
            const int64_t sub = (blk * A.nsplit + split) * ZW + w;
            const uint64_t row = ((cu64*)A.list_off)[sub];
            uint32_t n = ((cu32*)A.list_len)[sub];
            if (row + n > A.list_rows) n = 0;                    // never past the arrays, whatever off and len hold
            typedef const F __attribute__((address_space(1))) GF;
            typedef const uint32_t __attribute__((address_space(1))) GU;
            GF* ps = (GF*)A.list_samples + row * kLanes + lane;
            GU* pq = (GU*)A.list_meta + row * kLanes + lane;
            uint32_t k = 0;
            for (; k + U <= n; k += U, ps += U * kLanes, pq += U * kLanes) {
                uint32_t mt[U];
                F v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) mt[u] = __builtin_nontemporal_load(pq + u * kLanes);
#pragma unroll
                for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(ps + u * kLanes);
#pragma unroll
                for (int u = 0; u < U; ++u) add_entry(v[u], mt[u]);
            }
            for (; k < n; ++k, ps += kLanes, pq += kLanes) {
                const uint32_t mt = *pq;
                const F v = *ps;
                add_entry(v, mt);
            }
        } else if constexpr (MF) {
            // one plane of a lane: its VEC samples and mask bytes into the sums
            auto add_plane = [&](const F& v, const M& m, int64_t zz) {
                const double c = cenp[zz];                           // uniform index: a scalar load
                const double c2 = c * c;
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    const float val = vget(v, i);
                    bool ok = mom_pred<PRED>(val, lim, lo, hi);
                    if constexpr (BITS) ok = ok && ((m >> i) & 1u) != 0;
                    else if (ARR) ok = ok && (vget(m, i) != 0);
                    acc_add<EXT>(acc[i], val, ok, c, c2, (int)zz);
                }
            };
            // two carried pointers, made opaque once per batch, and every address of a batch the one before plus the uniform
            // plane step (left to itself the loop optimiser keeps 2 U pointers in registers: 124 VGPRs instead of 80)
            const int64_t dstep = (int64_t)ZW * A.plane_stride, mstep = BITS ? (int64_t)ZW * 32 : (int64_t)ZW * A.mask.plane_stride;
            // (pointers to global memory by type: one that went through the asm statement as a plain pointer is loaded from with
            //  flat_load, which also counts in lgkmcnt, where the scalar loads of the coordinates wait)
            typedef const float __attribute__((address_space(1))) gfloat;
            typedef const uint8_t __attribute__((address_space(1))) gbyte;
            typedef const F __attribute__((address_space(1))) GF;
            typedef const M __attribute__((address_space(1))) GM;
            gfloat* pz = (gfloat*)(p + z * A.plane_stride);      // the samples of plane z ...
            // (BITS: A.mask.arr is the packed form - launch_main - and this the byte that holds the lane's nibble)
            gbyte* qz = BITS ? (gbyte*)(A.mask.arr + (blk * A.nz + z) * 32 + (lane >> 1))
                             : (gbyte*)(pm + z * A.mask.plane_stride);  // ... and the first mask that has not been asked for yet
            // the odd lanes own the high nibble of their byte.  The shift runs under the lane mask (scalar registers) and in place:
            // a shift amount kept in a vector register, or a nibble written beside its byte, costs <4, 8, 8, sums> a wave per SIMD
            const bool odd = (lane & 1) != 0;
            // the mask of the plane at q.  BITS: the byte as it comes (a plain load: the waves of a block share its line); it becomes
            // the lane's four bits once the whole batch has been waited for
            auto load_mask = [&](gbyte* q) -> M {
                if constexpr (BITS) return (M)*q;
                else return __builtin_nontemporal_load((GM*)q);
            };

            bool more = z + (int64_t)(U - 1) * ZW < ze;
            M m[U];                                              // the masks of the batch that starts at z
            if (more) {
#pragma unroll
                for (int u = 0; u < U; ++u, qz += mstep) m[u] = load_mask(qz);
            }
            while (more) {
                // every mask of the batch is waited for here, before the first load it decides: the loads of the samples then
                // go out back to back (waited for one by one, the last mask would be waited for behind the samples already asked for)
                M all = m[0];
#pragma unroll
                for (int u = 1; u < U; ++u) all |= m[u];
                asm volatile("" : "+v"(pz), "+v"(qz) : "v"(all));
                if constexpr (BITS) {
                    if (odd) {
#pragma unroll
                        for (int u = 0; u < U; ++u) asm volatile("v_lshrrev_b32 %0, 4, %0" : "+v"(m[u]));
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) asm volatile("v_and_b32 %0, 15, %0" : "+v"(m[u]));
                }
                F v[U];
#pragma unroll
                for (int u = 0; u < U; ++u, pz += dstep) {
                    v[u] = F{};
                    if (m[u] != 0) v[u] = __builtin_nontemporal_load((GF*)pz);
                }
                more = z + (int64_t)(2 * U - 1) * ZW < ze;       // wave-uniform
                // the next batch's mask of plane u goes out as soon as this batch's has been used, into the same register
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    add_plane(v[u], m[u], z + (int64_t)u * ZW);
                    if (more) { m[u] = load_mask(qz); qz += mstep; }
                }
                z += (int64_t)U * ZW;
            }
            // tail
            for (; z < ze; z += ZW, pz += dstep, qz += mstep) {
                F v{};
                M mt;
                if constexpr (BITS) mt = ((M)*qz >> (odd ? 4 : 0)) & 0xfu;
                else mt = *(GM*)qz;
                if (mt != 0) v = *(GF*)pz;
                add_plane(v, mt, z);
            }
        } else {
            for (; z + (int64_t)(U - 1) * ZW < ze; z += (int64_t)U * ZW) {
                F v[U];
                M m[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t zz = z + (int64_t)u * ZW;
                    v[u] = __builtin_nontemporal_load(reinterpret_cast<const F*>(p + zz * A.plane_stride));
                    if (ARR) m[u] = __builtin_nontemporal_load(reinterpret_cast<const M*>(pm + zz * A.mask.plane_stride));
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t zz = z + (int64_t)u * ZW;
                    const double c = cenp[zz];                       // uniform index: a scalar load
                    const double c2 = c * c;
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        const float val = vget(v[u], i);
                        bool ok = mom_pred<PRED>(val, lim, lo, hi);
                        if (ARR) ok = ok && (vget(m[u], i) != 0);
                        acc_add<EXT>(acc[i], val, ok, c, c2, (int)zz);
                    }
                }
            }
            // tail
            for (; z < ze; z += ZW) {
                const F v = *reinterpret_cast<const F*>(p + z * A.plane_stride);
                M m = 0;
                if (ARR) m = *reinterpret_cast<const M*>(pm + z * A.mask.plane_stride);
                const double c = cenp[z];
                const double c2 = c * c;
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    const float val = vget(v, i);
                    bool ok = mom_pred<PRED>(val, lim, lo, hi);
                    if (ARR) ok = ok && (vget(m, i) != 0);
                    acc_add<EXT>(acc[i], val, ok, c, c2, (int)z);
                }
            }
        }
    }
    // where the lane's results go.  MF: worked out again from the lane number instead of being kept through the march: seven
    // registers, which the march needs to stay at the waves per SIMD of the loop that loads everything (<4,4,8,sums>: 85 -> 79
    // VGPRs, six waves)
    int64_t og = g, oy = y, ox = x;
    bool olive = live;
    if constexpr (MF) {
        int ln = threadIdx.x;
        asm volatile("" : "+v"(ln));
        og = blk * kLanes + ln;
        olive = og < A.ngroups;
        const int64_t ogg = olive ? og : 0;
        oy = ogg / A.groups_per_row;
        ox = (ogg - oy * A.groups_per_row) * VEC;
    }
    if (EXT < kCount) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i].n = acc[i].any ? 1 : 0;
    }

    // ---- combine the ZW waves of the block through LDS (one VEC element at a time)
    if (ZW > 1) {
        __shared__ double sh[(ZW > 1 ? ZW - 1 : 1) * 6 * kLanes];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            if (w > 0) {
                double* s = sh + (w - 1) * 6 * kLanes + lane;
                s[0 * kLanes] = acc[i].s0;
                s[1 * kLanes] = acc[i].s1;
                s[2 * kLanes] = acc[i].s2;
                s[3 * kLanes] = __longlong_as_double((long long)acc[i].n);
                s[4 * kLanes] = __longlong_as_double(((long long)__float_as_int(acc[i].bmax) << 32) | (unsigned int)acc[i].imax);
                s[5 * kLanes] = __longlong_as_double(((long long)__float_as_int(acc[i].bmin) << 32) | (unsigned int)acc[i].imin);
            }
            __syncthreads();
            if (w == 0) {
#pragma unroll
                for (int ww = 1; ww < ZW; ++ww) {
                    const double* s = sh + (ww - 1) * 6 * kLanes + lane;
                    Acc b;
                    b.s0 = s[0 * kLanes]; b.s1 = s[1 * kLanes]; b.s2 = s[2 * kLanes];
                    b.n = (int)__double_as_longlong(s[3 * kLanes]);
                    long long q = __double_as_longlong(s[4 * kLanes]);
                    b.bmax = __int_as_float((int)(q >> 32)); b.imax = (int)(q & 0xffffffffLL);
                    q = __double_as_longlong(s[5 * kLanes]);
                    b.bmin = __int_as_float((int)(q >> 32)); b.imin = (int)(q & 0xffffffffLL);
                    acc_merge<EXT>(acc[i], b);
                }
            }
            __syncthreads();
        }
    }

    if (w == 0 && olive) {
        const int64_t ncols = A.ngroups * VEC;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            if (A.nsplit == 1) finalize(A, acc[i], oy, ox + i);
            else ws_store(A, acc[i], split, og * VEC + i, ncols);
        }
    }
}

template <int EXT>
__global__ __launch_bounds__(256) void moments_combine_kernel(const MomArgs A, int vec) {
    const int64_t ncols = A.ngroups * vec;
    const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= ncols) return;
    Acc a;
    ws_load(A, a, 0, col, ncols);
    for (int s = 1; s < A.nsplit; ++s) {
        Acc b;
        ws_load(A, b, s, col, ncols);
        acc_merge<EXT>(a, b);
    }
    const int64_t g = col / vec;
    const int64_t y = g / A.groups_per_row;
    const int64_t x = (g - y * A.groups_per_row) * vec + (col - g * vec);
    finalize(A, a, y, x);
}

// ---- second pass for order N: sum v*(c-mu)^N / S0 -------------------------
struct OrdArgs {
    const float* cube;
    int64_t nz, ny, nx, row_stride, plane_stride;
    MaskDev mask;
    const double* cen;
    const double* mu;
    const double* s0;
    double* out;
    int64_t out_row_stride;
    int order;
};

__global__ __launch_bounds__(256) void moment_order_kernel(const OrdArgs A) {
    const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= A.ny * A.nx) return;
    const int64_t y = col / A.nx, x = col - y * A.nx;
    const float* p = A.cube + y * A.row_stride + x;
    const uint8_t* pm = (A.mask.flags & SPC_MASK_ARRAY) ? A.mask.arr + y * A.mask.row_stride + x : nullptr;
    const double mu = A.mu[y * A.out_row_stride + x];
    double s = 0.0;
    for (int64_t z = 0; z < A.nz; ++z) {
        const float v = p[z * A.plane_stride];
        bool inc = spc_pred(A.mask.flags, A.mask.thr_lo, A.mask.thr_hi, v);
        if (pm) inc = inc && pm[z * A.mask.plane_stride] != 0;
        if (inc && v == v) {
            const double d = A.cen[z] - mu;
            double pw = d;
            for (int k = 1; k < A.order; ++k) pw *= d;
            s = fma((double)v, pw, s);
        }
    }
    A.out[y * A.out_row_stride + x] = s / A.s0[y * A.out_row_stride + x];
}

// same sum with the access pattern of the main kernel: a lane owns 4 adjacent spaxels (16-byte loads),
// the 4 waves of a block split z (4 planes in flight), LDS combine
template <bool ARR>
__global__ __launch_bounds__(256) void moment_order_v4_kernel(const OrdArgs A) {
    constexpr int ZW = 4, U = 4;
    typedef float f32x4o __attribute__((ext_vector_type(4)));
    __shared__ double sh[ZW - 1][4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t gpr = A.nx / 4;
    const int64_t g = (int64_t)blockIdx.x * 64 + lane;
    const bool live = g < A.ny * gpr;
    const int64_t gg = live ? g : 0;
    const int64_t y = gg / gpr, x = (gg - y * gpr) * 4;
    const float* p = A.cube + y * A.row_stride + x;
    const uint8_t* pm = ARR ? A.mask.arr + y * A.mask.row_stride + x : nullptr;
    double mu[4], s[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { mu[c] = A.mu[y * A.out_row_stride + x + c]; s[c] = 0.0; }
    for (int64_t z0 = w; z0 < A.nz; z0 += ZW * U) {
        f32x4o v[U];
        uint32_t m[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t z = min(z0 + (int64_t)u * ZW, A.nz - 1);
            v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4o*>(p + z * A.plane_stride));
            m[u] = ARR ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(pm + z * A.mask.plane_stride)) : 0x01010101u;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t z = z0 + (int64_t)u * ZW;
            if (z >= A.nz) break;                              // wave-uniform
            const double cz = A.cen[z];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float val = v[u][c];
                const bool ok = spc_pred_valid(A.mask, val) & (((m[u] >> (8 * c)) & 0xffu) != 0);
                const double d = cz - mu[c];
                double pw = d;
                for (int k = 1; k < A.order; ++k) pw *= d;
                s[c] = fma(ok ? (double)val : 0.0, ok ? pw : 0.0, s[c]);
            }
        }
    }
    if (w > 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) sh[w - 1][c][lane] = s[c];
    }
    __syncthreads();
    if (w != 0 || !live) return;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int k = 0; k < ZW - 1; ++k) s[c] += sh[k][c][lane];
        A.out[y * A.out_row_stride + x + c] = s[c] / A.s0[y * A.out_row_stride + x + c];
    }
}

// bits: the packed mask array, or nullptr; list_u: 0, or the rows in flight of the LIST form that reads A.list_* (4 or 8);
// vlist_u: 0, or the rows in flight of the voxel-list form (LIST = 2) that reads A.list_* as a voxel list (8 or 16)
struct Plan { int vec, zw, u, nsplit; int64_t zchunk; bool mask_first; const uint8_t* bits; int list_u; int vlist_u; };

template <int VEC, int ZW, int U, bool ARR, int EXT>
int launch_main(const MomArgs& A, hipStream_t st, bool thresholds, bool mask_first, const uint8_t* bits, int list_u, int vlist_u) {
    dim3 block(kLanes, ZW);
    dim3 grid((unsigned)((A.ngroups + kLanes - 1) / kLanes), (unsigned)A.nsplit);
    if constexpr (ARR && VEC == 4) {
        if (mask_first && bits) {
            // the BITS forms never read the byte array: its pointer carries the packed form, so that the arguments keep the
            // layout (and every other instantiation the instructions) they had
            MomArgs B = A;
            B.mask.arr = bits;
            if (vlist_u) {
                // the voxel-list forms: the plan's ZW and split, U rows of 8-byte entries in flight
                if (vlist_u == 16) {
                    if (thresholds) hipLaunchKernelGGL((moments_kernel<VEC, ZW, 16, ARR, EXT, 1, true, true, 2>), grid, block, 0, st, B);
                    else hipLaunchKernelGGL((moments_kernel<VEC, ZW, 16, ARR, EXT, 0, true, true, 2>), grid, block, 0, st, B);
                } else {
                    if (thresholds) hipLaunchKernelGGL((moments_kernel<VEC, ZW, 8, ARR, EXT, 1, true, true, 2>), grid, block, 0, st, B);
                    else hipLaunchKernelGGL((moments_kernel<VEC, ZW, 8, ARR, EXT, 0, true, true, 2>), grid, block, 0, st, B);
                }
                SPC_LAUNCH_CHECK();
                return SPC_OK;
            }
            if (list_u) {
                // the LIST forms: the plan's ZW and split with a batch of their own (U counts planes in the march, rows here)
                if (list_u == 8) {
                    if (thresholds) hipLaunchKernelGGL((moments_kernel<VEC, ZW, 8, ARR, EXT, 1, true, true, 1>), grid, block, 0, st, B);
                    else hipLaunchKernelGGL((moments_kernel<VEC, ZW, 8, ARR, EXT, 0, true, true, 1>), grid, block, 0, st, B);
                } else {
                    if (thresholds) hipLaunchKernelGGL((moments_kernel<VEC, ZW, 4, ARR, EXT, 1, true, true, 1>), grid, block, 0, st, B);
                    else hipLaunchKernelGGL((moments_kernel<VEC, ZW, 4, ARR, EXT, 0, true, true, 1>), grid, block, 0, st, B);
                }
                SPC_LAUNCH_CHECK();
                return SPC_OK;
            }
            if (thresholds) hipLaunchKernelGGL((moments_kernel<VEC, ZW, U, ARR, EXT, 1, true, true>), grid, block, 0, st, B);
            else hipLaunchKernelGGL((moments_kernel<VEC, ZW, U, ARR, EXT, 0, true, true>), grid, block, 0, st, B);
            SPC_LAUNCH_CHECK();
            return SPC_OK;
        }
        if (mask_first) {
            if (thresholds) hipLaunchKernelGGL((moments_kernel<VEC, ZW, U, ARR, EXT, 1, true>), grid, block, 0, st, A);
            else hipLaunchKernelGGL((moments_kernel<VEC, ZW, U, ARR, EXT, 0, true>), grid, block, 0, st, A);
            SPC_LAUNCH_CHECK();
            return SPC_OK;
        }
    }
    if (thresholds) hipLaunchKernelGGL((moments_kernel<VEC, ZW, U, ARR, EXT, 1>), grid, block, 0, st, A);
    else hipLaunchKernelGGL((moments_kernel<VEC, ZW, U, ARR, EXT, 0>), grid, block, 0, st, A);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

// 16-byte lanes: ZW in {1, 4, 8}, U in {2, 4, 8}; the narrower lanes (odd nx, unaligned views): ZW in {1, 4}, U = 4
// Mask-first forms (launch_main): their register counts rest on three things that a compiler change can undo - the empty asm
// statements on the carried pointers and on the lane number, and the global address space of the pointers (see the kernel) -
// so check -Rpass-analysis=kernel-resource-usage after one (profiles/moments_mask_first_bench.txt has the table: <4,4,8,sums,0>
// 79 VGPRs, six waves per SIMD).  Two groups of mask-first forms hold a wave per SIMD fewer than the loop that loads everything
// and are not what make_plan picks: U = 8 with extrema (all eight 16-byte loads stay live across the branches: 131 - 134 VGPRs;
// make_plan takes U = 2 with extrema) and <4,1,8,count,0> (81 VGPRs; ZW = 1 is for cubes of fewer than 16 planes).  They are
// reached through SPC_MOMENTS_U / SPC_MOMENTS_ZW only.
// The BITS forms beside them (profiles/moments_mask_bits_resources.txt): <4,4,8,sums,0> 77 VGPRs, <4,8,8,sums,0> 79, six waves
// each; they rest on the nibble being shifted and masked IN PLACE (the asm statements in the kernel): with a shift amount in
// a vector register <4,8,8,sums> held 82 and five waves and a nearly empty mask ran 8 % slower than on its bytes.
// <4,4,8,count,0> holds 81 against the byte form's 80: five waves against six (and still gains what the sums form gains).
template <bool ARR, int EXT>
int launch_plan(const MomArgs& A, hipStream_t st, const Plan& p, bool thr) {
    if (p.vec == 4) {
        switch (p.zw * 16 + p.u) {
            case 1 * 16 + 2: return launch_main<4, 1, 2, ARR, EXT>(A, st, thr, p.mask_first, p.bits, p.list_u, p.vlist_u);
            case 1 * 16 + 4: return launch_main<4, 1, 4, ARR, EXT>(A, st, thr, p.mask_first, p.bits, p.list_u, p.vlist_u);
            case 1 * 16 + 8: return launch_main<4, 1, 8, ARR, EXT>(A, st, thr, p.mask_first, p.bits, p.list_u, p.vlist_u);
            case 4 * 16 + 2: return launch_main<4, 4, 2, ARR, EXT>(A, st, thr, p.mask_first, p.bits, p.list_u, p.vlist_u);
            case 4 * 16 + 4: return launch_main<4, 4, 4, ARR, EXT>(A, st, thr, p.mask_first, p.bits, p.list_u, p.vlist_u);
            case 4 * 16 + 8: return launch_main<4, 4, 8, ARR, EXT>(A, st, thr, p.mask_first, p.bits, p.list_u, p.vlist_u);
            case 8 * 16 + 2: return launch_main<4, 8, 2, ARR, EXT>(A, st, thr, p.mask_first, p.bits, p.list_u, p.vlist_u);
            case 8 * 16 + 4: return launch_main<4, 8, 4, ARR, EXT>(A, st, thr, p.mask_first, p.bits, p.list_u, p.vlist_u);
            default: return launch_main<4, 8, 8, ARR, EXT>(A, st, thr, p.mask_first, p.bits, p.list_u, p.vlist_u);
        }
    }
    if (p.vec == 2) return p.zw > 1 ? launch_main<2, 4, 4, ARR, EXT>(A, st, thr, p.mask_first, p.bits, p.list_u, p.vlist_u) : launch_main<2, 1, 4, ARR, EXT>(A, st, thr, p.mask_first, p.bits, p.list_u, p.vlist_u);
    return p.zw > 1 ? launch_main<1, 4, 4, ARR, EXT>(A, st, thr, p.mask_first, p.bits, p.list_u, p.vlist_u) : launch_main<1, 1, 4, ARR, EXT>(A, st, thr, p.mask_first, p.bits, p.list_u, p.vlist_u);
}

Plan make_plan(const spc_cube_f32* c, const MaskDev& m, bool ext) {
    Plan p;
    p.bits = nullptr;
    p.list_u = 0;
    p.vlist_u = 0;
    auto aligned = [&](int v) {
        const bool arr = (m.flags & SPC_MASK_ARRAY) != 0;
        return (c->nx % v == 0) && (c->row_stride % v == 0) && (c->plane_stride % v == 0) &&
               (((uintptr_t)c->d_data) % (4 * v) == 0) &&
               (!arr || ((m.row_stride % v == 0) && (m.plane_stride % v == 0) && (((uintptr_t)m.arr) % v == 0)));
    };
    // tuning hooks (SPC_MOMENTS_*): defaults chosen from MI355X measurements
    int vec = spc_switch("SPC_MOMENTS_VEC", 4);
    if (vec != 1 && vec != 2 && vec != 4) vec = 4;
    while (vec > 1 && !aligned(vec)) vec >>= 1;
    p.vec = vec;
    // MI355X sweeps at 1024^3 (tools/tune_moments.py; profiles/r01_tune_moments.log, r04_moments_issue.log)
    const bool arr_ = (m.flags & SPC_MASK_ARRAY) != 0;
    (void)arr_;
    p.mask_first = spc_switch("SPC_MOMENTS_MASK_FIRST", 1) != 0;   // 0: the loop that loads every sample (16-byte lanes with a mask array)
    p.u = spc_switch("SPC_MOMENTS_U", ext ? 2 : 8);
    if (p.u != 2 && p.u != 4 && p.u != 8) p.u = 4;
    const int64_t ngroups = c->ny * (c->nx / p.vec);
    const int64_t nblocks = (ngroups + kLanes - 1) / kLanes;
    // in-block z split: ZW waves share the columns when z is long enough
    // eight waves per block pay on planes up to 8 MiB (C2: 0.866 -> 0.827 ms), not on the north star's 16 MiB planes (13.06 -> 13.22 ms)
    p.zw = spc_switch("SPC_MOMENTS_ZW", c->nz >= 512 && !ext && c->ny * c->nx <= (1 << 21) ? 8 : (c->nz >= 16 ? 4 : 1));
    if (p.zw != 1 && p.zw != 4 && p.zw != 8) p.zw = 1;
    if (p.vec != 4) { p.u = 4; if (p.zw > 4) p.zw = 4; }
    // grid z split only when the map alone cannot fill the chip (256 CUs x ~8 blocks)
    int nsplit = 1;
    const int64_t target = 2048;
    if (nblocks < target && c->nz >= 256)
        nsplit = (int)std::min<int64_t>(std::min<int64_t>((target + nblocks - 1) / nblocks, c->nz / 64), 16);
    nsplit = std::max(1, spc_switch("SPC_MOMENTS_NSPLIT", nsplit));
    p.zchunk = (c->nz + nsplit - 1) / nsplit;
    p.nsplit = (int)((c->nz + p.zchunk - 1) / p.zchunk);
    return p;
}

// ---- the mask array as bits (layout: include/spcube_hip.h) ---------------------------------------------------
// Lane group g = y * (nx / 4) + x / 4 as in moments_kernel<4, ...>; block b = g / 64, lane l = g % 64; the 32 bytes of plane z
// of block b at (b * nz + z) * 32, lane l in nibble (l & 1) of byte l >> 1.  Nothing of a launch plan enters.
struct PackArgs {
    const uint8_t* arr;
    int64_t nz, row_stride, plane_stride;
    int64_t groups_per_row, ngroups;
    uint8_t* bits;
};

constexpr int kPackPlanes = 8;   // planes per wave and step: 8 x 32 = 256 contiguous bytes of bits, one dword per lane

// One wave = one block of 64 lane groups, eight planes per step.  A lane reads its mask dword of each plane and makes the
// nibble; the eight lanes that share a dword of the bits (lanes 8 j .. 8 j + 7 -> bytes 4 j .. 4 j + 3) OR their shifted nibbles
// together by three neighbour exchanges, after which each of them holds the dword of every plane; lane 8 j + p stores plane p's.
// A wave's store covers the 256 bytes of its eight planes.  Dead lanes (g >= ngroups) contribute zero bits; planes past nz
// are neither read nor stored.
__global__ __launch_bounds__(256) void mask_pack_bits_kernel(const PackArgs A) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t blk = blockIdx.x;
    const int64_t g = blk * kLanes + lane;
    const bool live = g < A.ngroups;
    const int64_t gg = live ? g : 0;
    const int64_t y = gg / A.groups_per_row;
    const int64_t x = (gg - y * A.groups_per_row) * 4;
    const uint8_t* pm = A.arr + y * A.row_stride + x;
    const int64_t nsteps = (A.nz + kPackPlanes - 1) / kPackPlanes;
    const int p_mine = lane & 7;
    for (int64_t s = (int64_t)blockIdx.y * 4 + w; s < nsteps; s += (int64_t)gridDim.y * 4) {
        const int64_t z0 = s * kPackPlanes;
        uint32_t m[kPackPlanes];
#pragma unroll
        for (int p = 0; p < kPackPlanes; ++p) {
            m[p] = 0;
            if (live && z0 + p < A.nz)                               // z0 + p < nz: wave-uniform
                m[p] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(pm + (z0 + p) * A.plane_stride));
        }
        uint32_t mine = 0;
#pragma unroll
        for (int p = 0; p < kPackPlanes; ++p) {
            uint32_t n = ((m[p] & 0xffu) != 0 ? 1u : 0u) | ((m[p] & 0xff00u) != 0 ? 2u : 0u) |
                         ((m[p] & 0xff0000u) != 0 ? 4u : 0u) | ((m[p] & 0xff000000u) != 0 ? 8u : 0u);
            n <<= 4 * (lane & 7);
            n |= __shfl_xor(n, 1);
            n |= __shfl_xor(n, 2);
            n |= __shfl_xor(n, 4);
            if (p == p_mine) mine = n;
        }
        if (z0 + p_mine < A.nz)
            *reinterpret_cast<uint32_t*>(A.bits + (blk * A.nz + z0 + p_mine) * 32 + (lane >> 3) * 4) = mine;
    }
}

size_t mask_bits_bytes(int64_t nz, int64_t ny, int64_t nx) {
    if (nz <= 0 || ny <= 0 || nx <= 0 || nx % 4 != 0) return 0;
    const int64_t ngroups = ny * (nx / 4);
    return (size_t)((ngroups + kLanes - 1) / kLanes) * (size_t)nz * 32;
}

// ---- the list of included lane segments (layout: include/spcube_hip.h) -----------------------------------------
// One wave per sublist s = b * nsub + j, j = split * zw + w: it marches the planes wave w of split `split` of block b marches
// in moments_kernel, reading the lane's nibble of the bits as the BITS form does.
struct ListArgs {
    const uint8_t* bits;
    int64_t nz, zchunk, nsub, total;   // total = nblocks * nsub
    int zw;
    uint32_t* len;                     // count: the longest lane's included planes ...
    uint32_t* lines;                   // ... and the non-zero 32-bit words of the sublist's bits rows
    const float* cube;                 // fill
    int64_t row_stride, plane_stride, groups_per_row, ngroups;
    const uint64_t* off;
    const uint32_t* flen;
    f32x4* samples;
    uint32_t* meta;
    uint64_t rows;
};

constexpr int kListWaves = 4;          // sublists per block of the count and fill kernels
constexpr int kListBatch = 8;          // planes in flight per lane

__global__ __launch_bounds__(kLanes * kListWaves) void list_count_kernel(const ListArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * kListWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (s >= A.total) return;                                        // wave-uniform
    const int64_t b = s / A.nsub;
    const int j = (int)(s - b * A.nsub);
    const int split = j / A.zw, w = j - split * A.zw;
    const int64_t zb = (int64_t)split * A.zchunk;
    const int64_t ze = min(A.nz, zb + A.zchunk);
    const uint8_t* q = A.bits + b * A.nz * 32 + (lane >> 1);
    const int sh = (lane & 1) * 4;
    uint32_t cnt = 0, lines = 0;
    auto take = [&](uint32_t byte) {
        const bool inc = ((byte >> sh) & 0xfu) != 0;
        cnt += inc ? 1u : 0u;
        // eight lanes share a 32-bit word of the bits and a 128-byte line of the cube: bit 0 of every byte of the ballot after the folds
        unsigned long long any = __ballot(inc);
        any |= any >> 1;
        any |= any >> 2;
        any |= any >> 4;
        lines += (uint32_t)__popcll(any & 0x0101010101010101ULL);
    };
    int64_t z = zb + w;
    for (; z + (int64_t)(kListBatch - 1) * A.zw < ze; z += (int64_t)kListBatch * A.zw) {
        uint32_t byte[kListBatch];
#pragma unroll
        for (int u = 0; u < kListBatch; ++u) byte[u] = q[(z + (int64_t)u * A.zw) * 32];
#pragma unroll
        for (int u = 0; u < kListBatch; ++u) take(byte[u]);
    }
    for (; z < ze; z += A.zw) take(q[z * 32]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt = max(cnt, (uint32_t)__shfl_xor((int)cnt, o));
    if (lane == 0) {
        A.len[s] = cnt;
        A.lines[s] = lines;
    }
}

__global__ __launch_bounds__(kLanes * kListWaves) void list_fill_kernel(const ListArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * kListWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (s >= A.total) return;                                        // wave-uniform
    const int64_t b = s / A.nsub;
    const int j = (int)(s - b * A.nsub);
    const int split = j / A.zw, w = j - split * A.zw;
    const int64_t zb = (int64_t)split * A.zchunk;
    const int64_t ze = min(A.nz, zb + A.zchunk);
    const int64_t g = b * kLanes + lane;
    const bool live = g < A.ngroups;                                 // dead lanes load nothing and hold only padding
    const int64_t gg = live ? g : 0;
    const int64_t y = gg / A.groups_per_row;
    const int64_t x = (gg - y * A.groups_per_row) * 4;
    const float* p = A.cube + y * A.row_stride + x;
    const uint8_t* q = A.bits + b * A.nz * 32 + (lane >> 1);
    const int sh = (lane & 1) * 4;
    // the rows of this sublist, cut to what the arrays hold whatever off and len say
    const uint64_t row0 = A.off[s];
    uint32_t n = A.flen[s];
    const uint64_t room = row0 < A.rows ? A.rows - row0 : 0;
    if (n > room) n = (uint32_t)room;
    f32x4* ps = A.samples + row0 * kLanes + lane;
    uint32_t* pq = A.meta + row0 * kLanes + lane;
    uint32_t k = 0;                                                  // the lane's own running index
    auto put = [&](const f32x4& v, uint32_t nib, int64_t z) {
        if (nib != 0 && k < n) {
            ps[(uint64_t)k * kLanes] = v;
            pq[(uint64_t)k * kLanes] = (uint32_t)z | (nib << 28);
            ++k;
        }
    };
    int64_t z = zb + w;
    for (; z + (int64_t)(kListBatch - 1) * A.zw < ze; z += (int64_t)kListBatch * A.zw) {
        uint32_t nib[kListBatch];
        f32x4 v[kListBatch];
#pragma unroll
        for (int u = 0; u < kListBatch; ++u) nib[u] = live ? (uint32_t)(q[(z + (int64_t)u * A.zw) * 32] >> sh) & 0xfu : 0u;
#pragma unroll
        for (int u = 0; u < kListBatch; ++u) {
            v[u] = f32x4{};
            if (nib[u] != 0) v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + (z + (int64_t)u * A.zw) * A.plane_stride));
        }
#pragma unroll
        for (int u = 0; u < kListBatch; ++u) put(v[u], nib[u], z + (int64_t)u * A.zw);
    }
    for (; z < ze; z += A.zw) {
        const uint32_t nib = live ? (uint32_t)(q[z * 32] >> sh) & 0xfu : 0u;
        f32x4 v{};
        if (nib != 0) v = *reinterpret_cast<const f32x4*>(p + z * A.plane_stride);
        put(v, nib, z);
    }
    // padding: samples 0, meta 0 - a plane the mask excludes
    for (; k < n; ++k) {
        ps[(uint64_t)k * kLanes] = f32x4{};
        pq[(uint64_t)k * kLanes] = 0u;
    }
}

// ---- the voxel list, made from a list (layout: include/spcube_hip.h, spc_moments_vlist_*) -------------------------
// One wave per sublist of the list, the list's rows read coalesced; neither kernel reads the cube or the bits.
struct VlistArgs {
    const uint32_t* meta;              // the list: [rows][64] z | nibble << 28 ...
    const f32x4* samples;              // ... and [rows][64] the lane's four samples (fill)
    const uint64_t* off;
    const uint32_t* len;
    uint64_t rows;
    int64_t total;                     // nblocks * nsub
    uint32_t* vlen_out;                // count: the longest lane's included voxels
    const uint64_t* voff;              // fill
    const uint32_t* vlen;
    u32x2* entries;
    uint64_t vrows;
};

constexpr int kVlistBatch = 8;         // list rows in flight per lane of the count kernel
constexpr int kVlistFillBatch = 4;     // ... and of the fill kernel (20 bytes a row)
constexpr int kVlistLongSublist = 128; // mean rows per sublist from which the sums and count forms keep 16 rows in flight (moments_run)

__global__ __launch_bounds__(kLanes * kListWaves) void vlist_count_kernel(const VlistArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * kListWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (s >= A.total) return;                                        // wave-uniform
    // the rows of this sublist, cut to what the list holds whatever off and len say
    const uint64_t row0 = A.off[s];
    uint32_t n = A.len[s];
    const uint64_t room = row0 < A.rows ? A.rows - row0 : 0;
    if (n > room) n = (uint32_t)room;
    const uint32_t* pq = A.meta + row0 * kLanes + lane;
    uint32_t cnt = 0, k = 0;
    for (; k + kVlistBatch <= n; k += kVlistBatch, pq += kVlistBatch * kLanes) {
        uint32_t mt[kVlistBatch];
#pragma unroll
        for (int u = 0; u < kVlistBatch; ++u) mt[u] = __builtin_nontemporal_load(pq + u * kLanes);
#pragma unroll
        for (int u = 0; u < kVlistBatch; ++u) cnt += (uint32_t)__popc(mt[u] >> 28);
    }
    for (; k < n; ++k, pq += kLanes) cnt += (uint32_t)__popc(*pq >> 28);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt = max(cnt, (uint32_t)__shfl_xor((int)cnt, o));
    if (lane == 0) A.vlen_out[s] = cnt;
}

__global__ __launch_bounds__(kLanes * kListWaves) void vlist_fill_kernel(const VlistArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * kListWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (s >= A.total) return;                                        // wave-uniform
    // the rows read and the rows written, each cut to what its arrays hold whatever the offsets and lengths say
    const uint64_t row0 = A.off[s];
    uint32_t n = A.len[s];
    const uint64_t room = row0 < A.rows ? A.rows - row0 : 0;
    if (n > room) n = (uint32_t)room;
    const uint64_t vrow0 = A.voff[s];
    uint32_t vn = A.vlen[s];
    const uint64_t vroom = vrow0 < A.vrows ? A.vrows - vrow0 : 0;
    if (vn > vroom) vn = (uint32_t)vroom;
    const uint32_t* pq = A.meta + row0 * kLanes + lane;
    const f32x4* ps = A.samples + row0 * kLanes + lane;
    u32x2* pe = A.entries + vrow0 * kLanes + lane;
    uint32_t kv = 0;                                                 // the lane's own running row
    auto put = [&](const f32x4& v, uint32_t mt) {
        const uint32_t z = mt & 0x0fffffffu;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (((mt >> (28 + i)) & 1u) != 0 && kv < vn) {
                u32x2 e;
                e.x = __float_as_uint(v[i]);
                e.y = z | ((uint32_t)i << 28) | (1u << 30);
                pe[(uint64_t)kv * kLanes] = e;
                ++kv;
            }
        }
    };
    uint32_t k = 0;
    for (; k + kVlistFillBatch <= n; k += kVlistFillBatch, pq += kVlistFillBatch * kLanes, ps += kVlistFillBatch * kLanes) {
        uint32_t mt[kVlistFillBatch];
        f32x4 v[kVlistFillBatch];
#pragma unroll
        for (int u = 0; u < kVlistFillBatch; ++u) mt[u] = __builtin_nontemporal_load(pq + u * kLanes);
#pragma unroll
        for (int u = 0; u < kVlistFillBatch; ++u) v[u] = __builtin_nontemporal_load(ps + u * kLanes);
#pragma unroll
        for (int u = 0; u < kVlistFillBatch; ++u) put(v[u], mt[u]);
    }
    for (; k < n; ++k, pq += kLanes, ps += kLanes) {
        const uint32_t mt = *pq;
        const f32x4 v = *ps;
        put(v, mt);
    }
    // padding: all zero, bit 30 clear - not an entry
    for (; kv < vn; ++kv) pe[(uint64_t)kv * kLanes] = u32x2{0u, 0u};
}

// the list a voxel list is counted and filled from: its desc a plan, its arrays holding the rows it names (with_samples: fill)
int vlist_source_check(const spc_moments_list* list, bool with_samples, int64_t* total) {
    SPC_REQUIRE(list != nullptr, "list is NULL");
    const spc_moments_list_desc& d = list->desc;
    SPC_REQUIRE((d.zw == 1 || d.zw == 4 || d.zw == 8) && d.nsplit >= 1 && d.zchunk >= 1 && d.nsub == (int64_t)d.nsplit * d.zw &&
                d.nblocks >= 1 && d.nblocks < (1LL << 31), "the list's desc is not a launch plan");
    *total = d.nblocks * d.nsub;
    SPC_REQUIRE((*total + kListWaves - 1) / kListWaves < (1LL << 31), "too many sublists");
    SPC_REQUIRE(list->d_off != nullptr && list->d_len != nullptr && list->nsublists >= (size_t)*total,
                "the list's d_off and d_len: %zu entries given, %lld sublists", list->nsublists, (long long)*total);
    SPC_REQUIRE(list->rows == 0 || (list->d_meta != nullptr && (!with_samples || list->d_samples != nullptr)),
                "the list's d_samples or d_meta is NULL");
    SPC_REQUIRE(list->meta_bytes / 256 >= list->rows && (!with_samples || list->samples_bytes / 1024 >= list->rows),
                "the list's d_samples / d_meta too small for %llu rows (1024 and 256 bytes each)", (unsigned long long)list->rows);
    SPC_REQUIRE(spc_aligned(list->d_meta, 4) && spc_aligned(list->d_off, 8) && spc_aligned(list->d_len, 4) &&
                (!with_samples || spc_aligned(list->d_samples, 16)),
                "the list's d_samples must be 16-byte, d_off 8-byte, d_meta and d_len 4-byte aligned");
    return SPC_OK;
}

bool same_desc(const spc_moments_list_desc& d, const spc_moments_list_desc& l) {
    return d.zw == l.zw && d.nsplit == l.nsplit && d.zchunk == l.zchunk && d.nblocks == l.nblocks && d.nsub == l.nsub;
}

constexpr int64_t kListMaxNz = 1LL << 28;      // z shares its meta word with the nibble

// what every moments entry works out before it launches: the checks, the kernel arguments, the plan after the workspace
// fallback and whether the launch reads the packed mask
int moments_setup(const spc_cube_f32* cube, const spc_mask* mask, const double* d_cen, bool need_cen, double dv, double m1_add,
                  const spc_moment_outputs* out, const void* d_workspace, size_t workspace_bytes,
                  const void* d_mask_bits, size_t bits_bytes, MomArgs& A, Plan& p) {
    int rc = spc_check_cube(cube);
    if (rc) return rc;
    SPC_REQUIRE(out != nullptr, "outputs struct is NULL");
    SPC_REQUIRE(!need_cen || d_cen != nullptr, "d_cen is NULL");
    SPC_REQUIRE(cube->nz < (1LL << 31), "nz too large");
    rc = spc_mask_to_dev(mask, cube, &A.mask);
    if (rc) return rc;
    A.cube = cube->d_data;
    A.nz = cube->nz; A.ny = cube->ny; A.nx = cube->nx;
    A.row_stride = cube->row_stride; A.plane_stride = cube->plane_stride;
    A.cen = d_cen; A.dv = dv; A.m1_add = m1_add;
    A.out = *out;
    A.out_row_stride = out->out_row_stride ? out->out_row_stride : cube->nx;
    const bool ext = out->d_argmax || out->d_argmin || out->d_vmax || out->d_vmin;
    p = make_plan(cube, A.mask, ext);
    spc_canonical_pred(A.mask.flags, A.mask.thr_lo, A.mask.thr_hi, &A.lim, &A.lo, &A.hi);
    A.xcd_group = spc_switch("SPC_MOMENTS_XCD", 0);    // measured: +- 1 % either way on the real kernel (profiles/r04_moments_issue.log)
    A.groups_per_row = cube->nx / p.vec;
    A.ngroups = cube->ny * A.groups_per_row;
    A.nsplit = p.nsplit;
    A.zchunk = p.zchunk;
    A.ws = (double*)d_workspace;
    if (p.nsplit > 1) {
        const size_t need = (size_t)p.nsplit * kWsFields * sizeof(double) * (size_t)(cube->ny * cube->nx);
        if (!d_workspace || workspace_bytes < need) {
            // not enough workspace: fall back to a single z range (still correct)
            A.nsplit = 1; A.zchunk = cube->nz; p.nsplit = 1; p.zchunk = cube->nz;
        }
    }
    const bool arr = (A.mask.flags & SPC_MASK_ARRAY) != 0;
    // the packed mask only where the launch is the mask-first march of 16-byte lanes; everything else reads the bytes as before
    p.bits = nullptr;
    if (d_mask_bits && arr && p.vec == 4 && p.mask_first && spc_switch("SPC_MOMENTS_MASK_BITS", 1) != 0) {
        const size_t need = mask_bits_bytes(cube->nz, cube->ny, cube->nx);
        if (need && bits_bytes >= need) p.bits = (const uint8_t*)d_mask_bits;
    }
    return SPC_OK;
}

// the plan of a launch as a list is made for it
spc_moments_list_desc list_desc(const MomArgs& A, const Plan& p) {
    spc_moments_list_desc d;
    d.zw = p.zw; d.nsplit = A.nsplit; d.zchunk = A.zchunk;
    d.nblocks = (A.ngroups + kLanes - 1) / kLanes;
    d.nsub = (int64_t)A.nsplit * p.zw;
    return d;
}

// there is a list for this launch: the march of 16-byte lanes over the packed mask (have_bits: the bits were given and are
// read; without them the same conditions on the plan alone), short enough for z to share a word with the nibble
int list_exists(const MomArgs& A, const Plan& p, bool have_bits, const char* who) {
    const bool arr = (A.mask.flags & SPC_MASK_ARRAY) != 0;
    if (!arr || p.vec != 4 || !p.mask_first || A.nz >= kListMaxNz || (have_bits && !p.bits) ||
        spc_switch("SPC_MOMENTS_MASK_BITS", 1) == 0 || spc_switch("SPC_MOMENTS_LIST", 1) == 0) {
        spc_set_error("%s: no list for this launch (it needs a mask array read as bits by the mask-first march of 16-byte lanes, "
                      "nz < 2^28 and SPC_MOMENTS_LIST not 0)", who);
        return SPC_ERR_UNSUPPORTED;
    }
    return SPC_OK;
}

int moments_run(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, const double* d_cen, double dv, double m1_add,
                const spc_moment_outputs* out, void* d_workspace, size_t workspace_bytes, const void* d_mask_bits, size_t bits_bytes,
                const spc_moments_list* list, const spc_moments_vlist* vlist) {
    MomArgs A{};
    Plan p;
    int rc = moments_setup(cube, mask, d_cen, true, dv, m1_add, out, d_workspace, workspace_bytes, d_mask_bits, bits_bytes, A, p);
    if (rc) return rc;
    SPC_DEVICE(device);
    const bool ext = out->d_argmax || out->d_argmin || out->d_vmax || out->d_vmin;
    const bool thr = (A.mask.flags & (SPC_MASK_GT | SPC_MASK_GE | SPC_MASK_LT | SPC_MASK_LE)) != 0;
    const bool arr = (A.mask.flags & SPC_MASK_ARRAY) != 0;
    // the list only where it was made for exactly this plan and its arrays hold the rows it names; otherwise the bits march
    if (list && p.bits && A.nz < kListMaxNz && spc_switch("SPC_MOMENTS_LIST", 1) != 0) {
        const spc_moments_list_desc d = list_desc(A, p);
        const spc_moments_list_desc& l = list->desc;
        const bool same = d.zw == l.zw && d.nsplit == l.nsplit && d.zchunk == l.zchunk && d.nblocks == l.nblocks && d.nsub == l.nsub;
        if (same && list->d_samples && list->d_meta && list->d_off && list->d_len && list->nsublists >= (size_t)(d.nblocks * d.nsub) &&
            list->samples_bytes / 1024 >= list->rows && list->meta_bytes / 256 >= list->rows &&
            spc_aligned(list->d_samples, 16) && spc_aligned(list->d_meta, 4) && spc_aligned(list->d_off, 8) && spc_aligned(list->d_len, 4)) {
            A.list_samples = (const f32x4*)list->d_samples;
            A.list_meta = (const uint32_t*)list->d_meta;
            A.list_off = list->d_off;
            A.list_len = list->d_len;
            A.list_rows = list->rows;
            // rows in flight per lane (profiles/moments_list_bench.txt)
            p.list_u = spc_switch("SPC_MOMENTS_LIST_U", ext ? 4 : 8) == 4 ? 4 : 8;
        }
    }
    // the voxel list under the same conditions, for exactly this plan; otherwise what the call was without it
    if (vlist && p.bits && A.nz < kListMaxNz && spc_switch("SPC_MOMENTS_LIST", 1) != 0 && spc_switch("SPC_MOMENTS_VLIST", 1) != 0) {
        const spc_moments_list_desc d = list_desc(A, p);
        if (same_desc(d, vlist->desc) && vlist->d_entries && vlist->d_off && vlist->d_len && vlist->nsublists >= (size_t)(d.nblocks * d.nsub) &&
            vlist->entries_bytes / 512 >= vlist->rows && spc_aligned(vlist->d_entries, 8) && spc_aligned(vlist->d_off, 8) &&
            spc_aligned(vlist->d_len, 4)) {
            A.list_samples = (const f32x4*)vlist->d_entries;     // (MomArgs: the voxel-list forms read the list's fields)
            A.list_meta = nullptr;
            A.list_off = vlist->d_off;
            A.list_len = vlist->d_len;
            A.list_rows = vlist->rows;
            // rows in flight per lane (profiles/moments_vlist_bench.txt): the U = 16 forms hold 142 - 148 VGPRs, three waves per SIMD
            // against five, and pay only where a sublist is many batches long - 180 rows on average at the north star (5 % faster
            // than U = 8), not at 38 or 70 rows (27 % and 20 % slower); with extrema U = 8 wins at every shape measured
            const uint64_t nsublists = (uint64_t)(d.nblocks * d.nsub);
            const bool long_sublists = vlist->rows / nsublists >= (uint64_t)kVlistLongSublist;
            p.vlist_u = spc_switch("SPC_MOMENTS_VLIST_U", !ext && long_sublists ? 16 : 8) == 16 ? 16 : 8;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const int what = ext ? kExtrema : (out->d_nvalid ? kCount : kSums);
    if (arr) rc = what == kExtrema ? launch_plan<true, kExtrema>(A, st, p, thr)
                : what == kCount ? launch_plan<true, kCount>(A, st, p, thr) : launch_plan<true, kSums>(A, st, p, thr);
    else rc = what == kExtrema ? launch_plan<false, kExtrema>(A, st, p, thr)
            : what == kCount ? launch_plan<false, kCount>(A, st, p, thr) : launch_plan<false, kSums>(A, st, p, thr);
    if (rc) return rc;
    if (A.nsplit > 1) {
        const int64_t ncols = cube->ny * cube->nx;
        dim3 grid((unsigned)((ncols + 255) / 256));
        if (ext) hipLaunchKernelGGL(moments_combine_kernel<kExtrema>, grid, dim3(256), 0, st, A, p.vec);
        else hipLaunchKernelGGL(moments_combine_kernel<kCount>, grid, dim3(256), 0, st, A, p.vec);
        SPC_LAUNCH_CHECK();
    }
    return SPC_OK;
}

}  // namespace

extern "C" {

size_t spc_mask_bits_bytes(int64_t nz, int64_t ny, int64_t nx) { return mask_bits_bytes(nz, ny, nx); }

int spc_mask_pack_bits(int device, void* stream, int64_t nz, int64_t ny, int64_t nx, const spc_mask* mask,
                       void* d_bits, size_t bits_bytes) {
    SPC_REQUIRE(nz > 0 && ny > 0 && nx > 0, "mask shape must be positive (got %lld,%lld,%lld)", (long long)nz, (long long)ny, (long long)nx);
    SPC_REQUIRE(mask != nullptr && (mask->flags & SPC_MASK_ARRAY) && mask->d_array != nullptr, "no mask array to pack");
    SPC_REQUIRE(d_bits != nullptr, "d_bits is NULL");
    const size_t need = mask_bits_bytes(nz, ny, nx);
    const int64_t rs = mask->row_stride ? mask->row_stride : nx, ps = mask->plane_stride ? mask->plane_stride : ny * nx;
    SPC_REQUIRE(rs >= nx && ps >= rs * (ny - 1) + nx, "mask strides smaller than the shape");
    // the lanes read dwords: the conditions of make_plan's aligned(4) for the mask
    if (need == 0 || rs % 4 != 0 || ps % 4 != 0 || !spc_aligned(mask->d_array, 4) || !spc_aligned(d_bits, 4)) {
        spc_set_error("spc_mask_pack_bits: nx, the mask's strides and its address must be multiples of 4");
        return SPC_ERR_UNSUPPORTED;
    }
    SPC_REQUIRE(bits_bytes >= need, "d_bits too small: %zu bytes given, %zu needed (spc_mask_bits_bytes)", bits_bytes, need);
    SPC_DEVICE(device);
    PackArgs A{};
    A.arr = mask->d_array; A.nz = nz; A.row_stride = rs; A.plane_stride = ps;
    A.groups_per_row = nx / 4; A.ngroups = ny * A.groups_per_row;
    A.bits = (uint8_t*)d_bits;
    const int64_t nblocks = (A.ngroups + kLanes - 1) / kLanes;
    SPC_REQUIRE(nblocks < (1LL << 31), "mask too large");
    // enough blocks to fill the chip when the map alone is small; four waves of a block take interleaved steps
    const int64_t nsteps = (nz + kPackPlanes - 1) / kPackPlanes;
    const int64_t gy = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>((nsteps + 3) / 4, (4096 + nblocks - 1) / nblocks), 65535));
    hipLaunchKernelGGL(mask_pack_bits_kernel, dim3((unsigned)nblocks, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, A);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

size_t spc_moments_workspace_bytes(int64_t nz, int64_t ny, int64_t nx) {
    if (nz <= 0 || ny <= 0 || nx <= 0) return 0;
    // upper bound on nsplit used by make_plan
    int64_t nsplit_max = std::max<int64_t>(1, std::min<int64_t>(nz / 64, 16));
    // (the two switches that move make_plan's split; -1: not set)
    const int env = spc_switch("SPC_MOMENTS_NSPLIT", -1);
    if (env != -1) nsplit_max = std::max<int64_t>(nsplit_max, env);
    const int64_t nblocks = (ny * nx / 4 + kLanes - 1) / kLanes;
    if (env == -1 && spc_switch("SPC_MOMENTS_VEC", -1) == -1 && (nblocks >= 2048 || nz < 256)) return 0;
    return (size_t)nsplit_max * kWsFields * sizeof(double) * (size_t)(ny * nx);
}

int spc_moments_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                    const double* d_cen, double dv, double m1_add, const spc_moment_outputs* out,
                    void* d_workspace, size_t workspace_bytes) {
    return spc_moments_bits_f32(device, stream, cube, mask, d_cen, dv, m1_add, out, d_workspace, workspace_bytes, nullptr, 0);
}

int spc_moments_bits_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                         const double* d_cen, double dv, double m1_add, const spc_moment_outputs* out,
                         void* d_workspace, size_t workspace_bytes, const void* d_mask_bits, size_t bits_bytes) {
    return moments_run(device, stream, cube, mask, d_cen, dv, m1_add, out, d_workspace, workspace_bytes, d_mask_bits, bits_bytes, nullptr, nullptr);
}

int spc_moments_list_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                         const double* d_cen, double dv, double m1_add, const spc_moment_outputs* out,
                         void* d_workspace, size_t workspace_bytes, const void* d_mask_bits, size_t bits_bytes,
                         const spc_moments_list* list) {
    return moments_run(device, stream, cube, mask, d_cen, dv, m1_add, out, d_workspace, workspace_bytes, d_mask_bits, bits_bytes, list, nullptr);
}

int spc_moments_list_plan_f32(const spc_cube_f32* cube, const spc_mask* mask, const spc_moment_outputs* out,
                              const void* d_workspace, size_t workspace_bytes, spc_moments_list_desc* desc) {
    SPC_REQUIRE(desc != nullptr, "desc is NULL");
    MomArgs A{};
    Plan p;
    int rc = moments_setup(cube, mask, nullptr, false, 0.0, 0.0, out, d_workspace, workspace_bytes, nullptr, 0, A, p);
    if (rc) return rc;
    rc = list_exists(A, p, false, "spc_moments_list_plan_f32");
    if (rc) return rc;
    *desc = list_desc(A, p);
    return SPC_OK;
}

int spc_moments_list_count_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                               const spc_moment_outputs* out, const void* d_workspace, size_t workspace_bytes,
                               const void* d_mask_bits, size_t bits_bytes, uint32_t* d_len, uint32_t* d_lines,
                               size_t nsublists, spc_moments_list_desc* desc) {
    SPC_REQUIRE(desc != nullptr, "desc is NULL");
    SPC_REQUIRE(d_mask_bits != nullptr, "d_mask_bits is NULL");
    SPC_REQUIRE(d_len != nullptr && d_lines != nullptr, "d_len or d_lines is NULL");
    MomArgs A{};
    Plan p;
    int rc = moments_setup(cube, mask, nullptr, false, 0.0, 0.0, out, d_workspace, workspace_bytes, d_mask_bits, bits_bytes, A, p);
    if (rc) return rc;
    rc = list_exists(A, p, true, "spc_moments_list_count_f32");
    if (rc) return rc;
    const spc_moments_list_desc d = list_desc(A, p);
    const int64_t total = d.nblocks * d.nsub;
    SPC_REQUIRE(nsublists >= (size_t)total, "d_len and d_lines too small: %zu entries given, %lld sublists", nsublists, (long long)total);
    SPC_REQUIRE(spc_aligned(d_len, 4) && spc_aligned(d_lines, 4), "d_len and d_lines must be 4-byte aligned");
    SPC_REQUIRE((total + kListWaves - 1) / kListWaves < (1LL << 31), "too many sublists");
    *desc = d;
    SPC_DEVICE(device);
    ListArgs L{};
    L.bits = p.bits; L.nz = A.nz; L.zchunk = d.zchunk; L.nsub = d.nsub; L.total = total; L.zw = d.zw;
    L.len = d_len; L.lines = d_lines;
    hipLaunchKernelGGL(list_count_kernel, dim3((unsigned)((total + kListWaves - 1) / kListWaves)), dim3(kLanes * kListWaves), 0,
                       (hipStream_t)stream, L);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

int spc_moments_list_fill_f32(int device, void* stream, const spc_cube_f32* cube, const void* d_mask_bits, size_t bits_bytes,
                              const spc_moments_list* list) {
    int rc = spc_check_cube(cube);
    if (rc) return rc;
    SPC_REQUIRE(list != nullptr, "list is NULL");
    SPC_REQUIRE(d_mask_bits != nullptr, "d_mask_bits is NULL");
    SPC_REQUIRE(cube->nz < kListMaxNz, "nz too large for a list (%lld)", (long long)cube->nz);
    // 16-byte lanes: make_plan's aligned(4) for the cube
    if (cube->nx % 4 != 0 || cube->row_stride % 4 != 0 || cube->plane_stride % 4 != 0 || !spc_aligned(cube->d_data, 16)) {
        spc_set_error("spc_moments_list_fill_f32: nx, the cube's strides and its address must be multiples of 4 elements");
        return SPC_ERR_UNSUPPORTED;
    }
    const size_t need = mask_bits_bytes(cube->nz, cube->ny, cube->nx);
    SPC_REQUIRE(need && bits_bytes >= need, "d_mask_bits too small: %zu bytes given, %zu needed (spc_mask_bits_bytes)", bits_bytes, need);
    const spc_moments_list_desc& d = list->desc;
    const int64_t ngroups = cube->ny * (cube->nx / 4);
    SPC_REQUIRE((d.zw == 1 || d.zw == 4 || d.zw == 8) && d.nsplit >= 1 && d.zchunk >= 1 && d.nsub == (int64_t)d.nsplit * d.zw &&
                d.nblocks == (ngroups + kLanes - 1) / kLanes, "desc is not a launch plan of this cube");
    // the splits cover [0, nz) and none of them is empty
    SPC_REQUIRE(d.zchunk <= cube->nz && (int64_t)(d.nsplit - 1) * d.zchunk < cube->nz && (int64_t)d.nsplit * d.zchunk >= cube->nz,
                "desc: %d splits of %lld planes do not cover %lld planes", d.nsplit, (long long)d.zchunk, (long long)cube->nz);
    const int64_t total = d.nblocks * d.nsub;
    SPC_REQUIRE(list->d_off != nullptr && list->d_len != nullptr && list->nsublists >= (size_t)total,
                "d_off and d_len: %zu entries given, %lld sublists", list->nsublists, (long long)total);
    SPC_REQUIRE(list->rows == 0 || (list->d_samples != nullptr && list->d_meta != nullptr), "d_samples or d_meta is NULL");
    SPC_REQUIRE(list->samples_bytes / 1024 >= list->rows && list->meta_bytes / 256 >= list->rows,
                "d_samples / d_meta too small for %llu rows (1024 and 256 bytes each)", (unsigned long long)list->rows);
    SPC_REQUIRE(spc_aligned(list->d_samples, 16) && spc_aligned(list->d_meta, 4) && spc_aligned(list->d_off, 8) && spc_aligned(list->d_len, 4),
                "d_samples must be 16-byte, d_off 8-byte, d_meta and d_len 4-byte aligned");
    SPC_REQUIRE((total + kListWaves - 1) / kListWaves < (1LL << 31), "too many sublists");
    SPC_DEVICE(device);
    ListArgs L{};
    L.bits = (const uint8_t*)d_mask_bits; L.nz = cube->nz; L.zchunk = d.zchunk; L.nsub = d.nsub; L.total = total; L.zw = d.zw;
    L.cube = cube->d_data; L.row_stride = cube->row_stride; L.plane_stride = cube->plane_stride;
    L.groups_per_row = cube->nx / 4; L.ngroups = ngroups;
    L.off = list->d_off; L.flen = list->d_len;
    L.samples = (f32x4*)list->d_samples; L.meta = (uint32_t*)list->d_meta; L.rows = list->rows;
    hipLaunchKernelGGL(list_fill_kernel, dim3((unsigned)((total + kListWaves - 1) / kListWaves)), dim3(kLanes * kListWaves), 0,
                       (hipStream_t)stream, L);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

int spc_moments_vlist_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                          const double* d_cen, double dv, double m1_add, const spc_moment_outputs* out,
                          void* d_workspace, size_t workspace_bytes, const void* d_mask_bits, size_t bits_bytes,
                          const spc_moments_list* list, const spc_moments_vlist* vlist) {
    return moments_run(device, stream, cube, mask, d_cen, dv, m1_add, out, d_workspace, workspace_bytes, d_mask_bits, bits_bytes, list, vlist);
}

int spc_moments_vlist_count_f32(int device, void* stream, const spc_moments_list* list, uint32_t* d_vlen, size_t nsublists) {
    int64_t total = 0;
    int rc = vlist_source_check(list, false, &total);
    if (rc) return rc;
    SPC_REQUIRE(d_vlen != nullptr, "d_vlen is NULL");
    SPC_REQUIRE(nsublists >= (size_t)total, "d_vlen too small: %zu entries given, %lld sublists", nsublists, (long long)total);
    SPC_REQUIRE(spc_aligned(d_vlen, 4), "d_vlen must be 4-byte aligned");
    SPC_DEVICE(device);
    VlistArgs V{};
    V.meta = (const uint32_t*)list->d_meta; V.off = list->d_off; V.len = list->d_len; V.rows = list->rows; V.total = total;
    V.vlen_out = d_vlen;
    hipLaunchKernelGGL(vlist_count_kernel, dim3((unsigned)((total + kListWaves - 1) / kListWaves)), dim3(kLanes * kListWaves), 0,
                       (hipStream_t)stream, V);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

int spc_moments_vlist_fill_f32(int device, void* stream, const spc_moments_list* list, const spc_moments_vlist* vlist) {
    int64_t total = 0;
    int rc = vlist_source_check(list, true, &total);
    if (rc) return rc;
    SPC_REQUIRE(vlist != nullptr, "vlist is NULL");
    SPC_REQUIRE(same_desc(list->desc, vlist->desc), "the voxel list's desc is not the list's");
    SPC_REQUIRE(vlist->d_off != nullptr && vlist->d_len != nullptr && vlist->nsublists >= (size_t)total,
                "d_off and d_len: %zu entries given, %lld sublists", vlist->nsublists, (long long)total);
    SPC_REQUIRE(vlist->rows == 0 || vlist->d_entries != nullptr, "d_entries is NULL");
    SPC_REQUIRE(vlist->entries_bytes / 512 >= vlist->rows, "d_entries too small for %llu rows (512 bytes each)",
                (unsigned long long)vlist->rows);
    SPC_REQUIRE(spc_aligned(vlist->d_entries, 8) && spc_aligned(vlist->d_off, 8) && spc_aligned(vlist->d_len, 4),
                "d_entries and d_off must be 8-byte, d_len 4-byte aligned");
    SPC_DEVICE(device);
    VlistArgs V{};
    V.meta = (const uint32_t*)list->d_meta; V.samples = (const f32x4*)list->d_samples;
    V.off = list->d_off; V.len = list->d_len; V.rows = list->rows; V.total = total;
    V.voff = vlist->d_off; V.vlen = vlist->d_len; V.entries = (u32x2*)vlist->d_entries; V.vrows = vlist->rows;
    hipLaunchKernelGGL(vlist_fill_kernel, dim3((unsigned)((total + kListWaves - 1) / kListWaves)), dim3(kLanes * kListWaves), 0,
                       (hipStream_t)stream, V);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

int spc_moment_order_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                         const double* d_cen, int order, const double* d_mu, const double* d_s0,
                         double* d_out, int64_t out_row_stride) {
    int rc = spc_check_cube(cube);
    if (rc) return rc;
    SPC_REQUIRE(order >= 1 && order <= 64, "order must be in [1,64], got %d", order);
    SPC_REQUIRE(d_cen && d_mu && d_s0 && d_out, "NULL pointer argument");
    OrdArgs A{};
    rc = spc_mask_to_dev(mask, cube, &A.mask);
    if (rc) return rc;
    SPC_DEVICE(device);
    A.cube = cube->d_data;
    A.nz = cube->nz; A.ny = cube->ny; A.nx = cube->nx;
    A.row_stride = cube->row_stride; A.plane_stride = cube->plane_stride;
    A.cen = d_cen; A.mu = d_mu; A.s0 = d_s0; A.out = d_out; A.order = order;
    A.out_row_stride = out_row_stride ? out_row_stride : cube->nx;
    const int64_t ncols = cube->ny * cube->nx;
    const bool arr_ = (A.mask.flags & SPC_MASK_ARRAY) != 0;
    const bool v4 = (cube->nx % 4 == 0) && (cube->row_stride % 4 == 0) && (cube->plane_stride % 4 == 0) &&
                    ((((uintptr_t)cube->d_data) & 15) == 0) &&
                    (!arr_ || ((A.mask.row_stride % 4 == 0) && (A.mask.plane_stride % 4 == 0) && ((((uintptr_t)A.mask.arr) & 3) == 0)));
    if (v4) {
        const int64_t ng = cube->ny * (cube->nx / 4);
        if (arr_) hipLaunchKernelGGL(moment_order_v4_kernel<true>, dim3((unsigned)((ng + 63) / 64)), dim3(256), 0, (hipStream_t)stream, A);
        else hipLaunchKernelGGL(moment_order_v4_kernel<false>, dim3((unsigned)((ng + 63) / 64)), dim3(256), 0, (hipStream_t)stream, A);
    } else
        hipLaunchKernelGGL(moment_order_kernel, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, A);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

}  // extern "C"
