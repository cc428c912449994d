// spc_select_global.hip - order statistics of a whole float32 cube (median / percentile / mad_std with axis=None):
// spc_percentile_global_f32, and one pass of it as an entry of its own for cubes sharded over ranks
// (spc_key_histogram_f32, spc_key_to_f32).  The keys are spc_select_impl.h's order-preserving integers.
//
// The cube is one long ray here, so the digits of the key are found with shared histograms: one
// streaming pass per key BYTE (4 passes) counts, among the samples whose key matches the prefix
// found so far, the next byte; the host walks the 256 counters.  Histograms are built in LDS -
// 16 interleaved copies ([bin][lane & 15]: same-bin updates of different copies fall on different
// banks; real data put most samples in a handful of top-byte bins) - and flushed with one 64-bit
// atomic per bin and block.  A fifth pass (minimum key above the selected one) is only needed
// when the two order statistics of an interpolated percentile are different values.
#include "spc_select_impl.h"

namespace {

struct GSelArgs {
    const float* cube;
    int64_t nz, ny, nx, row_stride, plane_stride;
    MaskDev mask;
    int64_t nrows, rowlen, row_a, row_b;   // as in the statistics kernel: 1 row when contiguous
    uint32_t prefix, pmask;
    int shift;
    int has_center;
    float center;
    unsigned long long* hist;              // [256]
    uint32_t* next;                        // MODE 1: minimum key > prefix
};

template <bool ARR, int MODE>
__global__ __launch_bounds__(256) void gselect_kernel(const GSelArgs A) {
    __shared__ uint32_t lh[256 * 16];
    __shared__ uint32_t s_min;
    const int t = threadIdx.x;
    if (MODE == 0) {
        for (int i = t; i < 256 * 16; i += 256) lh[i] = 0;
    } else if (t == 0) {
        s_min = 0xffffffffu;
    }
    __syncthreads();
    const int copy = t & 15;
    uint32_t mymin = 0xffffffffu;
    auto take = [&](float v, unsigned mk) {
        const bool ok = spc_pred_valid(A.mask, v) & (mk != 0);
        if (!ok) return;
        if (A.has_center) v = __builtin_fabsf(v - A.center);
        const uint32_t k = fkey(v);
        if (MODE == 0) {
            if ((k & A.pmask) == A.prefix) atomicAdd(&lh[((k >> A.shift) & 0xffu) * 16 + copy], 1u);
        } else {
            if (k > A.prefix) mymin = min(mymin, k);
        }
    };
    // (one contiguous run: every block strides through it; rows of a strided view: the blocks share the rows out)
    const bool rows = A.nrows > 1;
    const int64_t stride = rows ? 256 : (int64_t)gridDim.x * 256, first = rows ? 0 : (int64_t)blockIdx.x * 256;
    for (int64_t r = rows ? blockIdx.x : 0; r < A.nrows; r += rows ? gridDim.x : 1) {
        const int64_t off = !rows ? 0 : (r / A.ny) * A.row_a + (r % A.ny) * A.row_b;
        const int64_t moff = !rows ? 0 : (r / A.ny) * A.mask.plane_stride + (r % A.ny) * A.mask.row_stride;
        const float* p = A.cube + off;
        const uint8_t* pm = ARR ? A.mask.arr + moff : nullptr;
        const bool al = ((((uintptr_t)p) & 15) == 0) && (!ARR || ((((uintptr_t)pm) & 3) == 0));
        const int64_t n4 = al ? A.rowlen / 4 : 0;
        for (int64_t i = first + t; i < n4; i += stride) {
            const f32x4s v = __builtin_nontemporal_load(reinterpret_cast<const f32x4s*>(p) + i);
            const uint32_t m = ARR ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(pm) + i) : 0x01010101u;
#pragma unroll
            for (int c = 0; c < 4; ++c) take(v[c], (m >> (8 * c)) & 0xffu);
        }
        for (int64_t j = n4 * 4 + first + t; j < A.rowlen; j += stride) take(p[j], ARR ? pm[j] : 1u);
    }
    if (MODE == 0) {
        __syncthreads();
        unsigned long long tot = 0;
#pragma unroll
        for (int c = 0; c < 16; ++c) tot += lh[t * 16 + c];
        if (tot) atomicAdd(&A.hist[t], tot);
    } else {
        atomicMin(&s_min, mymin);
        __syncthreads();
        if (t == 0 && s_min != 0xffffffffu) atomicMin(A.next, s_min);
    }
}

// How the blocks walk the cube (one contiguous run - the cube and, where there is one, its mask array - or the nz * ny rows of
// a view), how many of them, and the 256 counters + (as uint32) the "next key" cell from the caller's workspace
static int gsel_geometry(GSelArgs* A, int* nblocks, void* d_workspace, size_t workspace_bytes) {
    const bool arr = (A->mask.flags & SPC_MASK_ARRAY) != 0;
    const bool contig = (A->row_stride == A->nx) && (A->plane_stride == A->ny * A->nx) &&
                        (!arr || (A->mask.row_stride == A->nx && A->mask.plane_stride == A->ny * A->nx));
    if (contig) { A->nrows = 1; A->rowlen = A->nz * A->ny * A->nx; A->row_a = 0; A->row_b = 0; }
    else { A->nrows = A->nz * A->ny; A->rowlen = A->nx; A->row_a = A->plane_stride; A->row_b = A->row_stride; }
    const int64_t per_block = 256 * 4 * 8;
    *nblocks = (int)std::max<int64_t>(1, std::min<int64_t>(2048, contig ? (A->rowlen + per_block - 1) / per_block : (A->nrows + 3) / 4));
    SpcWorkspace ws(d_workspace, workspace_bytes);
    SPC_WS_TAKE(d_hist, ws, unsigned long long, 257);
    A->hist = d_hist;
    A->next = reinterpret_cast<uint32_t*>(d_hist + 256);
    return SPC_OK;
}

// one pass over the cube: the histogram of the next key byte (A.hist, zeroed here), or the smallest key above the prefix (A.next)
static hipError_t gsel_pass(const GSelArgs& A, bool next_key, int nblocks, hipStream_t st) {
    const hipError_t e = next_key ? hipMemsetAsync(A.next, 0xff, sizeof(uint32_t), st)
                                  : hipMemsetAsync(A.hist, 0, sizeof(unsigned long long) * 256, st);
    if (e != hipSuccess) return e;
    sel_with_bool((A.mask.flags & SPC_MASK_ARRAY) != 0, [&](auto arr_c) {
        sel_with_bool(next_key, [&](auto next_c) {
            hipLaunchKernelGGL((gselect_kernel<decltype(arr_c)::value, decltype(next_c)::value ? 1 : 0>), dim3(nblocks), dim3(256), 0, st, A);
        });
    });
    return hipGetLastError();
}

}  // namespace

extern "C" int spc_percentile_global_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                                         double q, int has_center, float center, double* h_out,
                                         void* d_workspace, size_t workspace_bytes) {
    int rc = spc_check_cube(cube);
    if (rc) return rc;
    SPC_REQUIRE(h_out != nullptr, "h_out is NULL");
    SPC_REQUIRE(q >= 0.0 && q <= 100.0, "Percentiles must be in the range [0, 100]");
    GSelArgs A{};
    rc = sel_set_cube<false>(&A, cube, mask);
    if (rc) return rc;
    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    A.has_center = has_center; A.center = center;
    int nblocks = 0;
    rc = gsel_geometry(&A, &nblocks, d_workspace, workspace_bytes);
    if (rc) return rc;
    unsigned long long h[256];
    hipError_t e = hipSuccess;
    unsigned long long n = 0, below = 0, eq = 0;
    long long klo = 0, khi = 0, k = 0;
    double frac = 0.0;
    for (int pass = 0; pass < 4 && e == hipSuccess; ++pass) {
        A.shift = 24 - 8 * pass;
        e = gsel_pass(A, false, nblocks, st);
        if (e == hipSuccess) e = hipMemcpyAsync(h, A.hist, sizeof(h), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) break;
        if (pass == 0) {
            for (int d = 0; d < 256; ++d) n += h[d];
            if (n == 0) break;
            const double pos = q / 100.0 * (double)(n - 1);
            klo = (long long)floor(pos);
            khi = std::min<long long>((long long)ceil(pos), (long long)n - 1);
            frac = pos - floor(pos);
            k = klo;
        }
        int d = 0;
        while (d < 255 && (unsigned long long)k >= h[d]) { k -= (long long)h[d]; below += h[d]; ++d; }
        eq = h[d];
        A.prefix |= (uint32_t)d << A.shift;
        A.pmask |= 0xffu << A.shift;
    }
    uint32_t key_lo = A.prefix, key_hi = A.prefix;
    if (e == hipSuccess && n > 0 && (unsigned long long)khi >= below + eq) {     // the upper statistic is the next larger value
        e = gsel_pass(A, true, nblocks, st);
        if (e == hipSuccess) e = hipMemcpyAsync(&key_hi, A.next, sizeof(key_hi), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    SPC_HIP(e);
    if (n == 0) { *h_out = NAN; return SPC_OK; }
    const double a = (double)spc_key_to_f32(key_lo), b = (double)spc_key_to_f32(key_hi);
    *h_out = (q == 50.0 && a == b) ? a : ((frac == 0.5) ? 0.5 * (a + b) : a + (b - a) * frac);
    return SPC_OK;
}

// One pass of the whole-cube selection as its own entry point, for cubes that are sharded over ranks: the ranks sum
// their 256 counters (or take the minimum of their next keys) before the walk, see distributed.sharded_percentile.
//   h_hist != NULL: h_hist[d] = number of included samples whose key agrees with `prefix` on the bits of `pmask` and
//                   has byte value d at bit `shift` (24, 16, 8, 0);
//   h_next != NULL: *h_next = the smallest key above `prefix` (0xffffffff when there is none).
// Keys are the order-preserving integers of the samples (of |x - center| with has_center); spc_key_to_f32 maps back.
extern "C" int spc_key_histogram_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                                     uint32_t prefix, uint32_t pmask, int shift, int has_center, float center,
                                     uint64_t* h_hist, uint32_t* h_next, void* d_workspace, size_t workspace_bytes) {
    int rc = spc_check_cube(cube);
    if (rc) return rc;
    SPC_REQUIRE((h_hist != nullptr) != (h_next != nullptr), "exactly one of h_hist / h_next must be given");
    SPC_REQUIRE(h_next || shift == 24 || shift == 16 || shift == 8 || shift == 0, "shift must be 24, 16, 8 or 0");
    GSelArgs A{};
    rc = sel_set_cube<false>(&A, cube, mask);
    if (rc) return rc;
    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    A.has_center = has_center; A.center = center;
    A.prefix = prefix; A.pmask = pmask; A.shift = shift;
    int nblocks = 0;
    rc = gsel_geometry(&A, &nblocks, d_workspace, workspace_bytes);
    if (rc) return rc;
    hipError_t e = gsel_pass(A, h_hist == nullptr, nblocks, st);
    if (e == hipSuccess) {
        e = h_hist ? hipMemcpyAsync(h_hist, A.hist, sizeof(unsigned long long) * 256, hipMemcpyDeviceToHost, st)
                   : hipMemcpyAsync(h_next, A.next, sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    SPC_HIP(e);
    return SPC_OK;
}

extern "C" float spc_key_to_f32(uint32_t key) {
    const uint32_t u = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

size_t spc_ws_percentile_global(void) { return spc_ws_round(sizeof(unsigned long long) * 257) + 256; }
