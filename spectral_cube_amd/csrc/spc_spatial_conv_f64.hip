// spc_spatial_conv_f64.hip - spatial_smooth of a float64 cube (gfx950): spc_spatial_conv_f64.
//
// The reference's spatial_smooth (dask_spectral_cube.py:962-993: astropy's convolve per channel) on the float64 samples
// as they are - the arithmetic of the float32 stencil (spc_spatial_conv.hip) without the final rounding to float32.  An
// outer-product kernel takes, in this order: one ring kernel with nothing between the passes (symmetric factors of up to
// 33 taps, none negative, centre taps positive; SPC_SPATIAL64_RING=0 turns it off, read per call), else two passes over
// a slab of the caller's workspace (LDS tiles with four outputs per thread; halos too wide for them take the x tile with
// one output per thread or the untiled passes), which also redo the call, gated by a flag word, when the ring meets an
// infinite valid sample under a padding tap.  The ring and the passes add an output's
// taps in the same order: the same float64 values.  Any other kernel is summed directly.
#include "spc_wide.h"

#include <algorithm>
#include <type_traits>
#include <utility>

namespace {

template <class F, int... G>
__device__ __forceinline__ void for_each_const(F&& f, std::integer_sequence<int, G...>) { (f(std::integral_constant<int, G>{}), ...); }

// Per channel, the convolution of spc_spectral_conv_f64.hip (astropy's convolve: zeros outside the image, invalid samples
// left out of both sums, one division) in 2-D.  An outer-product kernel runs as two passes over a slab of planes: the x pass
// leaves (sum kx d [valid], sum kx [valid]) per voxel in the caller's workspace, the y pass combines them and divides;
// any other kernel is summed directly (nky x nkx taps per output, neighbours from the caches).
struct Sp64Args {
    Cube64 c;
    MaskDev64 m;
    double* out;
    int64_t out_row_stride, out_plane_stride;
    const double* ky; const double* kx;     // separable: the two factors; direct: ky = the 2-D table, kx unused
    int nky, nkx;
    double* tmp;                            // (planes, ny, nx, 2) of the slab
    int64_t z0;                             // first plane of the slab
    const unsigned* gate;                   // != nullptr: run only when the word is set (the ring kernel met an infinite valid sample)
    int64_t y0;                             // first row of the launch: row y = y0 + blockIdx.y (slabs of at most 65535 rows)
};
__global__ __launch_bounds__(256) void spatial64_xpass_kernel(const Sp64Args A) {
    if (A.gate && *A.gate == 0u) return;
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t y = A.y0 + blockIdx.y, zl = blockIdx.z, z = A.z0 + zl;
    if (x >= A.c.nx) return;
    const int H = A.nkx / 2;
    double num = 0.0, den = 0.0;
    const bool arr = (A.m.flags & SPC_MASK_ARRAY) != 0;
    const double* pd = A.c.p + z * A.c.plane_stride + y * A.c.row_stride;
    const uint8_t* pmk = arr ? A.m.arr + z * A.m.plane_stride + y * A.m.row_stride : nullptr;
    constexpr int kIn = 8;                                       // loads requested together (clamped into the row)
    for (int j0 = 0; j0 < A.nkx; j0 += kIn) {                    // astropy's order along the fast axis
        double vv[kIn];
        unsigned mk[kIn];
#pragma unroll
        for (int q = 0; q < kIn; ++q) {
            const int64_t ic = min(max(x - H + j0 + q, (int64_t)0), A.c.nx - 1);
            vv[q] = pd[ic];
            mk[q] = arr ? pmk[ic] : 1u;
        }
#pragma unroll
        for (int q = 0; q < kIn; ++q) {
            const int j = j0 + q;
            if (j < A.nkx) {                                     // (uniform)
                const double kw = A.kx[A.nkx - 1 - j];           // flipped kernel, input x - H + j
                const int64_t i = x - H + j;
                const bool inr = i >= 0 && i < A.c.nx;
                const bool ok = spc_pred_valid(A.m, vv[q]) && mk[q] != 0u;
                const double v = (inr && ok) ? vv[q] : 0.0, w = inr ? (ok ? 1.0 : 0.0) : 1.0;
                if (kw != 0.0) { num = fma(kw, v, num); den = fma(kw, w, den); }
            }
        }
    }
    double* t = A.tmp + ((zl * A.c.ny + y) * A.c.nx + x) * 2;
    t[0] = num; t[1] = den;
}
__global__ __launch_bounds__(256) void spatial64_ypass_kernel(const Sp64Args A) {
    if (A.gate && *A.gate == 0u) return;
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t y = A.y0 + blockIdx.y, zl = blockIdx.z, z = A.z0 + zl;
    if (x >= A.c.nx) return;
    const int H = A.nky / 2;
    // a row outside the image is a row of valid zeros: its x-pass denominator is the whole x kernel
    double ksx = 0.0;
    for (int j = 0; j < A.nkx; ++j) ksx += A.kx[j];
    double num = 0.0, den = 0.0;
    constexpr int kIn = 8;
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    for (int j0 = 0; j0 < A.nky; j0 += kIn) {
        f64x2 tt[kIn];
#pragma unroll
        for (int q = 0; q < kIn; ++q) {
            const int64_t ic = min(max(y - H + j0 + q, (int64_t)0), A.c.ny - 1);
            tt[q] = *reinterpret_cast<const f64x2*>(A.tmp + ((zl * A.c.ny + ic) * A.c.nx + x) * 2);
        }
#pragma unroll
        for (int q = 0; q < kIn; ++q) {
            const int j = j0 + q;
            if (j < A.nky) {
                const double kw = A.ky[A.nky - 1 - j];
                const int64_t i = y - H + j;
                const bool inr = i >= 0 && i < A.c.ny;           // (uniform) a row outside the image: valid zeros
                const double tn = inr ? tt[q].x : 0.0, td = inr ? tt[q].y : ksx;
                if (kw != 0.0) { num = fma(kw, tn, num); den = fma(kw, td, den); }
            }
        }
    }
    double res;
    if (den != 0.0) res = quot_top(num, den);
    else { double cv; res = inc64(A.c, A.m, z, y, x, cv) ? cv : NAN; }
    A.out[z * A.out_plane_stride + y * A.out_row_stride + x] = res;
}
// The two passes through LDS: a block of the x pass stages its row segment once (256 outputs + the halo; the untiled pass asks the
// texture path for 58 samples per output), a block of the y pass a tile of 16 rows x 64 columns of (num, den) pairs + the halo rows
// (464 bytes of L2 traffic per output otherwise).  Same arithmetic, same order.  The one-output x pass here serves halos of
// 128 to 511 columns; the four-output passes below serve the rest.
constexpr int kSpHaloMax = 511, kSpYRows = 16, kSpYHalo = 23;     // (y tiles of up to 62 rows x 64 columns x 16 bytes = 62 KB of dynamic LDS + the taps: inside the 64 KB a launch gets without hipFuncSetAttribute; 49 y taps and more take the untiled pass)
__global__ __launch_bounds__(256) void spatial64_xpass_lds_kernel(const Sp64Args A) {
    if (A.gate && *A.gate == 0u) return;
    __shared__ double sv[256 + 2 * kSpHaloMax];
    __shared__ float sw[256 + 2 * kSpHaloMax];
    __shared__ double sk[2 * kSpHaloMax + 1];                   // the flipped taps (a scalar load per tap waited out its latency in every lane's loop)
    const int t = threadIdx.x, H = A.nkx / 2;
    for (int j = t; j < A.nkx; j += 256) sk[j] = A.kx[A.nkx - 1 - j];
    const int64_t x0 = (int64_t)blockIdx.x * 256, y = A.y0 + blockIdx.y, zl = blockIdx.z, z = A.z0 + zl;
    const bool arr = (A.m.flags & SPC_MASK_ARRAY) != 0;
    const double* pd = A.c.p + z * A.c.plane_stride + y * A.c.row_stride;
    const uint8_t* pmk = arr ? A.m.arr + z * A.m.plane_stride + y * A.m.row_stride : nullptr;
    for (int e = t; e < 256 + 2 * H; e += 256) {
        const int64_t i = x0 - H + e, ic = min(max(i, (int64_t)0), A.c.nx - 1);
        const double v = pd[ic];
        const bool inr = i >= 0 && i < A.c.nx, ok = spc_pred_valid(A.m, v) && (!arr || pmk[ic] != 0);
        sv[e] = (inr && ok) ? v : 0.0;
        sw[e] = inr ? (ok ? 1.f : 0.f) : 1.f;                    // outside the image: a valid zero
    }
    __syncthreads();
    const int64_t x = x0 + t;
    if (x >= A.c.nx) return;
    double num = 0.0, den = 0.0;
    for (int j = 0; j < A.nkx; ++j) {                            // astropy's order along the fast axis
        const double kw = sk[j];                                 // flipped kernel, input x - H + j
        if (kw != 0.0) { num = fma(kw, sv[t + j], num); den = fma(kw, (double)sw[t + j], den); }
    }
    double* o = A.tmp + ((zl * A.c.ny + y) * A.c.nx + x) * 2;
    o[0] = num; o[1] = den;
}
// Round 6: the same two passes with FOUR adjacent outputs per thread.  A sample read from LDS feeds up to four accumulators
// (the outputs x .. x + 3 / the rows y .. y + 3 see it under the taps j .. j - 3, kept in a four-deep register window), so a
// block reads (nk + 3) samples and taps per four outputs where the one-output passes read nk per output: the passes were bound
// by LDS traffic (3 reads per tap and output), not by the 2 x nk float64 FMAs.  Every output still adds its taps in astropy's
// order (j ascending), zero taps skipped: the same float64 results, bit for bit.
// x pass: a block = 1024 outputs of one row; samples in LDS at s + (s >> 2) - one pad per four - so that the lanes of a wave,
// four samples apart, read 64-bit words five apart: no bank is asked twice within a half wave.
constexpr int kSpX4Halo = 127, kSpX4Out = 1024;
__device__ __forceinline__ int sp64_skew(int s) { return s + (s >> 2); }
__global__ __launch_bounds__(256) void spatial64_xpass_lds4_kernel(const Sp64Args A) {
    if (A.gate && *A.gate == 0u) return;
    constexpr int N = kSpX4Out + 2 * kSpX4Halo + 4;
    __shared__ double sv[N + N / 4 + 1];
    __shared__ float sw[N + N / 4 + 1];
    __shared__ double sk[2 * kSpX4Halo + 1];
    const int t = threadIdx.x, H = A.nkx / 2;
    for (int j = t; j < A.nkx; j += 256) sk[j] = A.kx[A.nkx - 1 - j];
    const int64_t x0 = (int64_t)blockIdx.x * kSpX4Out, y = A.y0 + blockIdx.y, zl = blockIdx.z, z = A.z0 + zl;
    const bool arr = (A.m.flags & SPC_MASK_ARRAY) != 0;
    const double* pd = A.c.p + z * A.c.plane_stride + y * A.c.row_stride;
    const uint8_t* pmk = arr ? A.m.arr + z * A.m.plane_stride + y * A.m.row_stride : nullptr;
    for (int e = t; e < kSpX4Out + 2 * H + 3; e += 256) {
        const int64_t i = x0 - H + e, ic = min(max(i, (int64_t)0), A.c.nx - 1);
        const double v = pd[ic];
        const bool inr = i >= 0 && i < A.c.nx, ok = spc_pred_valid(A.m, v) && (!arr || pmk[ic] != 0);
        sv[sp64_skew(e)] = (inr && ok) ? v : 0.0;
        sw[sp64_skew(e)] = inr ? (ok ? 1.f : 0.f) : 1.f;         // outside the image: a valid zero
    }
    __syncthreads();
    const int64_t x = x0 + 4 * t;
    if (x >= A.c.nx) return;
    double num[4] = {0.0, 0.0, 0.0, 0.0}, den[4] = {0.0, 0.0, 0.0, 0.0};
    double k0 = 0.0, k1 = 0.0, k2 = 0.0, k3 = 0.0;               // taps i, i - 1, i - 2, i - 3 (0 outside the kernel: skipped like a zero tap)
    for (int i = 0; i < A.nkx + 3; ++i) {
        k3 = k2; k2 = k1; k1 = k0; k0 = i < A.nkx ? sk[i] : 0.0;
        const int p = sp64_skew(4 * t + i);
        const double v = sv[p], w = (double)sw[p];
        if (k0 != 0.0) { num[0] = fma(k0, v, num[0]); den[0] = fma(k0, w, den[0]); }
        if (k1 != 0.0) { num[1] = fma(k1, v, num[1]); den[1] = fma(k1, w, den[1]); }
        if (k2 != 0.0) { num[2] = fma(k2, v, num[2]); den[2] = fma(k2, w, den[2]); }
        if (k3 != 0.0) { num[3] = fma(k3, v, num[3]); den[3] = fma(k3, w, den[3]); }
    }
    double* o = A.tmp + ((zl * A.c.ny + y) * A.c.nx + x) * 2;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (x + q < A.c.nx) { o[2 * q] = num[q]; o[2 * q + 1] = den[q]; }
}
// y pass: a tile of kSpYRows + 2 H rows x 64 columns; thread (column, row group) takes the rows 4 g .. 4 g + 3
__global__ __launch_bounds__(256) void spatial64_ypass_lds4_kernel(const Sp64Args A) {
    if (A.gate && *A.gate == 0u) return;
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    extern __shared__ f64x2 tile[];                              // (kSpYRows + 2 H) x 64 pairs: sized by the launch
    __shared__ double sk[2 * kSpYHalo + 1];
    const int t = threadIdx.x, col = t & 63, rg = t >> 6, H = A.nky / 2;
    if (t < A.nky) sk[t] = A.ky[A.nky - 1 - t];
    const int64_t x = (int64_t)blockIdx.x * 64 + col, y0 = (int64_t)blockIdx.y * kSpYRows, zl = blockIdx.z, z = A.z0 + zl;
    double ksx = 0.0;                                            // a row outside the image: valid zeros under the whole x kernel
    for (int j = 0; j < A.nkx; ++j) ksx += A.kx[j];
    const int64_t xc = min(x, A.c.nx - 1);
    for (int r0 = rg; r0 < kSpYRows + 2 * H; r0 += 16) {         // (four rows per lane requested together, clamped into the image)
        f64x2 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t ic = min(max(y0 - H + r0 + 4 * q, (int64_t)0), A.c.ny - 1);
            v[q] = *reinterpret_cast<const f64x2*>(A.tmp + ((zl * A.c.ny + ic) * A.c.nx + xc) * 2);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int rr = r0 + 4 * q;
            const int64_t i = y0 - H + rr;
            if (rr < kSpYRows + 2 * H) tile[rr * 64 + col] = (i >= 0 && i < A.c.ny) ? v[q] : f64x2{0.0, ksx};
        }
    }
    __syncthreads();
    if (x >= A.c.nx) return;
    static_assert(kSpYRows == 16, "four row groups of four rows");
    double num[4] = {0.0, 0.0, 0.0, 0.0}, den[4] = {0.0, 0.0, 0.0, 0.0};
    double k0 = 0.0, k1 = 0.0, k2 = 0.0, k3 = 0.0;
    for (int i = 0; i < A.nky + 3; ++i) {
        k3 = k2; k2 = k1; k1 = k0; k0 = i < A.nky ? sk[i] : 0.0;
        const f64x2 tv = tile[(4 * rg + i) * 64 + col];
        if (k0 != 0.0) { num[0] = fma(k0, tv.x, num[0]); den[0] = fma(k0, tv.y, den[0]); }
        if (k1 != 0.0) { num[1] = fma(k1, tv.x, num[1]); den[1] = fma(k1, tv.y, den[1]); }
        if (k2 != 0.0) { num[2] = fma(k2, tv.x, num[2]); den[2] = fma(k2, tv.y, den[2]); }
        if (k3 != 0.0) { num[3] = fma(k3, tv.x, num[3]); den[3] = fma(k3, tv.y, den[3]); }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t y = y0 + 4 * rg + q;
        if (y >= A.c.ny) break;
        double res;
        if (den[q] != 0.0) res = quot_top(num[q], den[q]);
        else { double cv; res = inc64(A.c, A.m, z, y, x, cv) ? cv : NAN; }
        A.out[z * A.out_plane_stride + y * A.out_row_stride + x] = res;
    }
}
// Third form (round 6): ONE kernel, nothing between the passes.  A block = one plane x a strip of 256 columns x a band of rows;
// it marches DOWN the band: a row segment (256 + 2 H columns) is classified once into LDS as (valid ? sample : 0, validity)
// pairs, every thread gathers the x pass of ITS column from there (R reads of 16 bytes, 2 R float64 FMAs, taps in scalar
// registers), and the y pass runs in SCATTER form on registers: the R outputs the new row still contributes to live in R
// (numerator, denominator) accumulator pairs that move down one place per row - acc[r] = fma(k[r], X, acc[r + 1]) accumulates
// AND shifts, no copies - so that acc[0] is the output that has just seen its last row.  The cube is read once and written
// once (the two-pass forms above move another 32 bytes per voxel through the workspace and re-read the y halo of every
// 16-row tile: traffic x2.9 of the algorithmic bytes).  Every output adds its taps in the order of the passes above (x taps
// ascending, then rows ascending): the same float64 values.  Symmetric kernels of up to R taps per axis (zero-padded to R;
// 17 distinct taps per axis fit the scalar registers, 33 would not); a padded tap times an INFINITE valid sample would be NaN
// where the passes above skip zero taps, so a block that meets one (only possible when the mask admits infinities) raises
// a flag and the two-pass kernels - launched behind it, retiring at once while the flag is clear - redo the call.
template <int R>
struct Ring64Args {
    Cube64 c;
    MaskDev64 m;
    double* out;
    int64_t out_row_stride, out_plane_stride;
    double ky[R / 2 + 1], kx[R / 2 + 1];    // k'[i] = k'[R - 1 - i], i = 0 .. R / 2: the taps centred in R entries
    double ksx;                             // the x taps' sum: what a row outside the image (valid zeros) gives
    int nstrips, nbands, band_rows;
    unsigned* flag;                         // != nullptr: the mask admits infinite samples
};
template <int R, bool ARR>
__global__ __launch_bounds__(256, 2) void spatial64_ring_kernel(const Ring64Args<R> A) {
    constexpr int H = R / 2, W = 256, NS = W + 2 * H;
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    __shared__ f64x2 buf[2][NS];
    const int t = threadIdx.x;
    int64_t b = blockIdx.x;                                  // strips fastest: x neighbours (2 H shared columns) run side by side
    const int strip = (int)(b % A.nstrips); b /= A.nstrips;
    const int band = (int)(b % A.nbands);
    const int64_t z = b / A.nbands;
    const int nx = (int)A.c.nx, ny = (int)A.c.ny;            // (ny <= 65535 and nx < 2^31: checked by the entry point)
    const int x0 = strip * W;
    const int ya = band * A.band_rows, yb = min(ya + A.band_rows, ny);
    const bool second = t < 2 * H;                           // this thread also stages element W + t (the first wave's lanes: R <= 33)
    const bool wave0 = __builtin_amdgcn_readfirstlane(t >> 6) == 0;
    const int c0 = x0 - H + t, c1 = c0 + W;
    const bool in0 = c0 >= 0 && c0 < nx, in1 = c1 < nx;
    // (lanes without a second element ask for their first one again - every lane issues both loads, see load_row - instead of
    //  fetching 256 columns of the NEXT strip: the kernel read 1.8x its input that way, PMC)
    const unsigned cc0 = (unsigned)min(max(c0, 0), nx - 1), cc1 = second ? (unsigned)min(c1, nx - 1) : cc0;
    const double* pd = A.c.p + z * A.c.plane_stride;
    const uint8_t* pm = ARR ? A.m.arr + z * A.m.plane_stride : nullptr;
    // the ring: logical place r of the row with phase q (= row mod U inside an unrolled group of U rows) is the register pair
    // q + r, so that a row accumulates IN PLACE (v_fmac_f64) and the places move down by U registers once per U rows
    // (64 / U v_mov_b64 per row; a place that moves down every row costs 66, or hand-written three-address FMAs the register
    // allocator answers with scratch)
    constexpr int U = 4, NR = R + U - 1;
    double sn[NR], sd[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) { sn[r] = 0.0; sd[r] = 0.0; }
    // the rows' own samples: asked for kPre rows ahead (a row of this wave lasts ~1.5 us, a fetch from HBM under load longer
    // than that), slot = the row's phase.  Straight-line code - rows clamped into the image, every lane asks for both of
    // "its" elements - so that the compiler can count the loads in flight (behind a branch it waits for all of them)
    constexpr int kPre = 3;
    double rq0[U], rq1[U];
    unsigned mq0[U], mq1[U];
#pragma unroll
    for (int q = 0; q < U; ++q) { rq0[q] = 0.0; rq1[q] = 0.0; mq0[q] = 1u; mq1[q] = 1u; }
    auto load_row = [&](auto slot, int u) {                  // (a uniform row pointer + a 32-bit lane offset)
        constexpr int S = decltype(slot)::value;
        const int uc = min(max(u, 0), ny - 1);
        const double* q = pd + (int64_t)uc * A.c.row_stride;
        rq0[S] = q[cc0];
        rq1[S] = q[cc1];
        if (ARR) {
            const uint8_t* qm = pm + (int64_t)uc * A.m.row_stride;
            mq0[S] = qm[cc0];
            mq1[S] = qm[cc1];
        }
    };
    const int u_begin = ya - H, u_end = yb + H;
    static_assert(kPre == 3 && U == 4, "the first rows' slots written out");
    load_row(std::integral_constant<int, 0>{}, u_begin);
    load_row(std::integral_constant<int, 1>{}, u_begin + 1);
    load_row(std::integral_constant<int, 2>{}, u_begin + 2);
    bool seen_inf = false;
    const int x = x0 + t;
    double* po = A.out + z * A.out_plane_stride + x;
    // Software pipeline: the step of row u stages row u, runs the y pass of row u - 1 (Xpn, Xpd: registers only), then the
    // x pass of row u from LDS.  A row outside the image is staged as valid zeros (its x pass gives (0, sum of the x taps)
    // like any other row: one code path); the march runs on to a multiple of U rows past the band (nothing is stored there).
    double Xpn = 0.0, Xpd = 0.0;                             // (before the first row: zeros into an empty ring)
    auto row_step = [&](auto phase, const int u) {
        constexpr int Q = decltype(phase)::value;
        const bool row_in = u >= 0 && u < ny;                // (uniform)
        const double r0 = rq0[Q], r1 = rq1[Q];
        const unsigned m0 = mq0[Q], m1 = mq1[Q];
        f64x2* const Bw = buf[Q & 1];                        // (U is even: the buffer is the phase's parity)
        {
            const bool ok = spc_pred_valid(A.m, r0) && m0 != 0u;
            Bw[t] = (in0 && row_in) ? (ok ? f64x2{r0, 1.0} : f64x2{0.0, 0.0}) : f64x2{0.0, 1.0};      // outside the image: a valid zero
            if (A.flag) seen_inf = seen_inf || (ok && in0 && row_in && fabs(r0) == INFINITY);
        }
        if (wave0 && second) {                              // (a scalar branch for three of the four waves)
            const bool ok = spc_pred_valid(A.m, r1) && m1 != 0u;
            Bw[W + t] = (in1 && row_in) ? (ok ? f64x2{r1, 1.0} : f64x2{0.0, 0.0}) : f64x2{0.0, 1.0};
            if (A.flag) seen_inf = seen_inf || (ok && in1 && row_in && fabs(r1) == INFINITY);
        }
        load_row(std::integral_constant<int, (Q + kPre) % U>{}, u + kPre);      // in flight under the arithmetic of three rows
        // (one barrier per row: a buffer is written again two rows later, behind the barrier of the row in between)
        __syncthreads();
        // y pass of row u - 1: place r takes tap R - 1 - r (symmetric: tap r); place 0 has then seen its last row
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double kk = A.ky[r <= H ? r : R - 1 - r];
            sn[Q + r] = fma(kk, Xpn, sn[Q + r]);
            sd[Q + r] = fma(kk, Xpd, sd[Q + r]);
        }
        const int y = u - 1 - H;
        if (y >= ya && y < yb && x < nx) {
            // (no tap negative, centre taps positive: an empty window means an invalid centre sample - NaN, no second look at the cube,
            //  and no load behind a branch)
            po[(int64_t)y * A.out_row_stride] = sd[Q] != 0.0 ? quot_top(sn[Q], sd[Q]) : NAN;
        }
        // x pass of row u.  Left alone the compiler asks for all R pairs at once - 132 registers beside the ring's 144 - and
        // sends a part of the ring to scratch (a sched_barrier does not hold the reads back: they are hoisted before the
        // machine scheduler runs).  The reads of a group's slots therefore go through a pointer that an empty asm statement
        // "redefines" together with the running sum: they cannot move above the FMAs that emptied their slots.
        constexpr int kD = 8, kG = 4;                        // pairs in flight, taps per group
        typedef const f64x2 __attribute__((address_space(3)))* lds_pairs;
        lds_pairs Bp = (lds_pairs)(Bw + t);
        double Xn = 0.0, Xd = 0.0;
        f64x2 sq[kD];
#pragma unroll
        for (int j = 0; j < kD; ++j) sq[j] = Bp[j];
        auto group = [&](auto gc) {
            constexpr int g = decltype(gc)::value;
#pragma unroll
            for (int q = 0; q < kG; ++q) {
                const int j = g * kG + q;
                if (j < R) {
                    const double kk = A.kx[j <= H ? j : R - 1 - j];
                    Xn = fma(kk, sq[j % kD].x, Xn);
                    Xd = fma(kk, sq[j % kD].y, Xd);
                }
            }
            asm volatile("" : "+v"(Bp), "+v"(Xn), "+v"(Xd));
#pragma unroll
            for (int q = 0; q < kG; ++q) {
                const int j = g * kG + q;
                if (j + kD < R) sq[j % kD] = Bp[j + kD];
            }
        };
        for_each_const(group, std::make_integer_sequence<int, (R + kG - 1) / kG>{});
        Xpn = Xn; Xpd = Xd;
    };
    static_assert(U == 4, "four phases written out");
    for (int u0 = u_begin; u0 <= u_end; u0 += U) {
        row_step(std::integral_constant<int, 0>{}, u0);
        row_step(std::integral_constant<int, 1>{}, u0 + 1);
        row_step(std::integral_constant<int, 2>{}, u0 + 2);
        row_step(std::integral_constant<int, 3>{}, u0 + 3);
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            sn[i] = i + U < NR ? sn[i + U] : 0.0;
            sd[i] = i + U < NR ? sd[i + U] : 0.0;
        }
    }
    if (A.flag && seen_inf) atomicOr(A.flag, 1u);
}

__global__ __launch_bounds__(256) void spatial64_direct_kernel(const Sp64Args A) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t y = A.y0 + blockIdx.y, z = A.z0 + blockIdx.z;
    if (x >= A.c.nx) return;
    const int Hy = A.nky / 2, Hx = A.nkx / 2;
    double num = 0.0, den = 0.0;
    for (int jy = 0; jy < A.nky; ++jy) {
        const int64_t iy = y - Hy + jy;
        for (int jx = 0; jx < A.nkx; ++jx) {
            const double kw = A.ky[(A.nky - 1 - jy) * A.nkx + (A.nkx - 1 - jx)];
            if (kw == 0.0) continue;
            const int64_t ix = x - Hx + jx;
            double v = 0.0, w = 1.0;
            if (iy >= 0 && iy < A.c.ny && ix >= 0 && ix < A.c.nx) {
                if (!inc64(A.c, A.m, z, iy, ix, v)) { v = 0.0; w = 0.0; }
            }
            num = fma(kw, v, num); den = fma(kw, w, den);
        }
    }
    double res;
    if (den != 0.0) res = quot_top(num, den);
    else { double cv; res = inc64(A.c, A.m, z, y, x, cv) ? cv : NAN; }
    A.out[z * A.out_plane_stride + y * A.out_row_stride + x] = res;
}

template <int R>
int launch_ring64(hipStream_t st, const Sp64Args& S, const double* h_ky, int nky, const double* h_kx, int nkx, unsigned* d_flag) {
    Ring64Args<R> A{};
    A.c = S.c; A.m = S.m; A.out = S.out; A.out_row_stride = S.out_row_stride; A.out_plane_stride = S.out_plane_stride;
    const int py = (R - nky) / 2, px = (R - nkx) / 2;           // the taps centred in R entries; symmetric: the first half names them all
    for (int i = 0; i <= R / 2; ++i) {
        A.ky[i] = (i >= py) ? h_ky[i - py] : 0.0;
        A.kx[i] = (i >= px) ? h_kx[i - px] : 0.0;
    }
    double ksx = 0.0;
    for (int j = 0; j < nkx; ++j) ksx = fma(h_kx[nkx - 1 - j], 1.0, ksx);      // the x pass of a row of valid zeros, in its order
    A.ksx = ksx;
    A.flag = d_flag;
    A.nstrips = (int)((S.c.nx + 255) / 256);
    // bands: the whole column when the planes and strips alone fill the chip, else bands of >= 64 rows (2 (R / 2) halo rows each)
    const int64_t base = S.c.nz * A.nstrips;
    int64_t nb = std::max<int64_t>(1, std::min<int64_t>((2048 + base - 1) / base, (S.c.ny + 63) / 64));
    A.band_rows = (int)((S.c.ny + nb - 1) / nb);
    A.nbands = (int)((S.c.ny + A.band_rows - 1) / A.band_rows);
    const int64_t nblocks = base * A.nbands;
    SPC_REQUIRE(nblocks < (1ll << 31), "too many blocks");
    if (S.m.flags & SPC_MASK_ARRAY) hipLaunchKernelGGL((spatial64_ring_kernel<R, true>), dim3((unsigned)nblocks), dim3(256), 0, st, A);
    else hipLaunchKernelGGL((spatial64_ring_kernel<R, false>), dim3((unsigned)nblocks), dim3(256), 0, st, A);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

}  // namespace

// taps + the (num, den) planes of a slab: at most 256 MiB (the caller keeps its scratch), at least one plane; + the ring form's flag word
size_t spc_ws_spatial_conv_f64(int64_t nz, int64_t ny, int64_t nx, int64_t nky, int64_t nkx) {
    const size_t plane = (size_t)ny * (size_t)nx * 2 * sizeof(double);
    const size_t slab = std::max<size_t>(plane, std::min<size_t>((size_t)nz * plane, (size_t)1 << 28));
    return spc_ws_round(sizeof(double) * (size_t)(std::max<int64_t>(nky, 1) * std::max<int64_t>(nkx, 1) + nky + nkx)) + spc_ws_round(slab) + 512 + 256;
}

extern "C" {

int spc_spatial_conv_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, const double* h_ky, int nky,
                         const double* h_kx, int nkx, int separable, double* d_out, int64_t out_row_stride, int64_t out_plane_stride,
                         void* d_workspace, size_t workspace_bytes) {
    Sp64Args A{};
    int rc = cube64_args(cube, mask, &A.c, &A.m);
    if (rc) return rc;
    SPC_REQUIRE(h_ky && d_out && (!separable || h_kx), "NULL pointer argument");
    SPC_REQUIRE(nky >= 1 && (nky & 1) && nkx >= 1 && (nkx & 1) && nky <= 1023 && nkx <= 1023,
                "kernel axes must be odd and at most 1023 (got %d x %d)", nky, nkx);
    if (separable) {                                            // (the sum of an outer product is the product of the sums)
        double sy = 0.0, sx = 0.0;
        for (int i = 0; i < nky; ++i) sy += h_ky[i];
        for (int i = 0; i < nkx; ++i) sx += h_kx[i];
        const double prod = sy * sx;
        rc = check_kernel_sum(&prod, 1);
    } else {
        rc = check_kernel_sum(h_ky, (size_t)nky * (size_t)nkx);
    }
    if (rc) return rc;
    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    SpcWorkspace ws(d_workspace, workspace_bytes);
    const size_t ntab = separable ? (size_t)(nky + nkx) : (size_t)nky * (size_t)nkx;
    SPC_WS_TAKE(d_k, ws, double, ntab);
    if (separable) {
        SPC_HIP(spc_table_upload(d_k, h_ky, sizeof(double) * (size_t)nky, st));
        SPC_HIP(spc_table_upload(d_k + nky, h_kx, sizeof(double) * (size_t)nkx, st));
        A.ky = d_k; A.kx = d_k + nky;
    } else {
        SPC_HIP(spc_table_upload(d_k, h_ky, sizeof(double) * ntab, st));
        A.ky = d_k; A.kx = nullptr;
    }
    A.nky = nky; A.nkx = nkx; A.out = d_out;
    A.out_row_stride = out_row_stride ? out_row_stride : cube->nx;
    A.out_plane_stride = out_plane_stride ? out_plane_stride : cube->ny * A.out_row_stride;
    const unsigned gx = (unsigned)((cube->nx + 255) / 256);
    // kernels with one row per blockIdx.y: slabs of at most 65535 rows (gridDim.y), the rows addressed from A.y0 (the stencils
    // read their halo rows from the whole image)
    auto over_rows = [&](auto launch) -> int {
        for (int64_t y0 = 0; y0 < cube->ny; y0 += 65535) {
            A.y0 = y0;
            launch((unsigned)std::min<int64_t>(65535, cube->ny - y0));
            SPC_LAUNCH_CHECK();
        }
        A.y0 = 0;
        return SPC_OK;
    };
    if (!separable) {
        for (int64_t z0 = 0; z0 < cube->nz; z0 += 65535) {
            A.z0 = z0;
            const unsigned gz = (unsigned)std::min<int64_t>(65535, cube->nz - z0);
            rc = over_rows([&](unsigned gy) { hipLaunchKernelGGL(spatial64_direct_kernel, dim3(gx, gy, gz), dim3(256), 0, st, A); });
            if (rc) return rc;
        }
        return SPC_OK;
    }
    // symmetric factors of up to 33 taps, none negative, centre taps positive: the one-kernel ring form (SPC_SPATIAL64_RING=0: the
    // two-pass forms)
    const bool ring_on = spc_switch("SPC_SPATIAL64_RING", 1) != 0;     // (read per call: the tests compare both forms in one process)
    bool ring = ring_on && nky <= 33 && nkx <= 33 && h_ky[nky / 2] > 0.0 && h_kx[nkx / 2] > 0.0;
    for (int i = 0; ring && i < nky / 2; ++i) ring = h_ky[i] == h_ky[nky - 1 - i] && h_ky[i] >= 0.0;
    for (int i = 0; ring && i < nkx / 2; ++i) ring = h_kx[i] == h_kx[nkx - 1 - i] && h_kx[i] >= 0.0;
    A.gate = nullptr;
    if (ring) {
        unsigned* d_flag = nullptr;
        if (!(A.m.flags & SPC_MASK_FINITE)) {                   // the mask admits infinite samples: see spatial64_ring_kernel
            SPC_WS_TAKE(d_f, ws, unsigned, 64);
            d_flag = d_f;
            SPC_HIP(hipMemsetAsync(d_flag, 0, sizeof(unsigned), st));
        }
        if (std::max(nky, nkx) <= 17) rc = launch_ring64<17>(st, A, h_ky, nky, h_kx, nkx, d_flag);
        else rc = launch_ring64<33>(st, A, h_ky, nky, h_kx, nkx, d_flag);
        if (rc) return rc;
        if (!d_flag) return SPC_OK;
        A.gate = d_flag;                                        // the passes below run only if the ring kernel raised the flag
    }
    const size_t plane = (size_t)cube->ny * (size_t)cube->nx * 2 * sizeof(double);
    const size_t avail = ws.size > ws.used + 512 ? ws.size - ws.used - 512 : 0;
    const int64_t planes = (int64_t)std::min<size_t>(std::min<size_t>(avail / plane, (size_t)cube->nz), 65535);
    SPC_REQUIRE(planes >= 1, "d_workspace too small: the (num, den) planes of one channel need %zu bytes more (spc_workspace_bytes)", plane);
    SPC_WS_TAKE(d_tmp, ws, double, (size_t)planes * (size_t)cube->ny * (size_t)cube->nx * 2);
    A.tmp = d_tmp;
    for (int64_t z0 = 0; z0 < cube->nz; z0 += planes) {
        A.z0 = z0;
        const unsigned gz = (unsigned)std::min<int64_t>(planes, cube->nz - z0);
        // LDS tiles with four outputs per thread where the halo fits them, one output per thread (x pass) or the untiled pass beyond
        rc = over_rows([&](unsigned gy) {
            if (nkx / 2 <= kSpX4Halo)
                hipLaunchKernelGGL(spatial64_xpass_lds4_kernel, dim3((unsigned)((cube->nx + kSpX4Out - 1) / kSpX4Out), gy, gz), dim3(256), 0, st, A);
            else if (nkx / 2 <= kSpHaloMax)
                hipLaunchKernelGGL(spatial64_xpass_lds_kernel, dim3(gx, gy, gz), dim3(256), 0, st, A);
            else
                hipLaunchKernelGGL(spatial64_xpass_kernel, dim3(gx, gy, gz), dim3(256), 0, st, A);
        });
        if (rc) return rc;
        if (nky / 2 <= kSpYHalo && (cube->ny + kSpYRows - 1) / kSpYRows <= 65535)
            hipLaunchKernelGGL(spatial64_ypass_lds4_kernel, dim3((unsigned)((cube->nx + 63) / 64), (unsigned)((cube->ny + kSpYRows - 1) / kSpYRows), gz),
                               dim3(256), (size_t)(kSpYRows + 2 * (nky / 2)) * 64 * 16, st, A);
        else
            rc = over_rows([&](unsigned gy) { hipLaunchKernelGGL(spatial64_ypass_kernel, dim3(gx, gy, gz), dim3(256), 0, st, A); });
        SPC_LAUNCH_CHECK();
        if (rc) return rc;
    }
    return SPC_OK;
}

}  // extern "C"
