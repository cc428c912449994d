// spc_stack.hip - Fourier-shift every spectrum by its own (fractional) number of channels and stack them:
// spectral_cube.analysis_utilities.stack_spectra / fourier_shift / _fourier_shifter (analysis_utilities.py:14-94, 134-318).
//
// The reference's shift (fft, phase ramp exp(-2 pi i m s) over np.fft.fftfreq, ifft, real part) of a length-M sequence is
// a circular convolution with a real, M-periodic kernel
//     h_M(t) = sin(pi t) / (M sin(pi t / M))   M odd,      sin(pi t) / (M tan(pi t / M))   M even,      1 where M | t
// so  out[n] = sum_j x[j] h_M(n - j - s), x the zero-padded spectrum with every non-finite sample set to 0.  With
// s = si + f (si = rint(s), |f| <= 1/2) the kernel is needed at k - f for the M integers k only:
//     sin(pi (k - f)) = -(-1)^k sin(pi f),    sin(pi (k - f) / M) = S[k] cos(pi f / M) - C[k] sin(pi f / M)
// with S[k] = sin(pi k / M), C[k] = cos(pi k / M) from ONE table shared by every spaxel: a spaxel's M kernel values cost
// three sin / cos and M divisions, not M sines.  |f| <= 1/2 keeps the subtraction away from cancellation (|k - f| >= 1/2
// for k != 0, and k = 0 is -sin(pi f / M) exactly); f = 0 is the unit impulse, so an integer shift is a gather.
//
//  * a block of 256 lanes takes G (1, 2, 4 or 8: as many as fit 64 KiB of LDS) consecutive positions of the list; the
//    spectra are staged with the position index fastest, so neighbouring lanes read neighbouring x of one image plane.
//  * filled samples (mask predicate and fill fused into the load), non-finite ones as 0 plus an indicator byte.
//  * every spaxel's kernel values are built once in LDS; a work item is (spaxel, ST_R consecutive output channels): the
//    ST_R kernel values it needs slide by one per input channel, so they live in registers (the channel loop is unrolled
//    ST_R times and the register window rotates) and a step costs one LDS broadcast of the sample, one LDS load of a
//    kernel value and ST_R float64 FMAs.  ST_R is odd: lanes ST_R doubles apart never share an LDS bank.
//  * a spectrum without a non-finite sample skips the indicator convolution, as the reference does (:44-47, 74-76).
//  * M = 8192 runs with G = 1 and up to 138 KiB of LDS: the channel loop is tiled, never the block.
//  * the fused stack never writes a shifted spectrum: every (block, spaxel slot) owns a row of partial sums and counts
//    in the workspace, touched by one lane per channel; a second kernel adds the rows in slot order.  No floating-point
//    atomics, and the split into blocks depends on the sizes alone: two runs agree bit for bit.
#include "spc_common.h"

namespace {

constexpr int ST_BLOCK = 256;
constexpr int ST_R = 9;                    // output channels per work item (odd)
constexpr int ST_GMAX = 8;                 // spaxels per block and round
constexpr size_t ST_LDS_SMALL = 64 * 1024;
constexpr size_t ST_LDS_MAX = 160 * 1024;

template <typename T>
struct StArgs {
    const T* in;
    int64_t nz, ny, nx, rs, ps;           // input view, strides in elements
    SpcInclude<T> m;                      // which samples count; the others enter as fill
    T fill;
    const int32_t* idx;                   // npos flat spaxel indices y * nx + x
    const double* shift;                  // npos shifts in channels (NaN: an all-NaN row)
    int64_t npos;
    int pad_lo, M, nzp;                   // leading pad, padded length, nz rounded up to ST_R
    const double* tab;                    // S[0 .. M), C[0 .. M)
    double* out;                          // (M, npos) shifted spectra, or nullptr (fused)
    double* psum;                         // fused: (slots, M) partial sums
    uint32_t* pcnt;                       //        (slots, M) rows that are not NaN
    int G, logG;
    int64_t ngroups, gpb;                 // groups of G positions; groups per block
};

__global__ __launch_bounds__(ST_BLOCK) void st_table_kernel(double* tab, int M) {
    const int k = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (k >= M) return;
    const int kk = k < M - k ? k : M - k;                  // sin(pi k / M) = sin(pi (M - k) / M): the argument stays <= 1/2
    const double a = (double)kk / (double)M;
    tab[k] = sinpi(a);
    tab[M + k] = 2 * k > M ? -cospi(a) : cospi(a);
}

// the ST_R outputs n0 ... n0 + ST_R - 1 of one spaxel: acc = sum_z x[z] g[(n - z - c) mod M], ai the same of the indicator
template <typename T, bool IND>
__device__ __forceinline__ void st_fir(const double* g, const T* x, const uint8_t* b, int nzp, int M, int i0,
                                       double (&acc)[ST_R], double (&ai)[ST_R]) {
    double W[ST_R];                        // logical window w[r] = g[(i0 + r - z) mod M] lives in W[(r - u) mod ST_R]
    int j = i0;
#pragma unroll
    for (int r = 0; r < ST_R; ++r) {
        W[r] = g[j];
        j = (j + 1 == M) ? 0 : j + 1;
        acc[r] = 0.0;
        ai[r] = 0.0;
    }
    j = (i0 == 0) ? M - 1 : i0 - 1;        // the value that enters the window at the next channel
    for (int zb = 0; zb < nzp; zb += ST_R) {
#pragma unroll
        for (int u = 0; u < ST_R; ++u) {
            const double xv = (double)x[zb + u];
            const double bv = IND ? (double)b[zb + u] : 0.0;
#pragma unroll
            for (int r = 0; r < ST_R; ++r) {
                const double w = W[(r - u + ST_R) % ST_R];
                acc[r] = fma(xv, w, acc[r]);
                if (IND) ai[r] = fma(bv, w, ai[r]);
            }
            W[(ST_R - 1 - u) % ST_R] = g[j];
            j = (j == 0) ? M - 1 : j - 1;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(ST_BLOCK) void st_shift_kernel(const StArgs<T> A) {
    extern __shared__ __align__(16) unsigned char st_smem[];
    const int M = A.M, nzp = A.nzp, G = A.G;
    double* gt = reinterpret_cast<double*>(st_smem);                         // G x M kernel values
    T* xs = reinterpret_cast<T*>(gt + (size_t)G * M);                        // G x nzp samples (non-finite -> 0)
    uint8_t* bad = reinterpret_cast<uint8_t*>(xs + (size_t)G * nzp);         // G x nzp indicator bytes
    __shared__ int64_t s_y[ST_GMAX], s_x[ST_GMAX];
    __shared__ int s_good[ST_GMAX], s_bad[ST_GMAX], s_state[ST_GMAX], s_c[ST_GMAX], s_int[ST_GMAX];
    __shared__ double s_A[ST_GMAX], s_cf[ST_GMAX], s_sf[ST_GMAX];
    const int tid = threadIdx.x;
    const int ntiles = (M + ST_R - 1) / ST_R;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const int64_t g0 = (int64_t)blockIdx.x * A.gpb;
    const int64_t g1 = g0 + A.gpb < A.ngroups ? g0 + A.gpb : A.ngroups;
    for (int64_t grp = g0; grp < g1; ++grp) {
        const int64_t p0 = grp * G;
        const int ng = (int)(A.npos - p0 < G ? A.npos - p0 : G);
        if (tid < G) {
            int64_t sp = -1;
            if (tid < ng) sp = A.idx[p0 + tid];
            const bool ok = sp >= 0 && sp < A.ny * A.nx;                     // a position outside the map reads nothing
            s_y[tid] = ok ? sp / A.nx : -1;
            s_x[tid] = ok ? sp % A.nx : -1;
            s_good[tid] = 0;
            s_bad[tid] = 0;
        }
        __syncthreads();
        for (int e = tid; e < G * nzp; e += ST_BLOCK) {                      // position fastest: neighbouring lanes, neighbouring x
            const int gi = e & (G - 1), z = e >> A.logG;
            T val = (T)0;
            uint8_t isb = 0;
            if (z < A.nz && s_y[gi] >= 0) {
                const T v = A.in[z * A.ps + s_y[gi] * A.rs + s_x[gi]];
                const uint8_t mb = A.m.marr ? A.m.marr[z * A.m.mps + s_y[gi] * A.m.mrs + s_x[gi]] : (uint8_t)1;
                const T f = spc_include(A.m, v, mb) ? v : A.fill;
                if (spc_abs(f) <= std::numeric_limits<T>::max()) { val = f; s_good[gi] = 1; }        // (every writer stores the same 1)
                else { isb = 1; s_bad[gi] = 1; }
            }
            xs[(size_t)gi * nzp + z] = val;
            bad[(size_t)gi * nzp + z] = isb;
        }
        __syncthreads();
        if (tid < G) {
            int state = 0;                                                   // 0: all-NaN row, 1: no indicator, 2: with indicator
            if (tid < ng && s_y[tid] >= 0 && s_good[tid]) {
                const double s = A.shift[p0 + tid];
                if (fabs(s) <= 1.7976931348623157e308) {
                    const double si = rint(s), f = s - si;
                    int c = (int)fmod(si, (double)M) + A.pad_lo % M;         // out[n] takes g[(n - z - c) mod M]
                    c %= M;
                    if (c < 0) c += M;
                    s_c[tid] = c;
                    s_int[tid] = fabs(f) < 1e-30;
                    s_A[tid] = -sinpi(f) / (double)M;
                    s_cf[tid] = cospi(f / (double)M);
                    s_sf[tid] = sinpi(f / (double)M);
                    state = s_bad[tid] ? 2 : 1;
                }
            }
            s_state[tid] = state;
        }
        __syncthreads();
        for (int e = tid; e < ng * M; e += ST_BLOCK) {
            const int gi = e / M, k = e - gi * M;
            if (s_state[gi] == 0) continue;
            double v;
            if (s_int[gi]) {
                v = k == 0 ? 1.0 : 0.0;
            } else {
                const double S = A.tab[k], Cc = A.tab[M + k], cf = s_cf[gi], sf = s_sf[gi];
                double num = (k & 1) ? -s_A[gi] : s_A[gi];
                if (!(M & 1)) num *= Cc * cf + S * sf;
                v = num / (S * cf - Cc * sf);
            }
            gt[(size_t)gi * M + k] = v;
        }
        __syncthreads();
        for (int item = tid; item < ng * ntiles; item += ST_BLOCK) {
            const int gi = item / ntiles, n0 = (item - gi * ntiles) * ST_R;
            const int state = s_state[gi];
            const int64_t p = p0 + gi;
            double acc[ST_R], ai[ST_R];
            if (state != 0) {
                int i0 = n0 - s_c[gi];
                if (i0 < 0) i0 += M;
                const double* g = gt + (size_t)gi * M;
                const T* x = xs + (size_t)gi * nzp;
                const uint8_t* b = bad + (size_t)gi * nzp;
                if (state == 2) st_fir<T, true>(g, x, b, nzp, M, i0, acc, ai);
                else st_fir<T, false>(g, x, b, nzp, M, i0, acc, ai);
            }
            const int64_t slot = (int64_t)blockIdx.x * G + gi;
#pragma unroll
            for (int r = 0; r < ST_R; ++r) {
                const int n = n0 + r;
                if (n >= M) break;
                const bool isn = state == 0 || (state == 2 && ai[r] > 0.5);
                if (A.out) {
                    A.out[(int64_t)n * A.npos + p] = isn ? qnan : acc[r];
                } else if (!isn) {
                    A.psum[slot * M + n] += acc[r];                          // this lane alone owns (slot, n) in this round
                    A.pcnt[slot * M + n] += 1u;
                }
            }
        }
        __syncthreads();
    }
}

// the partial rows added in slot order: sum, rows that are not NaN, rows that are
__global__ __launch_bounds__(ST_BLOCK) void st_finish_kernel(const double* psum, const uint32_t* pcnt, int64_t nslots, int M, int64_t npos,
                                                             double* sum, int64_t* count, int64_t* nnan) {
    const int n = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (n >= M) return;
    double s = 0.0;
    int64_t c = 0;
    for (int64_t k = 0; k < nslots; ++k) {
        s += psum[k * M + n];
        c += pcnt[k * M + n];
    }
    sum[n] = s;
    count[n] = c;
    nnan[n] = npos - c;
}

// ---- host side -------------------------------------------------------------------------------------------------
struct StPlan {
    int M, nzp, G, logG;
    int64_t ngroups, nb, gpb;
    size_t lds;
};

inline size_t st_lds_bytes(int G, int M, int nzp, size_t elem) {
    return (size_t)G * ((size_t)M * 8 + (size_t)nzp * elem + (size_t)nzp);
}

// the split into blocks is a function of the sizes alone (never of the device): the fused sum is reproducible
inline StPlan st_plan(int64_t nz, int M, int64_t npos, size_t elem, bool fused) {
    StPlan p;
    p.M = M;
    p.nzp = (int)((nz + ST_R - 1) / ST_R * ST_R);
    p.G = ST_GMAX;
    p.logG = 3;
    while (p.G > 1 && st_lds_bytes(p.G, M, p.nzp, elem) > ST_LDS_SMALL) { p.G >>= 1; --p.logG; }
    p.lds = st_lds_bytes(p.G, M, p.nzp, elem);
    p.ngroups = (npos + p.G - 1) / p.G;
    int64_t cap = 65535;
    if (fused) {
        cap = (1 << 21) / M;
        cap = cap < 256 ? 256 : (cap > 1024 ? 1024 : cap);
    }
    p.nb = p.ngroups < cap ? p.ngroups : cap;
    if (p.nb < 1) p.nb = 1;
    p.gpb = (p.ngroups + p.nb - 1) / p.nb;
    if (p.gpb < 1) p.gpb = 1;
    p.nb = (p.ngroups + p.gpb - 1) / p.gpb;
    if (p.nb < 1) p.nb = 1;
    return p;
}

inline size_t st_ws_bytes(const StPlan& p, bool fused) {
    size_t n = spc_ws_round((size_t)2 * p.M * sizeof(double));
    if (fused) {
        const size_t cells = (size_t)p.nb * p.G * p.M;
        n += spc_ws_round(cells * sizeof(double)) + spc_ws_round(cells * sizeof(uint32_t));
    }
    return n + 256;
}

template <typename T>
int st_run(int device, void* stream, StArgs<T> A, const int32_t* d_idx, const double* d_shift, int64_t npos, int pad_lo, int pad_hi,
           double* d_out, double* d_sum, int64_t* d_count, int64_t* d_nan, void* d_workspace, size_t workspace_bytes) {
    const bool fused = d_out == nullptr;
    SPC_REQUIRE(d_idx != nullptr && d_shift != nullptr, "d_idx / d_shift is NULL");
    SPC_REQUIRE(npos >= 1 && npos <= 0x7fffffffLL * ST_GMAX, "the number of positions must be positive (got %lld)", (long long)npos);
    SPC_REQUIRE(pad_lo >= 0 && pad_hi >= 0, "the pads must not be negative (got %d, %d)", pad_lo, pad_hi);
    if (fused) SPC_REQUIRE(d_sum != nullptr && d_count != nullptr && d_nan != nullptr, "d_sum / d_count / d_nan is NULL");
    const int64_t M64 = A.nz + (int64_t)pad_lo + (int64_t)pad_hi;
    if (M64 > SPC_STACK_MAX_CHANNELS) {
        spc_set_error("a padded spectrum of %lld channels is above the built limit of %d", (long long)M64, SPC_STACK_MAX_CHANNELS);
        return SPC_ERR_UNSUPPORTED;
    }
    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const StPlan P = st_plan(A.nz, (int)M64, npos, sizeof(T), fused);
    SPC_REQUIRE(P.lds <= ST_LDS_MAX, "%zu bytes of LDS needed, %zu built", P.lds, ST_LDS_MAX);
    SpcWorkspace ws(d_workspace, workspace_bytes);
    SPC_WS_TAKE(tab, ws, double, 2 * (size_t)P.M);
    A.idx = d_idx; A.shift = d_shift; A.npos = npos;
    A.pad_lo = pad_lo; A.M = P.M; A.nzp = P.nzp; A.tab = tab;
    A.out = d_out; A.psum = nullptr; A.pcnt = nullptr;
    A.G = P.G; A.logG = P.logG; A.ngroups = P.ngroups; A.gpb = P.gpb;
    const int64_t nslots = P.nb * P.G;
    if (fused) {
        const size_t cells = (size_t)nslots * P.M;
        SPC_WS_TAKE(psum, ws, double, cells);
        SPC_WS_TAKE(pcnt, ws, uint32_t, cells);
        SPC_HIP(hipMemsetAsync(psum, 0, cells * sizeof(double), st));
        SPC_HIP(hipMemsetAsync(pcnt, 0, cells * sizeof(uint32_t), st));
        A.psum = psum; A.pcnt = pcnt;
    }
    hipLaunchKernelGGL(st_table_kernel, dim3((unsigned)((P.M + ST_BLOCK - 1) / ST_BLOCK)), dim3(ST_BLOCK), 0, st, tab, P.M);
    SPC_LAUNCH_CHECK();
    if (P.lds > ST_LDS_SMALL)
        SPC_HIP(hipFuncSetAttribute((const void*)st_shift_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds));
    hipLaunchKernelGGL((st_shift_kernel<T>), dim3((unsigned)P.nb), dim3(ST_BLOCK), P.lds, st, A);
    SPC_LAUNCH_CHECK();
    if (fused) {
        hipLaunchKernelGGL(st_finish_kernel, dim3((unsigned)((P.M + ST_BLOCK - 1) / ST_BLOCK)), dim3(ST_BLOCK), 0, st,
                           (const double*)A.psum, (const uint32_t*)A.pcnt, nslots, P.M, npos, d_sum, d_count, d_nan);
        SPC_LAUNCH_CHECK();
    }
    return SPC_OK;
}

template <typename T>
int st_entry(int device, void* stream, const typename SpcAbi<T>::cube* cube, const typename SpcAbi<T>::mask* mask, int nan_excluded, T fill,
             const int32_t* d_idx, const double* d_shift, int64_t npos, int pad_lo, int pad_hi, bool fused, double* d_out, double* d_sum,
             int64_t* d_count, int64_t* d_nan, void* d_workspace, size_t workspace_bytes) {
    StArgs<T> A{};
    int rc = sizeof(T) == 8 ? spc_check_cube_any_order_words(cube) : spc_check_cube(cube);
    if (rc) return rc;
    rc = spc_include_from(mask, cube, nan_excluded, &A.m);
    if (rc) return rc;
    A.in = cube->d_data; A.nz = cube->nz; A.ny = cube->ny; A.nx = cube->nx;
    A.rs = cube->row_stride; A.ps = cube->plane_stride;
    A.fill = fill;
    SPC_REQUIRE(fused || d_out != nullptr, "d_out is NULL");
    return st_run(device, stream, A, d_idx, d_shift, npos, pad_lo, pad_hi, d_out, d_sum, d_count, d_nan, d_workspace, workspace_bytes);
}

}  // namespace

extern "C" {

size_t spc_stack_workspace_bytes(int64_t nz, int64_t npos, int pad_lo, int pad_hi, int fused) {
    const int64_t M = nz + (int64_t)pad_lo + (int64_t)pad_hi;
    if (nz < 1 || npos < 1 || pad_lo < 0 || pad_hi < 0 || M > SPC_STACK_MAX_CHANNELS) return 0;
    const size_t a = st_ws_bytes(st_plan(nz, (int)M, npos, sizeof(float), fused != 0), fused != 0);
    const size_t b = st_ws_bytes(st_plan(nz, (int)M, npos, sizeof(double), fused != 0), fused != 0);
    return a > b ? a : b;
}

int spc_stack_shift_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded, float fill,
                        const int32_t* d_idx, const double* d_shift, int64_t npos, int pad_lo, int pad_hi, double* d_out,
                        void* d_workspace, size_t workspace_bytes) {
    return st_entry<float>(device, stream, cube, mask, nan_excluded, fill, d_idx, d_shift, npos, pad_lo, pad_hi, false, d_out, nullptr, nullptr,
                        nullptr, d_workspace, workspace_bytes);
}

int spc_stack_shift_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded, double fill,
                        const int32_t* d_idx, const double* d_shift, int64_t npos, int pad_lo, int pad_hi, double* d_out,
                        void* d_workspace, size_t workspace_bytes) {
    return st_entry<double>(device, stream, cube, mask, nan_excluded, fill, d_idx, d_shift, npos, pad_lo, pad_hi, false, d_out, nullptr, nullptr,
                        nullptr, d_workspace, workspace_bytes);
}

int spc_stack_sum_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded, float fill,
                      const int32_t* d_idx, const double* d_shift, int64_t npos, int pad_lo, int pad_hi, double* d_sum,
                      int64_t* d_count, int64_t* d_nan, void* d_workspace, size_t workspace_bytes) {
    return st_entry<float>(device, stream, cube, mask, nan_excluded, fill, d_idx, d_shift, npos, pad_lo, pad_hi, true, nullptr, d_sum, d_count,
                        d_nan, d_workspace, workspace_bytes);
}

int spc_stack_sum_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded, double fill,
                      const int32_t* d_idx, const double* d_shift, int64_t npos, int pad_lo, int pad_hi, double* d_sum,
                      int64_t* d_count, int64_t* d_nan, void* d_workspace, size_t workspace_bytes) {
    return st_entry<double>(device, stream, cube, mask, nan_excluded, fill, d_idx, d_shift, npos, pad_lo, pad_hi, true, nullptr, d_sum, d_count,
                        d_nan, d_workspace, workspace_bytes);
}

}  // extern "C"
