// spc_baseline.hip - polynomial baselines: fit a Legendre series to the line-free channels of every spectrum and subtract
// the model (docs/continuum_subtraction.rst does this for a constant with a masked median; anything of higher order goes
// through apply_function_parallel_spectral, spectral_cube.py:3103, one Python call per spectrum on the host; CASA's
// imcontsub fitorder=n).  The arithmetic is stated with the prototypes in include/spcube_hip.h.
//
// Fit: lanes run along x over the flattened (y, x) plane, so a narrow map still fills its waves; each lane owns a spaxel
// and keeps the upper triangle of G and the right-hand side b - (p+1)(p+2)/2 + (p+1) float64 sums, 27 at order 5 - in
// registers: the kernel is templated on the order.  blockIdx.y is a segment of the channel list.  A batch of BL_ZC list
// entries reads its channel numbers, then the mask bytes of all of them, then the samples those include, then does the
// arithmetic: the loads of a batch are in flight together (the include predicate is taken AFTER the loads - inside the branch
// that loads a sample it makes the compiler wait for every sample where it is loaded).  The basis row of a channel is the same for every lane: its
// address is uniform, the loads are scalar.  One segment: the lane solves and stores.  More: the partial sums go to the
// workspace, [segment][sum][spaxel] so that stores and loads are coalesced, and bl_finish_kernel adds them in segment
// order and solves.  No atomics anywhere.
// Apply: element-wise, the lane's coefficients in registers, batches of BL_ZA channels.
// Built with -ffp-contract=off: every product and sum is rounded on its own, so that the result can be restated in numpy.
#include "spc_common.h"

namespace {

constexpr int BL_BLOCK = 64;                  // one wave of spaxels
constexpr int BL_ZC = 8;                      // list entries per batch of the fit
constexpr int BL_ZA = 8;                      // channels per batch of the apply
constexpr int64_t BL_GRID_LIMIT = 65535;
constexpr int64_t BL_FULL_WAVES = 1024;       // 256 CUs x 4 SIMDs: a plane of this many waves is not split
constexpr int64_t BL_TARGET_WAVES = 2048;     // what a split plane is brought up to
constexpr int64_t BL_MIN_SEGMENT = 64;        // list entries a segment has at least
constexpr int64_t BL_MAX_SEGMENTS = 64;
constexpr int64_t BL_APPLY_TARGET_BLOCKS = 8192;

constexpr int bl_nacc(int order) { return (order + 1) * (order + 2) / 2 + (order + 1); }
// index of G_ab (a <= b) in the packed upper triangle, row by row
__host__ __device__ constexpr int bl_tri(int a, int b, int nc) { return a * nc - a * (a - 1) / 2 + (b - a); }

int64_t bl_segments(int64_t ny, int64_t nx, int64_t nfit) {
    const int64_t waves = (ny * nx + BL_BLOCK - 1) / BL_BLOCK;
    if (waves >= BL_FULL_WAVES || nfit < 2 * BL_MIN_SEGMENT) return 1;
    int64_t s = (BL_TARGET_WAVES + waves - 1) / waves;
    s = spc_min64(spc_min64(s, nfit / BL_MIN_SEGMENT), BL_MAX_SEGMENTS);
    const int64_t len = (nfit + s - 1) / s;
    return (nfit + len - 1) / len;            // no empty segment; the last one may be shorter
}

template <typename T>
struct BlFitArgs {
    const T* in;
    int64_t nz, nx, rs, ps, nspax;
    SpcInclude<T> m;
    const int32_t* chan;
    int64_t nfit, seg_len;
    int nseg;
    const double* basis;
    double* coef;
    int32_t* npts;
    double* part;                             // [nseg][nacc][nspax]
    int32_t* part_n;                          // [nseg][nspax]
};

// c = G^-1 b by G = L D L^T in the order the header states; NaN when n < P + 1 or a pivot is not > 0
template <int P>
__device__ __forceinline__ void bl_solve(const double* G, const double* b, int n, double* c) {
    constexpr int NC = P + 1;
    double L[NC][NC], D[NC];
    bool bad = n < NC;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        double s = G[bl_tri(j, j, NC)];
#pragma unroll
        for (int k = 0; k < j; ++k) s = s - L[j][k] * (L[j][k] * D[k]);
        D[j] = s;
        bad = bad | !(s > 0.0);
#pragma unroll
        for (int i = j + 1; i < NC; ++i) {
            double r = G[bl_tri(j, i, NC)];
#pragma unroll
            for (int k = 0; k < j; ++k) r = r - L[i][k] * (L[j][k] * D[k]);
            L[i][j] = r / s;
        }
    }
    double z[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - L[i][k] * z[k];
        z[i] = s;
    }
#pragma unroll
    for (int i = NC - 1; i >= 0; --i) {
        double s = z[i] / D[i];
#pragma unroll
        for (int k = i + 1; k < NC; ++k) s = s - L[k][i] * c[k];
        c[i] = s;
    }
    if (bad) {
#pragma unroll
        for (int i = 0; i < NC; ++i) c[i] = std::numeric_limits<double>::quiet_NaN();
    }
}

template <int P>
__device__ __forceinline__ void bl_store(double* coef, int32_t* npts, int64_t nspax, int64_t s, const double* G, const double* b, int n) {
    double c[P + 1];
    bl_solve<P>(G, b, n, c);
#pragma unroll
    for (int j = 0; j <= P; ++j) coef[j * nspax + s] = c[j];
    if (npts) npts[s] = n;
}

// blockIdx.x: BL_BLOCK spaxels of the flattened plane; blockIdx.y: a segment of the channel list
template <typename T, int P>
__global__ __launch_bounds__(BL_BLOCK) void bl_fit_kernel(const BlFitArgs<T> A) {
    constexpr int NC = P + 1, NG = NC * (NC + 1) / 2, NACC = NG + NC;
    constexpr int ZC = BL_ZC;
    const int64_t s = (int64_t)blockIdx.x * BL_BLOCK + threadIdx.x;
    if (s >= A.nspax) return;
    const int64_t y = s / A.nx, x = s - y * A.nx;
    const int64_t off = y * A.rs + x, moff = y * A.m.mrs + x;
    double G[NG], b[NC];
    int n = 0;
#pragma unroll
    for (int a = 0; a < NG; ++a) G[a] = 0.0;
#pragma unroll
    for (int a = 0; a < NC; ++a) b[a] = 0.0;
    const int64_t seg = blockIdx.y;
    const int64_t i0 = seg * A.seg_len, i1 = spc_min64(i0 + A.seg_len, A.nfit);
    for (int64_t i = i0; i < i1; i += ZC) {
        int64_t k[ZC];
        bool ok[ZC], fetch[ZC];
        uint8_t mb[ZC];
        T v[ZC];
        // the channel numbers: entries past the end of the segment repeat its last one (a listed channel; they do not count),
        // so that the loads below need no branch and are all in flight before the first one is waited for
#pragma unroll
        for (int c = 0; c < ZC; ++c) {
            const int64_t e = spc_min64(i + c, i1 - 1);
            const int64_t kk = A.chan ? (int64_t)A.chan[e] : e;
            ok[c] = (i + c < i1) & (kk >= 0) & (kk < A.nz);
            k[c] = kk < 0 ? 0 : spc_min64(kk, A.nz - 1);
        }
#pragma unroll
        for (int c = 0; c < ZC; ++c) {
            mb[c] = 1;
            if (A.m.marr) mb[c] = A.m.marr[k[c] * A.m.mps + moff];
        }
#pragma unroll
        for (int c = 0; c < ZC; ++c) {
            fetch[c] = ok[c] & (mb[c] != 0);                            // mask first: an excluded sample is not fetched
            v[c] = (T)0;
            if (fetch[c]) v[c] = A.in[k[c] * A.ps + off];
        }
#pragma unroll
        for (int c = 0; c < ZC; ++c) {
            double pr[NC];
#pragma unroll
            for (int a = 0; a < NC; ++a) pr[a] = A.basis[k[c] * NC + a];          // uniform address
            const bool inc = fetch[c] & spc_include(A.m, v[c], mb[c]) & (v[c] == v[c]);
            if (inc) {
                const double dv = (double)v[c];
#pragma unroll
                for (int a = 0; a < NC; ++a) {
#pragma unroll
                    for (int bb = a; bb < NC; ++bb) G[bl_tri(a, bb, NC)] = G[bl_tri(a, bb, NC)] + pr[a] * pr[bb];
                }
#pragma unroll
                for (int a = 0; a < NC; ++a) b[a] = b[a] + pr[a] * dv;
                ++n;
            }
        }
    }
    if (A.nseg == 1) {
        bl_store<P>(A.coef, A.npts, A.nspax, s, G, b, n);
        return;
    }
    double* part = A.part + seg * NACC * A.nspax + s;
#pragma unroll
    for (int a = 0; a < NG; ++a) part[a * A.nspax] = G[a];
#pragma unroll
    for (int a = 0; a < NC; ++a) part[(NG + a) * A.nspax] = b[a];
    A.part_n[seg * A.nspax + s] = n;
}

// the partial sums of the segments added in index order, then the solve
template <int P>
__global__ __launch_bounds__(BL_BLOCK) void bl_finish_kernel(const double* part, const int32_t* part_n, int nseg, int64_t nspax,
                                                             double* coef, int32_t* npts) {
    constexpr int NC = P + 1, NG = NC * (NC + 1) / 2, NACC = NG + NC;
    const int64_t s = (int64_t)blockIdx.x * BL_BLOCK + threadIdx.x;
    if (s >= nspax) return;
    double acc[NACC];
    int n = 0;
#pragma unroll
    for (int a = 0; a < NACC; ++a) acc[a] = 0.0;
    for (int g = 0; g < nseg; ++g) {
        const double* p = part + (int64_t)g * NACC * nspax + s;
#pragma unroll
        for (int a = 0; a < NACC; ++a) acc[a] = acc[a] + p[a * nspax];
        n += part_n[(int64_t)g * nspax + s];
    }
    bl_store<P>(coef, npts, nspax, s, acc, acc + NG, n);
}

template <typename T>
struct BlApplyArgs {
    const T* in;
    int64_t nz, nx, rs, ps, nspax;
    const double* basis;
    const double* coef;
    int mode;
    T* out;
    int64_t ors, ops;
};

// blockIdx.x: BL_BLOCK spaxels; blockIdx.y, strided by gridDim.y: batches of BL_ZA channels
template <typename T, int P>
__global__ __launch_bounds__(BL_BLOCK) void bl_apply_kernel(const BlApplyArgs<T> A) {
    constexpr int NC = P + 1;
    const int64_t s = (int64_t)blockIdx.x * BL_BLOCK + threadIdx.x;
    if (s >= A.nspax) return;
    const int64_t y = s / A.nx, x = s - y * A.nx;
    const int64_t off = y * A.rs + x, ooff = y * A.ors + x;
    double c[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) c[j] = A.coef[j * A.nspax + s];
    const int64_t nbatch = (A.nz + BL_ZA - 1) / BL_ZA;
    for (int64_t bt = blockIdx.y; bt < nbatch; bt += gridDim.y) {
        const int64_t z0 = bt * BL_ZA;
        const int nc = (int)spc_min64(BL_ZA, A.nz - z0);
        T v[BL_ZA];
#pragma unroll
        for (int q = 0; q < BL_ZA; ++q) {
            v[q] = (T)0;
            if (A.mode == 0 && q < nc) v[q] = A.in[(z0 + q) * A.ps + off];
        }
#pragma unroll
        for (int q = 0; q < BL_ZA; ++q) {
            if (q >= nc) continue;
            const double* row = A.basis + (z0 + q) * NC;                       // uniform address
            double model = c[0] * row[0];
#pragma unroll
            for (int j = 1; j < NC; ++j) model = model + c[j] * row[j];
            A.out[(z0 + q) * A.ops + ooff] = A.mode ? (T)model : (T)((double)v[q] - model);
        }
    }
}

struct BlSpan { uintptr_t lo, hi; const char* name; };
bool bl_overlap(const BlSpan& a, const BlSpan& b) { return a.lo < b.hi && b.lo < a.hi; }
BlSpan bl_span(const void* p, int64_t elems, size_t size, const char* name) {
    return BlSpan{(uintptr_t)p, (uintptr_t)p + (uintptr_t)elems * size, name};
}
int64_t bl_extent(int64_t nz, int64_t ny, int64_t nx, int64_t rs, int64_t ps) { return (nz - 1) * ps + (ny - 1) * rs + nx; }

// every output against every input and every other output
int bl_check_disjoint(const BlSpan* bufs, int nin, int nall) {
    for (int o = nin; o < nall; ++o) {
        if (bufs[o].lo == 0) continue;
        for (int q = 0; q < nall; ++q) {
            if (q == o || bufs[q].lo == 0) continue;
            SPC_REQUIRE(!bl_overlap(bufs[o], bufs[q]), "%s overlaps %s", bufs[o].name, bufs[q].name);
        }
    }
    return SPC_OK;
}

int bl_check_order(int order) {
    SPC_REQUIRE(order >= 0 && order <= SPC_BASELINE_MAX_ORDER, "order %d is outside 0 ... %d", order, SPC_BASELINE_MAX_ORDER);
    return SPC_OK;
}

size_t bl_workspace(int64_t ny, int64_t nx, int64_t nfit, int order) {
    const int64_t nseg = bl_segments(ny, nx, nfit);
    if (nseg <= 1) return 0;
    const size_t nspax = (size_t)ny * (size_t)nx;
    return spc_ws_round(sizeof(double) * (size_t)nseg * bl_nacc(order) * nspax) + sizeof(int32_t) * (size_t)nseg * nspax;     // what the entry carves
}

template <typename T, int P>
void bl_launch_fit(const BlFitArgs<T>& A, hipStream_t st) {
    const unsigned gx = (unsigned)((A.nspax + BL_BLOCK - 1) / BL_BLOCK);
    hipLaunchKernelGGL((bl_fit_kernel<T, P>), dim3(gx, (unsigned)A.nseg), dim3(BL_BLOCK), 0, st, A);
    if (A.nseg > 1)
        hipLaunchKernelGGL((bl_finish_kernel<P>), dim3(gx), dim3(BL_BLOCK), 0, st, (const double*)A.part, (const int32_t*)A.part_n,
                           A.nseg, A.nspax, A.coef, A.npts);
}

template <typename T, int P>
void bl_launch_apply(const BlApplyArgs<T>& A, hipStream_t st) {
    const int64_t gx = (A.nspax + BL_BLOCK - 1) / BL_BLOCK;
    const int64_t nbatch = (A.nz + BL_ZA - 1) / BL_ZA;
    const int64_t gy = spc_min64(spc_min64(nbatch, BL_GRID_LIMIT), (BL_APPLY_TARGET_BLOCKS + gx - 1) / gx);
    hipLaunchKernelGGL((bl_apply_kernel<T, P>), dim3((unsigned)gx, (unsigned)gy), dim3(BL_BLOCK), 0, st, A);
}

#define BL_BY_ORDER(order, CALL)                                                                   \
    switch (order) {                                                                               \
        case 0: CALL(0); break;                                                                    \
        case 1: CALL(1); break;                                                                    \
        case 2: CALL(2); break;                                                                    \
        case 3: CALL(3); break;                                                                    \
        case 4: CALL(4); break;                                                                    \
        default: CALL(5); break;                                                                   \
    }

template <typename T>
int bl_fit_entry(int device, void* stream, const typename SpcAbi<T>::cube* cube, const typename SpcAbi<T>::mask* mask, int order,
                 const int32_t* d_channels, int64_t nfit, const double* d_basis, double* d_coef, int32_t* d_npts, void* d_workspace,
                 size_t workspace_bytes) {
    int rc = spc_check_cube(cube);
    if (rc) return rc;
    rc = bl_check_order(order);
    if (rc) return rc;
    SPC_REQUIRE(d_basis != nullptr, "d_basis is NULL");
    SPC_REQUIRE(d_coef != nullptr, "d_coef is NULL");
    SPC_REQUIRE(nfit >= 1 && nfit <= (int64_t)0x7fffffff, "nfit %lld is outside 1 ... 2^31 - 1", (long long)nfit);
    SPC_REQUIRE(d_channels != nullptr || nfit == cube->nz, "no channel list: nfit %lld must be nz %lld", (long long)nfit,
                (long long)cube->nz);
    SPC_REQUIRE(cube->nz <= (int64_t)0x7fffffff, "nz %lld does not fit an int32 channel number", (long long)cube->nz);
    BlFitArgs<T> A{};
    rc = spc_include_from(mask, cube, 0, &A.m);
    if (rc) return rc;
    const int64_t nz = cube->nz, ny = cube->ny, nx = cube->nx;
    SPC_REQUIRE(ny <= INT64_MAX / nx && ny * nx <= (int64_t)0x7fffffff * BL_BLOCK, "a plane of %lld x %lld is too large",
                (long long)ny, (long long)nx);
    if (A.m.marr) {
        SPC_REQUIRE(A.m.mrs >= nx, "mask row_stride %lld < nx %lld", (long long)A.m.mrs, (long long)nx);
        SPC_REQUIRE(A.m.mps >= A.m.mrs * (ny - 1) + nx, "mask plane_stride too small");
    }
    A.in = cube->d_data;
    A.nz = nz; A.nx = nx; A.rs = cube->row_stride; A.ps = cube->plane_stride; A.nspax = ny * nx;
    A.chan = d_channels; A.nfit = nfit;
    A.nseg = (int)bl_segments(ny, nx, nfit);
    A.seg_len = (nfit + A.nseg - 1) / A.nseg;
    A.basis = d_basis; A.coef = d_coef; A.npts = d_npts;
    const int nacc = bl_nacc(order);
    SpcWorkspace ws(d_workspace, workspace_bytes);
    if (A.nseg > 1) {
        SPC_WS_TAKE(part, ws, double, (size_t)A.nseg * nacc * (size_t)A.nspax);
        SPC_WS_TAKE(part_n, ws, int32_t, (size_t)A.nseg * (size_t)A.nspax);
        A.part = part; A.part_n = part_n;
    }
    const BlSpan bufs[8] = {
        bl_span(cube->d_data, bl_extent(nz, ny, nx, A.rs, A.ps), sizeof(T), "the cube"),
        bl_span(A.m.marr, A.m.marr ? bl_extent(nz, ny, nx, A.m.mrs, A.m.mps) : 0, 1, "the mask array"),
        bl_span(d_channels, d_channels ? nfit : 0, sizeof(int32_t), "d_channels"),
        bl_span(d_basis, nz * (order + 1), sizeof(double), "d_basis"),
        bl_span(d_coef, (order + 1) * A.nspax, sizeof(double), "d_coef"),
        bl_span(d_npts, d_npts ? A.nspax : 0, sizeof(int32_t), "d_npts"),
        bl_span(A.nseg > 1 ? d_workspace : nullptr, (int64_t)ws.used, 1, "d_workspace"),
        BlSpan{0, 0, ""}};
    rc = bl_check_disjoint(bufs, 4, 7);
    if (rc) return rc;
    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
#define BL_CALL(P) bl_launch_fit<T, P>(A, st)
    BL_BY_ORDER(order, BL_CALL)
#undef BL_CALL
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

template <typename T>
int bl_apply_entry(int device, void* stream, const typename SpcAbi<T>::cube* cube, int order, const double* d_basis, const double* d_coef,
                   int mode, T* d_out, int64_t out_row_stride, int64_t out_plane_stride) {
    int rc = spc_check_cube(cube);
    if (rc) return rc;
    rc = bl_check_order(order);
    if (rc) return rc;
    SPC_REQUIRE(d_basis != nullptr, "d_basis is NULL");
    SPC_REQUIRE(d_coef != nullptr, "d_coef is NULL");
    SPC_REQUIRE(d_out != nullptr, "d_out is NULL");
    SPC_REQUIRE(mode == 0 || mode == 1, "mode %d is neither 0 (subtract) nor 1 (model)", mode);
    const int64_t nz = cube->nz, ny = cube->ny, nx = cube->nx;
    SPC_REQUIRE(ny <= INT64_MAX / nx && ny * nx <= (int64_t)0x7fffffff * BL_BLOCK, "a plane of %lld x %lld is too large",
                (long long)ny, (long long)nx);
    BlApplyArgs<T> A{};
    A.in = cube->d_data;
    A.nz = nz; A.nx = nx; A.rs = cube->row_stride; A.ps = cube->plane_stride; A.nspax = ny * nx;
    A.basis = d_basis; A.coef = d_coef; A.mode = mode;
    A.out = d_out;
    A.ors = out_row_stride ? out_row_stride : nx;
    A.ops = out_plane_stride ? out_plane_stride : A.ors * ny;
    SPC_REQUIRE(A.ors >= nx, "out_row_stride %lld < nx %lld", (long long)A.ors, (long long)nx);
    SPC_REQUIRE(A.ops >= A.ors * (ny - 1) + nx, "out_plane_stride too small");
    const BlSpan bufs[4] = {
        bl_span(cube->d_data, bl_extent(nz, ny, nx, A.rs, A.ps), sizeof(T), "the cube"),
        bl_span(d_basis, nz * (order + 1), sizeof(double), "d_basis"),
        bl_span(d_coef, (order + 1) * A.nspax, sizeof(double), "d_coef"),
        bl_span(d_out, bl_extent(nz, ny, nx, A.ors, A.ops), sizeof(T), "d_out")};
    rc = bl_check_disjoint(bufs, 3, 4);
    if (rc) return rc;
    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
#define BL_CALL(P) bl_launch_apply<T, P>(A, st)
    BL_BY_ORDER(order, BL_CALL)
#undef BL_CALL
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

}  // namespace

extern "C" {

int64_t spc_baseline_segments(int64_t nz, int64_t ny, int64_t nx, int64_t nfit) {
    (void)nz;
    if (ny < 1 || nx < 1 || nfit < 1 || ny > INT64_MAX / nx) return 1;
    return bl_segments(ny, nx, nfit);
}

size_t spc_baseline_workspace_bytes(int64_t nz, int64_t ny, int64_t nx, int64_t nfit, int order) {
    (void)nz;
    if (ny < 1 || nx < 1 || nfit < 1 || ny > INT64_MAX / nx || order < 0 || order > SPC_BASELINE_MAX_ORDER) return 0;
    return bl_workspace(ny, nx, nfit, order);
}

int spc_baseline_fit_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int order,
                         const int32_t* d_channels, int64_t nfit, const double* d_basis, double* d_coef, int32_t* d_npts,
                         void* d_workspace, size_t workspace_bytes) {
    return bl_fit_entry<float>(device, stream, cube, mask, order, d_channels, nfit, d_basis, d_coef, d_npts, d_workspace, workspace_bytes);
}

int spc_baseline_fit_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int order,
                         const int32_t* d_channels, int64_t nfit, const double* d_basis, double* d_coef, int32_t* d_npts,
                         void* d_workspace, size_t workspace_bytes) {
    return bl_fit_entry<double>(device, stream, cube, mask, order, d_channels, nfit, d_basis, d_coef, d_npts, d_workspace, workspace_bytes);
}

int spc_baseline_apply_f32(int device, void* stream, const spc_cube_f32* cube, int order, const double* d_basis,
                           const double* d_coef, int mode, float* d_out, int64_t out_row_stride, int64_t out_plane_stride) {
    return bl_apply_entry<float>(device, stream, cube, order, d_basis, d_coef, mode, d_out, out_row_stride, out_plane_stride);
}

int spc_baseline_apply_f64(int device, void* stream, const spc_cube_f64* cube, int order, const double* d_basis,
                           const double* d_coef, int mode, double* d_out, int64_t out_row_stride, int64_t out_plane_stride) {
    return bl_apply_entry<double>(device, stream, cube, order, d_basis, d_coef, mode, d_out, out_row_stride, out_plane_stride);
}

}  // extern "C"
