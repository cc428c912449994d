// spc_rank_filter.hip - sliding-window rank filters (scipy.ndimage median / minimum / maximum / percentile / rank
// filter) along the spectral axis and per image plane: SpectralCube.spectral_smooth_median / spectral_filter
// (spectral_cube.py:2844-2898, dask_spectral_cube.py:920-960) and spatial_smooth_median / spatial_filter
// (spectral_cube.py:2749-2806, dask_spectral_cube.py:995-1029).
//
// Every sample is loaded once as a FILLED sample (mask predicate and fill fused into the load) and turned into an
// order-preserving unsigned key: sign-flipped IEEE bits as in spc_select_impl.h, except that EVERY NaN (either sign, any
// payload) becomes the largest key.  Selection is done on keys, so "NaN ranks last" (numpy's sort order) costs nothing
// and the result is np.sort(window)[rank] bit for bit (a NaN result is the canonical quiet NaN).
//
//  * spectral, ksize <= RF_NET_MAX: a lane owns 16 bytes of x (4 float32 / 2 float64 spaxels), marches along z with the
//    last ksize keys in registers and sorts a copy with a compile-time merge-exchange network of integer min / max.
//  * spectral, any ksize: a lane owns one spaxel and keeps its SORTED window in LDS (slot-major, so a wave never has a
//    bank conflict); a step is one binary search for the outgoing key and one shifting insert of the incoming one.
//  * spatial: a block stages a 32 x 32 tile plus halo as keys in LDS; 3 x 3 and 5 x 5 windows go through the network,
//    every other footprint through a bitwise descent on the key (one counting sweep of the window per key bit).
//  * mode "constant" with a mask: the reference leaves a spectrum / plane without one included sample unfiltered
//    (_apply_spectral_function / _apply_spatial_function, spectral_cube.py:147-172); a second small kernel finds those
//    and writes them back as fill.  In every other mode the filter of an all-fill ray is all fill anyway.
#include "spc_common.h"

namespace {

constexpr int RF_NET_MAX = 9;             // spectral windows up to this many samples run the register network
constexpr int RF_BLOCK = 256;
constexpr int RF_ZCHUNK = 128;            // outputs per lane and chunk of the network kernel (ksize - 1 halo planes per chunk)
constexpr int RF_TILE = 32;               // spatial tile edge (outputs)
constexpr int RF_LDS_BYTES = 64 * 1024;

// ---- order-preserving keys, NaN last ------------------------------------------------------------------------
template <typename T> struct Key;
template <> struct Key<float> {
    typedef uint32_t K;
    static constexpr int BITS = 32;
    static __host__ __device__ __forceinline__ K to(float v) {
        uint32_t u;
        memcpy(&u, &v, 4);
        const K k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        return v != v ? 0xffffffffu : k;
    }
    static __device__ __forceinline__ float from(K k) {
        return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
    }
};
template <> struct Key<double> {
    typedef uint64_t K;
    static constexpr int BITS = 64;
    static __host__ __device__ __forceinline__ K to(double v) {
        uint64_t u;
        memcpy(&u, &v, 8);
        const K k = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
        return v != v ? ~0ull : k;
    }
    static __device__ __forceinline__ double from(K k) {
        return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
    }
};

enum { RF_REFLECT = 0, RF_CONSTANT = 1, RF_NEAREST = 2, RF_MIRROR = 3, RF_WRAP = 4 };

template <typename T>
struct RfArgs {
    typedef typename Key<T>::K K;
    const T* in;
    int64_t nz, ny, nx, rs, ps;           // input view, strides in elements
    SpcInclude<T> m;                      // which samples count; the others enter as fill
    T fill;
    int mode;
    K ckey;                               // key of cval (mode constant)
    int kz, ky, kx, rank;                 // window (kz spectral; ky, kx spatial) and the rank into it
    T* out;
    int64_t ors, ops;
    int64_t zchunk, nchunks;              // spectral: outputs per lane and chunk
};

// scipy's boundary modes (ni_support.c, NI_ExtendLine): index i of an axis of n samples -> the sample it stands for, -1
// = the constant.  Periodic forms, so any reach is in bounds (the callers refuse more than one axis length anyway).
__device__ __forceinline__ int64_t rf_map(int64_t i, int64_t n, int mode) {
    if (i >= 0 && i < n) return i;
    if (mode == RF_CONSTANT) return -1;
    if (mode == RF_NEAREST) return i < 0 ? 0 : n - 1;
    if (mode == RF_WRAP) { i %= n; return i < 0 ? i + n : i; }
    if (mode == RF_REFLECT) {             // d c b a | a b c d | d c b a
        const int64_t p = 2 * n;
        i %= p; if (i < 0) i += p;
        return i < n ? i : p - 1 - i;
    }
    if (n == 1) return 0;                 // mirror: d c b | a b c d | c b a
    const int64_t p = 2 * n - 2;
    i %= p; if (i < 0) i += p;
    return i < n ? i : p - i;
}

// the filled sample (z, y, x) as a key; all three indices in bounds
template <typename T>
__device__ __forceinline__ typename Key<T>::K rf_key_at(const RfArgs<T>& A, int64_t z, int64_t y, int64_t x) {
    const T v = A.in[z * A.ps + y * A.rs + x];
    const uint8_t mb = A.m.marr ? A.m.marr[z * A.m.mps + y * A.m.mrs + x] : (uint8_t)1;
    return Key<T>::to(spc_include(A.m, v, mb) ? v : A.fill);
}

template <typename K> __device__ __forceinline__ K rf_kmin(K a, K b) { return a < b ? a : b; }
template <typename K> __device__ __forceinline__ K rf_kmax(K a, K b) { return a < b ? b : a; }

// Merge exchange (Knuth, TAOCP 3, 5.2.2 algorithm M): a sorting network for any N, every index a compile-time constant
// once the loops are unrolled (the Makefile's unroll thresholds), so s[] stays in registers.
template <int N, typename K>
__host__ __device__ __forceinline__ void rf_sort_net(K (&s)[N]) {
    if (N < 2) return;
    int t = 0;
    while ((1 << t) < N) ++t;
#pragma unroll
    for (int p = 1 << (t - 1); p > 0; p >>= 1) {
        int q = 1 << (t - 1), r = 0, d = p;
#pragma unroll
        for (int guard = 0; guard < 8; ++guard) {          // (at most t <= 5 rounds per p for N <= 32)
#pragma unroll
            for (int i = 0; i < N - d; ++i) {
                if ((i & p) == r) {
                    const K a = s[i], b = s[i + d];
                    s[i] = a < b ? a : b;
                    s[i + d] = a < b ? b : a;
                }
            }
            if (q == p) break;
            d = q - p;
            q >>= 1;
            r = p;
        }
    }
}

template <int N, typename K>
__device__ __forceinline__ K rf_pick(const K (&s)[N], int rank) {
    K r = s[0];
#pragma unroll
    for (int j = 1; j < N; ++j) r = (rank == j) ? s[j] : r;
    return r;
}

// ---- spectral, network ------------------------------------------------------------------------------------------
// CPL consecutive samples of one row as keys; one 16-byte load (and one CPL-byte mask load) when VEC and all are there
template <typename T, int CPL, bool VEC>
__device__ __forceinline__ void rf_fetch_row(const RfArgs<T>& A, int64_t z, int64_t y, int64_t x0, int nv,
                                             typename Key<T>::K (&k)[CPL]) {
    const int64_t zi = rf_map(z, A.nz, A.mode);
    if (zi < 0) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) k[j] = A.ckey;
        return;
    }
    const T* p = A.in + zi * A.ps + y * A.rs + x0;
    const uint8_t* mp = A.m.marr ? A.m.marr + zi * A.m.mps + y * A.m.mrs + x0 : nullptr;
    T v[CPL];
    uint8_t mb[CPL];
    if (VEC && nv == CPL) {
        struct alignas(16) Pack { T e[CPL]; };
        const Pack q = *reinterpret_cast<const Pack*>(p);
#pragma unroll
        for (int j = 0; j < CPL; ++j) v[j] = q.e[j];
        if (mp) {
            struct alignas(CPL) MPack { uint8_t e[CPL]; };
            const MPack m = *reinterpret_cast<const MPack*>(mp);
#pragma unroll
            for (int j = 0; j < CPL; ++j) mb[j] = m.e[j];
        } else {
#pragma unroll
            for (int j = 0; j < CPL; ++j) mb[j] = 1;
        }
    } else {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            v[j] = j < nv ? p[j] : (T)0;
            mb[j] = (j < nv && mp) ? mp[j] : (uint8_t)1;
        }
    }
#pragma unroll
    for (int j = 0; j < CPL; ++j) k[j] = Key<T>::to(spc_include(A.m, v[j], mb[j]) ? v[j] : A.fill);
}

template <typename T, int W, bool VEC>
__global__ __launch_bounds__(RF_BLOCK) void rf_axis0_net_kernel(const RfArgs<T> A) {
    typedef typename Key<T>::K K;
    constexpr int CPL = 16 / (int)sizeof(T);
    const int64_t x0 = ((int64_t)blockIdx.x * RF_BLOCK + threadIdx.x) * CPL;
    if (x0 >= A.nx) return;
    const int nv = (int)spc_min64(CPL, A.nx - x0);
    const int64_t y = blockIdx.y;
    constexpr int BACK = W / 2;
    for (int64_t c = blockIdx.z; c < A.nchunks; c += gridDim.z) {
        const int64_t z0 = c * A.zchunk, z1 = spc_min64(A.nz, z0 + A.zchunk);
        K ring[W][CPL];                    // ring[j]: window offset j of the current output
#pragma unroll
        for (int j = 1; j < W; ++j) rf_fetch_row<T, CPL, VEC>(A, z0 - BACK + j - 1, y, x0, nv, ring[j]);
        for (int64_t z = z0; z < z1; ++z) {
#pragma unroll
            for (int j = 0; j + 1 < W; ++j) {
#pragma unroll
                for (int e = 0; e < CPL; ++e) ring[j][e] = ring[j + 1][e];
            }
            rf_fetch_row<T, CPL, VEC>(A, z - BACK + W - 1, y, x0, nv, ring[W - 1]);
            T r[CPL];
#pragma unroll
            for (int e = 0; e < CPL; ++e) {
                K s[W];
#pragma unroll
                for (int j = 0; j < W; ++j) s[j] = ring[j][e];
                rf_sort_net<W>(s);
                r[e] = Key<T>::from(rf_pick<W>(s, A.rank));
            }
            T* o = A.out + z * A.ops + y * A.ors + x0;
            if (VEC && nv == CPL) {
                struct alignas(16) Pack { T e[CPL]; };
                Pack q;
#pragma unroll
                for (int e = 0; e < CPL; ++e) q.e[e] = r[e];
                *reinterpret_cast<Pack*>(o) = q;
            } else {
#pragma unroll
                for (int e = 0; e < CPL; ++e) if (e < nv) o[e] = r[e];
            }
        }
    }
}

// ---- spectral, sorted window in LDS ----------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ typename Key<T>::K rf_fetch1(const RfArgs<T>& A, int64_t z, int64_t y, int64_t x) {
    const int64_t zi = rf_map(z, A.nz, A.mode);
    return zi < 0 ? A.ckey : rf_key_at(A, zi, y, x);
}

// NL lanes per block, one spaxel each; S[i * NL + lane] = i-th smallest key of the lane's window
template <typename T, int NL>
__global__ __launch_bounds__(NL) void rf_axis0_sorted_kernel(const RfArgs<T> A) {
    typedef typename Key<T>::K K;
    extern __shared__ __align__(16) unsigned char rf_smem[];
    K* S = reinterpret_cast<K*>(rf_smem) + threadIdx.x;
    const int64_t x = (int64_t)blockIdx.x * NL + threadIdx.x;
    if (x >= A.nx) return;                 // (no barrier below: a lane only touches its own column of S)
    const int64_t y = blockIdx.y;
    const int w = A.kz, back = A.kz / 2;
    for (int64_t c = blockIdx.z; c < A.nchunks; c += gridDim.z) {
        const int64_t z0 = c * A.zchunk, z1 = spc_min64(A.nz, z0 + A.zchunk);
        for (int j = 0; j < w; ++j) {      // insertion sort of the first window
            const K k = rf_fetch1(A, z0 - back + j, y, x);
            int i = j;
            while (i > 0 && S[(i - 1) * NL] > k) { S[i * NL] = S[(i - 1) * NL]; --i; }
            S[i * NL] = k;
        }
        for (int64_t z = z0; z < z1; ++z) {
            A.out[z * A.ops + y * A.ors + x] = Key<T>::from(S[A.rank * NL]);
            if (z + 1 == z1) break;
            const K o = rf_fetch1(A, z - back, y, x), n = rf_fetch1(A, z - back + w, y, x);
            if (n == o) continue;
            int lo = 0, hi = w;            // first slot holding o (it is there: the same load put it in)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (S[mid * NL] < o) lo = mid + 1; else hi = mid;
            }
            int p = lo < w ? lo : w - 1;
            if (n > o) {
                while (p + 1 < w && S[(p + 1) * NL] < n) { S[p * NL] = S[(p + 1) * NL]; ++p; }
            } else {
                while (p > 0 && S[(p - 1) * NL] > n) { S[p * NL] = S[(p - 1) * NL]; --p; }
            }
            S[p * NL] = n;
        }
    }
}

// mode constant with a mask: a spaxel without one included sample is written back as fill (not filtered)
template <typename T>
__global__ __launch_bounds__(RF_BLOCK) void rf_dead_spectra_kernel(const RfArgs<T> A) {
    const int64_t x = (int64_t)blockIdx.x * RF_BLOCK + threadIdx.x;
    if (x >= A.nx) return;
    const int64_t y = blockIdx.y;
    for (int64_t z = 0; z < A.nz; ++z) {
        const T v = A.in[z * A.ps + y * A.rs + x];
        const uint8_t mb = A.m.marr ? A.m.marr[z * A.m.mps + y * A.m.mrs + x] : (uint8_t)1;
        if (spc_include(A.m, v, mb)) return;
    }
    for (int64_t z = 0; z < A.nz; ++z) A.out[z * A.ops + y * A.ors + x] = A.fill;
}

// ---- spatial ---------------------------------------------------------------------------------------------------
// rank-th smallest of the ky x kx keys at tile (ty, tx): greedy descent from the top bit, keeping the largest prefix
// with at most `rank` keys below it
template <typename K, int BITS>
__device__ __forceinline__ K rf_descend(const K* tile, int tw, int ty, int tx, int ky, int kx, int rank) {
    K prefix = 0;
    for (int b = BITS - 1; b >= 0; --b) {
        const K cand = prefix | ((K)1 << b);
        int below = 0;
        for (int j = 0; j < ky; ++j) {
            const K* row = tile + (ty + j) * tw + tx;
            for (int i = 0; i < kx; ++i) below += row[i] < cand ? 1 : 0;
        }
        if (below <= rank) prefix = cand;
    }
    return prefix;
}

// KY, KX > 0: that footprint through the network; 0: any footprint (A.ky, A.kx) through the descent
template <typename T, int KY, int KX>
__global__ __launch_bounds__(RF_BLOCK) void rf_plane_kernel(const RfArgs<T> A) {
    typedef typename Key<T>::K K;
    extern __shared__ __align__(16) unsigned char rf_smem[];
    K* tile = reinterpret_cast<K*>(rf_smem);
    const int ky = KY ? KY : A.ky, kx = KX ? KX : A.kx;
    const int th = RF_TILE + ky - 1, tw = RF_TILE + kx - 1;
    const int64_t by = (int64_t)blockIdx.y * RF_TILE, bx = (int64_t)blockIdx.x * RF_TILE;
    const int tx = threadIdx.x % RF_TILE, ty0 = threadIdx.x / RF_TILE;       // 32 x 8 threads, 4 output rows each
    for (int64_t z = blockIdx.z; z < A.nz; z += gridDim.z) {
        for (int e = threadIdx.x; e < th * tw; e += RF_BLOCK) {
            const int r = e / tw, c = e - r * tw;
            const int64_t sy = rf_map(by + r - ky / 2, A.ny, A.mode), sx = rf_map(bx + c - kx / 2, A.nx, A.mode);
            tile[e] = (sy < 0 || sx < 0) ? A.ckey : rf_key_at(A, z, sy, sx);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < RF_TILE / 8; ++q) {
            const int ty = ty0 + 8 * q;
            const int64_t oy = by + ty, ox = bx + tx;
            if (oy < A.ny && ox < A.nx) {
                K res;
                if constexpr (KY > 0) {
                    K s[KY * KX];
#pragma unroll
                    for (int j = 0; j < KY; ++j) {
#pragma unroll
                        for (int i = 0; i < KX; ++i) s[j * KX + i] = tile[(ty + j) * tw + tx + i];
                    }
                    rf_sort_net<KY * KX>(s);
                    res = rf_pick<KY * KX>(s, A.rank);
                } else {
                    res = rf_descend<K, Key<T>::BITS>(tile, tw, ty, tx, ky, kx, A.rank);
                }
                A.out[z * A.ops + oy * A.ors + ox] = Key<T>::from(res);
            }
        }
        __syncthreads();
    }
}

// mode constant with a mask: a plane without one included sample is written back as fill (not filtered)
template <typename T>
__global__ __launch_bounds__(RF_BLOCK) void rf_dead_planes_kernel(const RfArgs<T> A) {
    const int64_t n = A.ny * A.nx;
    for (int64_t z = blockIdx.x; z < A.nz; z += gridDim.x) {
        int found = 0;
        for (int64_t e0 = 0; e0 < n && !found; e0 += RF_BLOCK) {           // (found is block-uniform: every lane leaves together)
            const int64_t e = e0 + threadIdx.x;
            int mine = 0;
            if (e < n) {
                const int64_t y = e / A.nx, x = e - y * A.nx;
                const T v = A.in[z * A.ps + y * A.rs + x];
                const uint8_t mb = A.m.marr ? A.m.marr[z * A.m.mps + y * A.m.mrs + x] : (uint8_t)1;
                mine = spc_include(A.m, v, mb) ? 1 : 0;
            }
            found = __syncthreads_or(mine);
        }
        if (found) continue;
        for (int64_t e = threadIdx.x; e < n; e += RF_BLOCK) {
            const int64_t y = e / A.nx, x = e - y * A.nx;
            A.out[z * A.ops + y * A.ors + x] = A.fill;
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------
template <typename T>
bool rf_vec_ok(const RfArgs<T>& A) {
    const size_t e = sizeof(T), cpl = 16 / sizeof(T);
    bool ok = spc_aligned(A.in, 16) && (A.rs * e) % 16 == 0 && (A.ps * e) % 16 == 0;
    ok = ok && spc_aligned(A.out, 16) && (A.ors * e) % 16 == 0 && (A.ops * e) % 16 == 0;
    if (A.m.marr) ok = ok && spc_aligned(A.m.marr, cpl) && A.m.mrs % cpl == 0 && A.m.mps % cpl == 0;
    return ok;
}

template <typename T, bool VEC>
void rf_launch_net(const RfArgs<T>& A, dim3 grid, hipStream_t st) {
    switch (A.kz) {
#define RF_CASE(W) case W: hipLaunchKernelGGL((rf_axis0_net_kernel<T, W, VEC>), grid, dim3(RF_BLOCK), 0, st, A); break;
        RF_CASE(1) RF_CASE(2) RF_CASE(3) RF_CASE(4) RF_CASE(5) RF_CASE(6) RF_CASE(7) RF_CASE(8) RF_CASE(9)
#undef RF_CASE
        default: break;
    }
}

// rows of at most 65535 per launch (gridDim.y); row offsets keep every alignment rf_vec_ok checked
template <typename T>
RfArgs<T> rf_row_slab(const RfArgs<T>& A, int64_t r0, int64_t n) {
    RfArgs<T> S = A;
    S.in = A.in + r0 * A.rs;
    if (S.m.marr) S.m.marr = A.m.marr + r0 * A.m.mrs;
    S.out = A.out + r0 * A.ors;
    S.ny = n;
    return S;
}

template <typename T>
int rf_run_axis0(int device, void* stream, RfArgs<T> A) {
    typedef typename Key<T>::K K;
    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const bool net = A.kz <= RF_NET_MAX;
    const bool vec = rf_vec_ok(A);
    // the sorted window: 64 lanes per block, 32 when 64 columns of kz keys pass 64 KB of LDS
    const int nl = (size_t)A.kz * sizeof(K) * 64 <= (size_t)RF_LDS_BYTES ? 64 : 32;
    SPC_REQUIRE((size_t)A.kz * sizeof(K) * nl <= (size_t)RF_LDS_BYTES, "ksize %d is above the built limit of %d", A.kz,
                SPC_RANK_FILTER_MAX_KSIZE);
    A.zchunk = net ? RF_ZCHUNK : (A.kz * 8 > 256 ? A.kz * 8 : 256);
    A.nchunks = (A.nz + A.zchunk - 1) / A.zchunk;
    const unsigned gz = (unsigned)spc_min64(A.nchunks, 65535);
    const bool dead = A.mode == RF_CONSTANT && (A.m.marr || A.m.pred || A.m.nan_excluded);
    for (int64_t r0 = 0; r0 < A.ny; r0 += 65535) {
        const RfArgs<T> S = rf_row_slab(A, r0, spc_min64(65535, A.ny - r0));
        if (net) {
            const int64_t cpl = 16 / sizeof(T), lanes = (S.nx + cpl - 1) / cpl;
            dim3 grid((unsigned)((lanes + RF_BLOCK - 1) / RF_BLOCK), (unsigned)S.ny, gz);
            if (vec) rf_launch_net<T, true>(S, grid, st);
            else rf_launch_net<T, false>(S, grid, st);
        } else {
            dim3 grid((unsigned)((S.nx + nl - 1) / nl), (unsigned)S.ny, gz);
            const size_t lds = (size_t)S.kz * sizeof(K) * nl;
            if (nl == 64) hipLaunchKernelGGL((rf_axis0_sorted_kernel<T, 64>), grid, dim3(64), lds, st, S);
            else hipLaunchKernelGGL((rf_axis0_sorted_kernel<T, 32>), grid, dim3(32), lds, st, S);
        }
        SPC_LAUNCH_CHECK();
        if (dead) {
            dim3 grid((unsigned)((S.nx + RF_BLOCK - 1) / RF_BLOCK), (unsigned)S.ny);
            hipLaunchKernelGGL((rf_dead_spectra_kernel<T>), grid, dim3(RF_BLOCK), 0, st, S);
            SPC_LAUNCH_CHECK();
        }
    }
    return SPC_OK;
}

template <typename T>
int rf_run_plane(int device, void* stream, const RfArgs<T>& A) {
    typedef typename Key<T>::K K;
    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const int64_t gy = (A.ny + RF_TILE - 1) / RF_TILE, gx = (A.nx + RF_TILE - 1) / RF_TILE;
    SPC_REQUIRE(gy <= 65535 && gx <= 0x7fffffff, "plane of %lld x %lld is too large", (long long)A.ny, (long long)A.nx);
    dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)spc_min64(A.nz, 65535));
    const size_t lds = (size_t)(RF_TILE + A.ky - 1) * (RF_TILE + A.kx - 1) * sizeof(K);
    if (A.ky == 3 && A.kx == 3) hipLaunchKernelGGL((rf_plane_kernel<T, 3, 3>), grid, dim3(RF_BLOCK), lds, st, A);
    else if (A.ky == 5 && A.kx == 5) hipLaunchKernelGGL((rf_plane_kernel<T, 5, 5>), grid, dim3(RF_BLOCK), lds, st, A);
    else hipLaunchKernelGGL((rf_plane_kernel<T, 0, 0>), grid, dim3(RF_BLOCK), lds, st, A);
    SPC_LAUNCH_CHECK();
    if (A.mode == RF_CONSTANT && (A.m.marr || A.m.pred || A.m.nan_excluded)) {
        hipLaunchKernelGGL((rf_dead_planes_kernel<T>), dim3((unsigned)spc_min64(A.nz, 65535)), dim3(RF_BLOCK), 0, st, A);
        SPC_LAUNCH_CHECK();
    }
    return SPC_OK;
}

// argument checks and the geometry both sample types share; window = kz (ky = kx = 0) or ky x kx (kz = 0)
template <typename T>
int rf_setup(RfArgs<T>& A, int kz, int ky, int kx, int rank, int mode, T cval, T* d_out, int64_t ors, int64_t ops) {
    SPC_REQUIRE(d_out != nullptr, "d_out is NULL");
    SPC_REQUIRE((const void*)d_out != (const void*)A.in, "the rank filter does not run in place");
    SPC_REQUIRE(mode >= RF_REFLECT && mode <= RF_WRAP, "unknown boundary mode %d", mode);
    int64_t w;
    if (kz) {
        SPC_REQUIRE(kz >= 1 && kz <= SPC_RANK_FILTER_MAX_KSIZE, "ksize must be 1 ... %d (got %d)", SPC_RANK_FILTER_MAX_KSIZE, kz);
        SPC_REQUIRE(kz / 2 <= A.nz, "ksize %d reaches more than one axis length (%lld) past the edge", kz, (long long)A.nz);
        w = kz;
    } else {
        SPC_REQUIRE(ky >= 1 && ky <= SPC_RANK_FILTER_MAX_KSIZE_SPATIAL && kx >= 1 && kx <= SPC_RANK_FILTER_MAX_KSIZE_SPATIAL,
                    "spatial ksize must be 1 ... %d per axis (got %d x %d)", SPC_RANK_FILTER_MAX_KSIZE_SPATIAL, ky, kx);
        SPC_REQUIRE(ky / 2 <= A.ny && kx / 2 <= A.nx, "ksize %d x %d reaches more than one axis length (%lld x %lld) past the edge",
                    ky, kx, (long long)A.ny, (long long)A.nx);
        w = (int64_t)ky * kx;
    }
    SPC_REQUIRE(rank >= 0 && rank < w, "rank %d outside the window of %lld samples", rank, (long long)w);
    A.kz = kz; A.ky = ky; A.kx = kx; A.rank = rank; A.mode = mode;
    A.ckey = Key<T>::to(cval);
    A.out = d_out;
    A.ors = ors ? ors : A.nx;
    A.ops = ops ? ops : A.ny * A.ors;
    SPC_REQUIRE(A.ors >= A.nx && A.ops >= A.ors * (A.ny - 1) + A.nx, "output strides too small");
    A.zchunk = A.nz; A.nchunks = 1;
    return SPC_OK;
}

template <typename T>
int rf_args(const typename SpcAbi<T>::cube* cube, const typename SpcAbi<T>::mask* mask, int nan_excluded, T fill, RfArgs<T>* A) {
    int rc = sizeof(T) == 8 ? spc_check_cube_any_order_words(cube) : spc_check_cube(cube);
    if (rc) return rc;
    rc = spc_include_from(mask, cube, nan_excluded, &A->m);
    if (rc) return rc;
    A->in = cube->d_data; A->nz = cube->nz; A->ny = cube->ny; A->nx = cube->nx;
    A->rs = cube->row_stride; A->ps = cube->plane_stride;
    A->fill = fill;
    return SPC_OK;
}

template <typename T>
int rf_axis0_entry(int device, void* stream, const typename SpcAbi<T>::cube* cube, const typename SpcAbi<T>::mask* mask, int nan_excluded,
                   T fill, int ksize, int rank, int mode, T cval, T* d_out, int64_t out_row_stride, int64_t out_plane_stride) {
    RfArgs<T> A{};
    int rc = rf_args<T>(cube, mask, nan_excluded, fill, &A);
    if (rc) return rc;
    SPC_REQUIRE(ksize != 0, "ksize must be 1 ... %d (got 0)", SPC_RANK_FILTER_MAX_KSIZE);
    rc = rf_setup(A, ksize, 0, 0, rank, mode, cval, d_out, out_row_stride, out_plane_stride);
    if (rc) return rc;
    return rf_run_axis0(device, stream, A);
}

template <typename T>
int rf_plane_entry(int device, void* stream, const typename SpcAbi<T>::cube* cube, const typename SpcAbi<T>::mask* mask, int nan_excluded,
                   T fill, int ky, int kx, int rank, int mode, T cval, T* d_out, int64_t out_row_stride, int64_t out_plane_stride) {
    RfArgs<T> A{};
    int rc = rf_args<T>(cube, mask, nan_excluded, fill, &A);
    if (rc) return rc;
    rc = rf_setup(A, 0, ky, kx, rank, mode, cval, d_out, out_row_stride, out_plane_stride);
    if (rc) return rc;
    return rf_run_plane(device, stream, A);
}

}  // namespace

extern "C" {

int spc_rank_filter_axis0_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded,
                              float fill, int ksize, int rank, int mode, float cval,
                              float* d_out, int64_t out_row_stride, int64_t out_plane_stride) {
    return rf_axis0_entry<float>(device, stream, cube, mask, nan_excluded, fill, ksize, rank, mode, cval, d_out, out_row_stride, out_plane_stride);
}

int spc_rank_filter_axis0_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded,
                              double fill, int ksize, int rank, int mode, double cval,
                              double* d_out, int64_t out_row_stride, int64_t out_plane_stride) {
    return rf_axis0_entry<double>(device, stream, cube, mask, nan_excluded, fill, ksize, rank, mode, cval, d_out, out_row_stride, out_plane_stride);
}

int spc_rank_filter_plane_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded,
                              float fill, int ky, int kx, int rank, int mode, float cval,
                              float* d_out, int64_t out_row_stride, int64_t out_plane_stride) {
    return rf_plane_entry<float>(device, stream, cube, mask, nan_excluded, fill, ky, kx, rank, mode, cval, d_out, out_row_stride, out_plane_stride);
}

int spc_rank_filter_plane_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded,
                              double fill, int ky, int kx, int rank, int mode, double cval,
                              double* d_out, int64_t out_row_stride, int64_t out_plane_stride) {
    return rf_plane_entry<double>(device, stream, cube, mask, nan_excluded, fill, ky, kx, rank, mode, cval, d_out, out_row_stride, out_plane_stride);
}

}  // extern "C"
