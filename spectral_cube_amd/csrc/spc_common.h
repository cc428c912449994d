// Internal helpers shared by the HIP translation units of libspcube_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <cmath>
#include <limits>
#include "../../include/spcube_hip.h"

void spc_set_error(const char* fmt, ...);

// ---- the SPC_* switches of the process environment: the one place that reads them ----------------------------
// docs/DESIGN_NOTES.md lists every switch with its default and when it is read.  spc_switch: atoi of the value when
// the variable is set ("" and text that is no number give 0), dflt when it is not.  A site that only asks whether a
// variable is set passes a default that no valid value takes: spc_switch(name, -1) != -1.  A site that reads once
// per process keeps the result in a static of its own; everything else reads per call, because the tests flip
// switches inside one process.
static inline const char* spc_switch_text(const char* name) { return getenv(name); }     // SPC_POOL_MAX_BYTES only: 64 bits
static inline int spc_switch(const char* name, int dflt) {
    const char* e = spc_switch_text(name);
    return e ? atoi(e) : dflt;
}

#define SPC_HIP(call)                                                         \
    do {                                                                      \
        hipError_t e_ = (call);                                               \
        if (e_ != hipSuccess) {                                               \
            spc_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                          __FILE__, __LINE__);                                \
            return SPC_ERR_HIP;                                               \
        }                                                                     \
    } while (0)

#define SPC_REQUIRE(cond, ...)                                                \
    do {                                                                      \
        if (!(cond)) {                                                        \
            spc_set_error(__VA_ARGS__);                                       \
            return SPC_ERR_INVALID;                                           \
        }                                                                     \
    } while (0)

#define SPC_LAUNCH_CHECK()                                                    \
    do {                                                                      \
        hipError_t e_ = hipGetLastError();                                    \
        if (e_ != hipSuccess) {                                               \
            spc_set_error("kernel launch failed: %s (%s:%d)",                 \
                          hipGetErrorString(e_), __FILE__, __LINE__);         \
            return SPC_ERR_HIP;                                               \
        }                                                                     \
    } while (0)

// RAII "current device" switch so concurrent host threads on different GPUs
// do not disturb each other (hipSetDevice is per-thread).
struct SpcDeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit SpcDeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = (hipSetDevice(dev) == hipSuccess);
        // the runtime keeps a thread's last error until it is read: one left by an earlier call - this hipSetDevice on a device
        // the machine does not have, a refused allocation - would otherwise be reported by the NEXT entry's SPC_LAUNCH_CHECK as
        // a failed launch of its own.  Every entry that launches switches the device first, so it starts from a clean state here.
        (void)hipGetLastError();
    }
    ~SpcDeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

#define SPC_DEVICE(dev)                                                       \
    SpcDeviceGuard guard_(dev);                                               \
    if (!guard_.ok) {                                                         \
        spc_set_error("hipSetDevice(%d) failed", dev);                        \
        return SPC_ERR_HIP;                                                   \
    }

// ---- caller-owned device scratch -------------------------------------------------------------
// No entry point allocates, frees or drains: whatever scratch a call needs (tile flags, partial
// records, weight tables, intermediate (num, den) planes) is carved out of the d_workspace the
// caller passes in - spc_workspace_bytes() says how much - and everything is queued on the
// caller's stream, so calls on different streams overlap and a stream of calls never blocks the
// host except where a result has to come back to it (documented per entry point).
struct SpcWorkspace {
    char* base;
    size_t size, used;
    SpcWorkspace(void* p, size_t n) : base((char*)p), size(p ? n : 0), used(0) {}
    // 256-byte aligned slices; nullptr when the workspace is too small
    void* take(size_t bytes) {
        const size_t at = (used + 255) & ~(size_t)255;
        if (!base || at + bytes > size) { used = at + bytes; return nullptr; }
        used = at + bytes;
        return base + at;
    }
};
static inline size_t spc_ws_round(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

#define SPC_WS_TAKE(var, ws, type, count)                                                          \
    type* var = (type*)(ws).take(sizeof(type) * (size_t)(count));                                   \
    if (!var) {                                                                                    \
        spc_set_error("d_workspace too small: this call needs at least %zu bytes (spc_workspace_bytes)", \
                      (ws).used);                                                                  \
        return SPC_ERR_INVALID;                                                                    \
    }

// A small host table (kernel taps, per-channel weights) -> device memory by kernel launches only:
// the bytes travel as kernel arguments, so the host buffer may die when the call returns and nothing
// synchronises (a hipMemcpyAsync from pageable memory would need the buffer kept alive or a wait).
hipError_t spc_table_upload(void* d_dst, const void* h_src, size_t bytes, hipStream_t st);

// per-entry-point scratch sizes (defined next to the entry points, dispatched by spc_workspace_bytes)
size_t spc_ws_spectral_conv(int64_t nz, int64_t ny, int64_t nx, int64_t ntaps, bool fused);
size_t spc_ws_spatial_conv_sep(int64_t nz, int64_t ny, int64_t nx, int64_t nky, int64_t nkx);
size_t spc_ws_spatial_conv2d(int64_t nz, int64_t ny, int64_t nx, int64_t nky, int64_t nkx);
size_t spc_ws_resample_bilinear(int64_t ny_out, int64_t nx_out);
size_t spc_ws_resample_bilinear_lerp(int64_t nz, int64_t ny_out, int64_t nx_out);
size_t spc_ws_stats(int kind, int64_t nz, int64_t ny, int64_t nx, int64_t p0, int64_t p1);
size_t spc_ws_percentile_global(void);
size_t spc_ws_sigma_clip(void);
size_t spc_ws_stats_global_f64(void);
size_t spc_ws_spectral_conv_f64(int64_t ntaps);
size_t spc_ws_spatial_conv_f64(int64_t nz, int64_t ny, int64_t nx, int64_t nky, int64_t nkx);
size_t spc_ws_spatial_conv_mfma(int64_t nz, int64_t ny, int64_t nx, int64_t nsum);
int spc_spatial_conv_split_store(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, const double* h_ky, int nky,
                                 const double* h_kx, int nkx, float* d_out, int64_t out_row_stride, int64_t out_plane_stride);

// ---- tile flags handed from a speculative kernel to the kernel that redoes flagged tiles -----
// Producer and consumer are queued back to back on one stream; the kernel boundary orders them.
__device__ __forceinline__ void spc_flag_set(unsigned char* p) { *reinterpret_cast<volatile unsigned char*>(p) = 1; }
__device__ __forceinline__ unsigned char spc_flag_get(const unsigned char* p) {
    return *reinterpret_cast<const volatile unsigned char*>(p);
}
static inline hipError_t spc_flags_clear(unsigned char* d_flags, size_t n, hipStream_t st) {
    return n ? hipMemsetAsync(d_flags, 0, n, st) : hipSuccess;
}

// ---- the mask of a cube on the device, float32 or float64 ----------------------------------------------------
// One layer for both sample types: T = float goes with (spc_cube_f32, spc_mask), T = double with (spc_cube_f64,
// spc_mask_f64), whose thresholds stay float64 (numpy compares a float64 cube in float64, spectral_cube/masks.py:225).
template <typename T> struct SpcAbi;
template <> struct SpcAbi<float> { typedef spc_cube_f32 cube; typedef spc_mask mask; };
template <> struct SpcAbi<double> { typedef spc_cube_f64 cube; typedef spc_mask_f64 mask; };

__host__ __device__ __forceinline__ float spc_abs(float v) { return fabsf(v); }
__host__ __device__ __forceinline__ double spc_abs(double v) { return fabs(v); }
__host__ __device__ __forceinline__ int64_t spc_min64(int64_t a, int64_t b) { return a < b ? a : b; }
static inline bool spc_aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

// mask predicate -> |v| <= lim && !(v <= lo) && !(v >= hi): three compares whatever the flags.  An absent bound is
// NaN (the negated compare is then true for every v), >= / <= become strict compares against the neighbouring float,
// a NaN threshold rejects everything (numpy: x > nan is False); lim = FLT_MAX / DBL_MAX under isfinite, +inf otherwise
// (NaN samples fail |v| <= lim either way: they are never valid).
template <typename T>
static inline void spc_canonical_pred(uint32_t f, T thr_lo, T thr_hi, T* lim, T* lo, T* hi) {
    const T inf = std::numeric_limits<T>::infinity();
    *lim = (f & SPC_MASK_FINITE) ? std::numeric_limits<T>::max() : inf;
    *lo = (T)NAN;
    *hi = (T)NAN;
    if (f & (SPC_MASK_GT | SPC_MASK_GE)) {
        if (thr_lo != thr_lo) *lim = (T)-1;
        else if (f & SPC_MASK_GT) *lo = thr_lo;
        else *lo = (thr_lo == -inf) ? (T)NAN : std::nextafter(thr_lo, -inf);
    }
    if (f & (SPC_MASK_LT | SPC_MASK_LE)) {
        if (thr_hi != thr_hi) *lim = (T)-1;
        else if (f & SPC_MASK_LT) *hi = thr_hi;
        else *hi = (thr_hi == inf) ? (T)NAN : std::nextafter(thr_hi, inf);
    }
}

template <typename T>
struct SpcMaskDev {
    uint32_t flags;
    T thr_lo, thr_hi;
    const uint8_t* arr;
    int64_t row_stride, plane_stride;
    T lim, lo, hi;               // the predicate terms in canonical form (spc_canonical_pred), set by spc_mask_to_dev
};
using MaskDev = SpcMaskDev<float>;
using MaskDev64 = SpcMaskDev<double>;

template <typename T>
static inline int spc_mask_to_dev(const typename SpcAbi<T>::mask* m, const typename SpcAbi<T>::cube* c, SpcMaskDev<T>* out) {
    out->flags = 0; out->thr_lo = 0; out->thr_hi = 0; out->arr = nullptr;
    out->row_stride = c->row_stride; out->plane_stride = c->plane_stride;
    spc_canonical_pred<T>(0u, 0, 0, &out->lim, &out->lo, &out->hi);
    if (!m) return SPC_OK;
    out->flags = m->flags; out->thr_lo = m->thr_lo; out->thr_hi = m->thr_hi;
    spc_canonical_pred<T>(m->flags, m->thr_lo, m->thr_hi, &out->lim, &out->lo, &out->hi);
    if (m->flags & SPC_MASK_ARRAY) {
        SPC_REQUIRE(m->d_array != nullptr, "SPC_MASK_ARRAY set but d_array is NULL");
        out->arr = m->d_array;
        if (m->row_stride) out->row_stride = m->row_stride;
        if (m->plane_stride) out->plane_stride = m->plane_stride;
    }
    SPC_REQUIRE((m->flags & ~63u) == 0, "unknown mask flags 0x%x", m->flags);
    return SPC_OK;
}

// C: spc_cube_f32 or spc_cube_f64
template <typename C>
static inline int spc_check_cube(const C* c) {
    SPC_REQUIRE(c != nullptr && c->d_data != nullptr, "cube pointer is NULL");
    SPC_REQUIRE(c->nz > 0 && c->ny > 0 && c->nx > 0, "cube shape must be positive (got %lld,%lld,%lld)",
                (long long)c->nz, (long long)c->ny, (long long)c->nx);
    SPC_REQUIRE(c->row_stride >= c->nx, "row_stride %lld < nx %lld", (long long)c->row_stride, (long long)c->nx);
    SPC_REQUIRE(c->plane_stride >= c->row_stride * (c->ny - 1) + c->nx, "plane_stride too small");
    return SPC_OK;
}

// for kernels that only ever form z * plane_stride + y * row_stride + x: also accepts a view whose
// first two axes are exchanged (row_stride > plane_stride), e.g. selection along y instead of z
template <typename C>
static inline int spc_check_cube_any_order(const C* c) {
    SPC_REQUIRE(c != nullptr && c->d_data != nullptr, "cube pointer is NULL");
    SPC_REQUIRE(c->nz > 0 && c->ny > 0 && c->nx > 0, "cube shape must be positive (got %lld,%lld,%lld)",
                (long long)c->nz, (long long)c->ny, (long long)c->nx);
    SPC_REQUIRE(c->row_stride >= c->nx && c->plane_stride >= c->nx, "row / plane stride smaller than nx");
    SPC_REQUIRE(c->plane_stride >= c->row_stride * (c->ny - 1) + c->nx ||
                c->row_stride >= c->plane_stride * (c->nz - 1) + c->nx, "overlapping rows and planes");
    return SPC_OK;
}

// The views spc_check_cube accepts, refused in the words the float64 rank filter and stack have always used (those of
// spc_check_cube_any_order, then the plane stride): kept so that no message moves; nothing else should call it.
template <typename C>
static inline int spc_check_cube_any_order_words(const C* c) {
    const int rc = spc_check_cube_any_order(c);
    if (rc) return rc;
    SPC_REQUIRE(c->plane_stride >= c->row_stride * (c->ny - 1) + c->nx, "plane_stride too small");
    return SPC_OK;
}

// the float64 moment kernel packs a count and two z indices into 21 bits each; cube64_args (spc_wide.h) hands its bound
// to every float64 operator that takes a cube in spectral order.  Called after the cube check proper
static inline int spc_check_nz_f64(const spc_cube_f64* c) {
    SPC_REQUIRE(c->nz < (1LL << 21), "nz too large for the float64 moment kernel (%lld)", (long long)c->nz);
    return SPC_OK;
}

// ---- "is this voxel included": the mask as the operators with a fill value see it -----------------------------
// A two-width operator embeds one SpcInclude<T> in its kernel arguments, fills it with spc_include_from and asks
// spc_include for every sample it loads (mb = the sample's byte of the mask array, 1 without one).
template <typename T>
struct SpcInclude {
    const uint8_t* marr;                  // mask array term, or nullptr
    int64_t mrs, mps;
    T lim, lo, hi;                        // predicate terms in canonical form (spc_canonical_pred)
    int pred;                             // any predicate flag set: otherwise a NaN sample is included (array term only)
    int nan_excluded;                     // a NaN sample is excluded whatever the terms say (a ~isnan mask of the cube's data)
};

template <typename T>
__device__ __forceinline__ bool spc_include(const SpcInclude<T>& I, T v, uint8_t mb) {
    const bool p = (spc_abs(v) <= I.lim) & !(v <= I.lo) & !(v >= I.hi);
    return (mb != 0) & (!I.pred | p) & (!I.nan_excluded | (v == v));
}

template <typename T>
static inline int spc_include_from(const typename SpcAbi<T>::mask* mask, const typename SpcAbi<T>::cube* cube, int nan_excluded,
                                   SpcInclude<T>* out) {
    SpcMaskDev<T> M;
    const int rc = spc_mask_to_dev(mask, cube, &M);
    if (rc) return rc;
    out->marr = (M.flags & SPC_MASK_ARRAY) ? M.arr : nullptr;
    out->mrs = M.row_stride; out->mps = M.plane_stride;
    out->lim = M.lim; out->lo = M.lo; out->hi = M.hi;
    out->pred = (M.flags & ~SPC_MASK_ARRAY) != 0;
    out->nan_excluded = nan_excluded != 0;
    return SPC_OK;
}

// Buffer descriptor over (up to 4 GiB from) a wave-uniform base.  The base must be provably uniform, otherwise hipcc wraps
// every buffer op in a waterfall loop: both halves go through readfirstlane.
__device__ __forceinline__ auto spc_plane_srd(const void* base) {
    const unsigned long long a = (unsigned long long)base;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), 0, (int)0xffffffffu, 0x00020000);
}

// predicate part of the mask AND "not NaN", in the canonical form: three compares and no flag tests (spc_pred below costs five
// flag-guarded compares and ~11 scalar instructions per sample whatever the mask: round 4 found the reductions bound by that)
template <typename T>
__device__ __forceinline__ bool spc_pred_valid(const SpcMaskDev<T>& m, T v) {
    return (spc_abs(v) <= m.lim) & !(v <= m.lo) & !(v >= m.hi);
}

// predicate part of the mask (array part is handled by the caller's loads); a NaN sample passes unless isfinite is asked for
__device__ __forceinline__ bool spc_pred(uint32_t flags, float thr_lo, float thr_hi, float v) {
    bool inc = true;
    if (flags & SPC_MASK_FINITE) inc = inc && (fabsf(v) <= 3.402823466e+38f);  // false for NaN/inf
    if (flags & SPC_MASK_GT) inc = inc && (v > thr_lo);
    if (flags & SPC_MASK_GE) inc = inc && (v >= thr_lo);
    if (flags & SPC_MASK_LT) inc = inc && (v < thr_hi);
    if (flags & SPC_MASK_LE) inc = inc && (v <= thr_hi);
    return inc;
}
