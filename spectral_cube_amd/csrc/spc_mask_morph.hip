// spc_mask_morph.hip - binary morphology of a uint8 include array: erosion, dilation, and either one repeated to its
// fixed point (scipy.ndimage.binary_erosion / binary_dilation / binary_propagation on cube.get_mask_array(),
// spectral_cube.py:552, which users of the reference run on the host).
//
// Rules (include/spcube_hip.h), for the offsets o of the structuring element and samples outside the array = border:
//     dilation r[p] = OR over o of in[p - o],  erosion r[p] = AND over o of in[p + o],  out[p] = mask[p] ? r[p] : in[p],
// `iterations` synchronous steps, or steps until nothing changes.  The numpy restatement of these rules (tests/
// morphology.py) equals scipy.ndimage 1.15 on every case of its table - asymmetric and hollow structures, even extents,
// border_value 1, erosion under a mask, structures taller than the axis: no difference was found.  (scipy's own default
// path, the one that tracks changed voxels, corrupts its heap when iterations != 1 and a structure is larger than the
// array; its brute_force=True path is the reference there.)
//
// Layout.  Voxels are packed to one bit each, 32 consecutive x to a uint32 word (bit i of word w = x 32 w + i), rows
// padded to a word: W = ceil(nx / 32) words a row, (nz, ny, W) words in all - 1/8 of the uint8 array.  The workspace
// holds two packed buffers and the packed mask.  An x offset is a shift with a carry from the neighbouring word, a y / z
// offset a whole-word OR with another row; the host groups the offsets by (dz, dy), one 7-bit set of dx each, so every
// source row is loaded once per output word.  The padding bits of a row always hold the border value, the words outside
// the array are the border word: nothing else is needed for the edges.
// Only dilation is built: erosion runs as its dual - the complement is packed (mm_pack_kernel flips the bits), dilated
// with the reflected offsets and the complemented border under the same mask, and complemented again when the bytes are
// written.  ~out = mask ? ~r : ~in has the same form as the rule above, so this is exact for every step, not only at
// the fixed point.
//
// Fixed number of steps, and repetition of a structure WITHOUT its centre: synchronous steps between the two buffers
// (mm_step_kernel).  Without the centre a step is not extensive, the sequence need not be monotone and may cycle (in
// scipy for ever): the steps end with SPC_ERR_UNSUPPORTED after MM_STEP_LIMIT of them.
// Repetition of a structure WITH its centre (binary_propagation, and iterations < 1 in general): every step only adds
// voxels, X <= F(X) with F(X) = mask ? D(X) : X monotone, so the synchronous sequence climbs to the LEAST fixed point of F
// above the input.  Any order of updates reaches the same set: a state made of updates S |= part of F(S) stays between
// the input and that fixed point (induction: F(S) <= F(lfp) = lfp), and a state no update changes is a fixed point above
// the input, hence >= lfp.  So the sweeps run in place on ONE buffer (mm_settle_kernel): a block loads its tile and a
// halo as deep as the structure reaches into LDS, repeats the step on the tile until the tile is settled, and stores the
// words that changed.  A block may read a neighbour's words before or after that neighbour's stores of the same sweep:
// either value is a state of the kind above (a word is stored whole).  A sweep in which no block stores anything saw the
// memory the sweep before left (kernel boundary) and found every tile settled against it: the fixed point.  Erosion to
// its fixed point takes the same route through the dual: it IS a dilation of the complement, the argument is this one.
// The host reads the change words (MM_BATCH x 4 bytes) after every batch of MM_BATCH sweeps: the one synchronisation.
#include "spc_common.h"

namespace {

constexpr int MM_BLOCK = 256;
constexpr int MM_R = SPC_MORPH_MAX_REACH;
constexpr int MM_NGROUPS = (2 * MM_R + 1) * (2 * MM_R + 1);           // one group per (dz, dy)
constexpr int MM_TZ = 8, MM_TY = 16, MM_TW = 8;                       // the tile of mm_settle_kernel: planes, rows, words
constexpr int MM_LW = MM_TW + 2;                                      // with one halo word at either end of a row
constexpr int MM_LDS_WORDS = (MM_TZ + 2 * MM_R) * (MM_TY + 2 * MM_R) * MM_LW;      // 12320 bytes
constexpr int MM_PER_THREAD = MM_TZ * MM_TY * MM_TW / MM_BLOCK;
constexpr int64_t MM_MAX_BLOCKS = 1 << 20;                            // grid-stride loops beyond
constexpr int MM_BATCH = 4;                                           // sweeps / steps per read of the change words
constexpr int64_t MM_STEP_LIMIT = 65536;                              // repeated steps of a structure without its centre
static_assert(MM_TZ * MM_TY * MM_TW % MM_BLOCK == 0, "whole words per thread");
static_assert(MM_R == 3, "the dx set of a group is 7 bits, bit dx + 3");

// the structuring element as the kernels read it: g[i] = (dz + 3) | (dy + 3) << 8 | (set of dx, bit dx + 3) << 16,
// a source at p - (dz, dy, dx); rz / ry = the largest |dz| / |dy|
struct MmGroups {
    int32_t n, rz, ry;
    int32_t g[MM_NGROUPS];
};

// the OR over the offsets for one output word; fetch(dz, dy, dw) = the word dz planes, dy rows and dw words on
template <typename F>
__device__ __forceinline__ uint32_t mm_dilate(const MmGroups& G, F fetch) {
    uint32_t r = 0;
    for (int i = 0; i < G.n; ++i) {                                   // uniform: the groups travel as kernel arguments
        const int32_t g = G.g[i];
        const int dz = (g & 0xff) - MM_R, dy = ((g >> 8) & 0xff) - MM_R;
        const uint32_t set = (uint32_t)g >> 16;
        const uint32_t cur = fetch(-dz, -dy, 0);
        if (set & 0x08u) r |= cur;
        if (set & 0x70u) {                                            // dx > 0: bit x comes from bit x - dx
            const uint32_t prev = fetch(-dz, -dy, -1);
            if (set & 0x10u) r |= (cur << 1) | (prev >> 31);
            if (set & 0x20u) r |= (cur << 2) | (prev >> 30);
            if (set & 0x40u) r |= (cur << 3) | (prev >> 29);
        }
        if (set & 0x07u) {                                            // dx < 0: from bit x + |dx|
            const uint32_t next = fetch(-dz, -dy, 1);
            if (set & 0x04u) r |= (cur >> 1) | (next << 31);
            if (set & 0x02u) r |= (cur >> 2) | (next << 30);
            if (set & 0x01u) r |= (cur >> 3) | (next << 29);
        }
    }
    return r;
}

// one lane of the wave reports a change: at most one atomic per wave and call
__device__ __forceinline__ void mm_report(uint32_t* changed, bool ch) {
    if (changed != nullptr && __ballot(ch) != 0ull && (threadIdx.x & 63u) == 0u)
        __hip_atomic_fetch_or(changed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- bytes <-> bits ---------------------------------------------------------------------------------------------
// bit t = (byte t of v != 0), t < 4
__device__ __forceinline__ uint32_t mm_nonzero4(uint32_t v) {
    uint32_t t = v | (v >> 4);
    t |= t >> 2;
    t |= t >> 1;                                                      // bit 8 t = OR of the bits of byte t
    return ((t & 0x01010101u) * 0x01020408u) >> 24;                   // bits 0, 8, 16, 24 -> bits 24 ... 27, no carries
}
// byte t = bit t of r, t < 4
__device__ __forceinline__ uint32_t mm_expand4(uint32_t r) {
    return (r & 1u) | ((r & 2u) << 7) | ((r & 4u) << 14) | ((r & 8u) << 21);
}

struct MmPack {
    const uint8_t* src;                  // (nz, ny, nx) bytes, strides rs / ps
    int64_t rs, ps;
    uint32_t* dst;                       // (nz, ny, W) words
    int64_t ny, nx, W, nwords;
    uint32_t flip, pad;                  // 0 or ~0: the complement is packed / the value of a row's padding bits
};

__global__ __launch_bounds__(MM_BLOCK) void mm_pack_kernel(const MmPack A) {
    for (int64_t i = (int64_t)blockIdx.x * MM_BLOCK + threadIdx.x; i < A.nwords; i += (int64_t)gridDim.x * MM_BLOCK) {
        const int64_t row = i / A.W, w = i - row * A.W, k = row / A.ny, j = row - k * A.ny;
        const uint8_t* p = A.src + k * A.ps + j * A.rs + w * 32;
        const int64_t left = A.nx - w * 32;
        uint32_t bits = 0;
        if (left >= 32 && ((uintptr_t)p & 15u) == 0) {
            const uint4 a = *reinterpret_cast<const uint4*>(p), b = *reinterpret_cast<const uint4*>(p + 16);
            bits = mm_nonzero4(a.x) | (mm_nonzero4(a.y) << 4) | (mm_nonzero4(a.z) << 8) | (mm_nonzero4(a.w) << 12) |
                   (mm_nonzero4(b.x) << 16) | (mm_nonzero4(b.y) << 20) | (mm_nonzero4(b.z) << 24) | (mm_nonzero4(b.w) << 28);
        } else if (left >= 32 && ((uintptr_t)p & 3u) == 0) {
#pragma unroll
            for (int t = 0; t < 8; ++t) bits |= mm_nonzero4(reinterpret_cast<const uint32_t*>(p)[t]) << (4 * t);
        } else {
            const int n = left < 32 ? (int)left : 32;
            for (int t = 0; t < n; ++t) bits |= (p[t] != 0 ? 1u : 0u) << t;
        }
        const uint32_t valid = left >= 32 ? ~0u : (1u << (int)left) - 1u;
        A.dst[i] = ((bits ^ A.flip) & valid) | (A.pad & ~valid);
    }
}

struct MmUnpack {
    const uint32_t* src;                 // (nz, ny, W) words
    uint8_t* dst;                        // (nz, ny, nx) bytes, compact
    int64_t nx, W, nwords;
    uint32_t flip;
};

__global__ __launch_bounds__(MM_BLOCK) void mm_unpack_kernel(const MmUnpack A) {
    for (int64_t i = (int64_t)blockIdx.x * MM_BLOCK + threadIdx.x; i < A.nwords; i += (int64_t)gridDim.x * MM_BLOCK) {
        const int64_t row = i / A.W, w = i - row * A.W;
        uint8_t* p = A.dst + row * A.nx + w * 32;
        const int64_t left = A.nx - w * 32;
        const uint32_t bits = A.src[i] ^ A.flip;
        if (left >= 32 && ((uintptr_t)p & 15u) == 0) {
            uint4 a, b;
            a.x = mm_expand4(bits); a.y = mm_expand4(bits >> 4); a.z = mm_expand4(bits >> 8); a.w = mm_expand4(bits >> 12);
            b.x = mm_expand4(bits >> 16); b.y = mm_expand4(bits >> 20); b.z = mm_expand4(bits >> 24); b.w = mm_expand4(bits >> 28);
            *reinterpret_cast<uint4*>(p) = a;
            *reinterpret_cast<uint4*>(p + 16) = b;
        } else if (left >= 32 && ((uintptr_t)p & 3u) == 0) {
#pragma unroll
            for (int t = 0; t < 8; ++t) reinterpret_cast<uint32_t*>(p)[t] = mm_expand4(bits >> (4 * t));
        } else {
            const int n = left < 32 ? (int)left : 32;
            for (int t = 0; t < n; ++t) p[t] = (uint8_t)((bits >> t) & 1u);
        }
    }
}

// ---- one synchronous step: dst = mask ? D(src) : src ------------------------------------------------------------------
struct MmStep {
    const uint32_t* src;
    uint32_t* dst;
    const uint32_t* mask;                // packed, padding bits 0; or nullptr
    int64_t nz, ny, W, nwords;
    uint32_t tail;                       // the bits of a row's last word that are voxels
    uint32_t border;                     // 0 or ~0
    uint32_t* changed;                   // or nullptr
    MmGroups G;
};

__global__ __launch_bounds__(MM_BLOCK) void mm_step_kernel(const MmStep A) {
    bool ch = false;
    for (int64_t i = (int64_t)blockIdx.x * MM_BLOCK + threadIdx.x; i < A.nwords; i += (int64_t)gridDim.x * MM_BLOCK) {
        const int64_t row = i / A.W, w = i - row * A.W, k = row / A.ny, j = row - k * A.ny;
        uint32_t r = mm_dilate(A.G, [&](int dz, int dy, int dw) -> uint32_t {
            const int64_t kk = k + dz, jj = j + dy, ww = w + dw;
            if (kk < 0 || kk >= A.nz || jj < 0 || jj >= A.ny || ww < 0 || ww >= A.W) return A.border;
            return A.src[(kk * A.ny + jj) * A.W + ww];
        });
        const uint32_t cur = A.src[i];
        if (A.mask != nullptr) {
            const uint32_t m = A.mask[i];
            r = (m & r) | (~m & cur);
        }
        if (w == A.W - 1) r = (r & A.tail) | (A.border & ~A.tail);
        A.dst[i] = r;
        ch |= r != cur;
    }
    mm_report(A.changed, ch);
}

// ---- one sweep to the fixed point of a structure that holds its centre: every tile settled in LDS, in place ----------
struct MmSettle {
    uint32_t* buf;
    const uint32_t* mask;                // or nullptr
    int64_t nz, ny, W;
    int64_t tiles_y, tiles_w, ntiles;
    uint32_t tail, border;
    uint32_t* changed;
    MmGroups G;
};

__global__ __launch_bounds__(MM_BLOCK) void mm_settle_kernel(const MmSettle A) {
    __shared__ uint32_t tile[MM_LDS_WORDS];
    const int rz = A.G.rz, ry = A.G.ry;
    const int ez = MM_TZ + 2 * rz, ey = MM_TY + 2 * ry;               // planes and rows staged, halo included
    bool stored = false;
    for (int64_t t = blockIdx.x; t < A.ntiles; t += gridDim.x) {
        const int64_t tw = t % A.tiles_w, tr = t / A.tiles_w, ty = tr % A.tiles_y, tz = tr / A.tiles_y;
        const int64_t k0 = tz * MM_TZ, j0 = ty * MM_TY, w0 = tw * MM_TW;
        __syncthreads();                                              // the tile before this one has been read
        for (int i = threadIdx.x; i < ez * ey * MM_LW; i += MM_BLOCK) {
            const int lw = i % MM_LW, lr = i / MM_LW, ly = lr % ey, lz = lr / ey;
            const int64_t kk = k0 - rz + lz, jj = j0 - ry + ly, ww = w0 - 1 + lw;
            const bool inside = kk >= 0 && kk < A.nz && jj >= 0 && jj < A.ny && ww >= 0 && ww < A.W;
            tile[i] = inside ? A.buf[(kk * A.ny + jj) * A.W + ww] : A.border;
        }
        uint32_t cur[MM_PER_THREAD], first[MM_PER_THREAD], m[MM_PER_THREAD], nxt[MM_PER_THREAD];
        int at[MM_PER_THREAD];
        int64_t gi[MM_PER_THREAD];
#pragma unroll
        for (int q = 0; q < MM_PER_THREAD; ++q) {
            const int id = threadIdx.x + q * MM_BLOCK, w = id % MM_TW, y = (id / MM_TW) % MM_TY, z = id / (MM_TW * MM_TY);
            const int64_t kk = k0 + z, jj = j0 + y, ww = w0 + w;
            const bool inside = kk < A.nz && jj < A.ny && ww < A.W;
            gi[q] = inside ? (kk * A.ny + jj) * A.W + ww : -1;
            m[q] = inside ? (A.mask != nullptr ? A.mask[gi[q]] : ~0u) : 0u;   // a word outside the array never changes
            if (inside && ww == A.W - 1) m[q] &= A.tail;              // nor do the padding bits
            at[q] = ((rz + z) * ey + (ry + y)) * MM_LW + 1 + w;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < MM_PER_THREAD; ++q) cur[q] = first[q] = tile[at[q]];
        for (;;) {
            bool ch = false;
#pragma unroll
            for (int q = 0; q < MM_PER_THREAD; ++q) {
                nxt[q] = cur[q];
                if ((m[q] & ~cur[q]) != 0u) {                         // a bit of the mask is still unset
                    const int a = at[q];
                    const uint32_t r = mm_dilate(A.G, [&](int dz, int dy, int dw) -> uint32_t {
                        return tile[a + (dz * ey + dy) * MM_LW + dw];
                    });
                    nxt[q] = cur[q] | (r & m[q]);                     // mask ? r : cur, r >= cur: the centre is an offset
                    ch |= nxt[q] != cur[q];
                }
            }
            if (!__syncthreads_or(ch ? 1 : 0)) break;                 // every read of this round is done
#pragma unroll
            for (int q = 0; q < MM_PER_THREAD; ++q) {
                if (nxt[q] != cur[q]) tile[at[q]] = nxt[q];
                cur[q] = nxt[q];
            }
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < MM_PER_THREAD; ++q) {
            if (cur[q] != first[q] && gi[q] >= 0) {                   // (a word outside the array has m = 0: it never changes)
                A.buf[gi[q]] = cur[q];
                stored = true;
            }
        }
    }
    mm_report(A.changed, stored);
}

// ---- host ---------------------------------------------------------------------------------------------------------------
struct MmShape {
    int64_t nz, ny, nx, W, nwords;
};

bool mm_shape(int64_t nz, int64_t ny, int64_t nx, MmShape* S) {
    if (nz <= 0 || ny <= 0 || nx <= 0) return false;
    S->nz = nz; S->ny = ny; S->nx = nx;
    S->W = (nx + 31) / 32;
    S->nwords = nz * ny * S->W;
    return true;
}

unsigned mm_grid(int64_t n, int64_t per_block) {
    const int64_t b = (n + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b < MM_MAX_BLOCKS ? b : MM_MAX_BLOCKS));
}

bool mm_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

// strides resolved and checked as the mask program's slots are (rows / planes views, exchanged first axes)
int mm_view(const char* what, const MmShape& S, const uint8_t* p, int64_t* rs, int64_t* ps, int64_t* extent) {
    SPC_REQUIRE(p != nullptr, "%s is NULL", what);
    if (!*rs) *rs = S.nx;
    if (!*ps) *ps = S.ny * *rs;
    SPC_REQUIRE(*rs >= S.nx && *ps >= S.nx, "%s: row / plane stride smaller than nx", what);
    SPC_REQUIRE(*ps >= *rs * (S.ny - 1) + S.nx || *rs >= *ps * (S.nz - 1) + S.nx, "%s: overlapping rows and planes", what);
    *extent = (S.nz - 1) * *ps + (S.ny - 1) * *rs + S.nx;
    return SPC_OK;
}

// the change words of a batch come back to the host: the call waits for its stream here
int mm_read_changed(const uint32_t* d_changed, uint32_t (&h)[MM_BATCH], hipStream_t st) {
    SPC_HIP(hipMemcpyAsync(h, d_changed, sizeof(h), hipMemcpyDeviceToHost, st));
    SPC_HIP(hipStreamSynchronize(st));
    return SPC_OK;
}

}  // namespace

extern "C" {

size_t spc_mask_morph_workspace_bytes(int64_t nz, int64_t ny, int64_t nx) {
    MmShape S;
    if (!mm_shape(nz, ny, nx, &S)) return 0;
    // two packed buffers, the packed mask, the change words; a slice may start up to 255 bytes into the workspace
    return 3 * spc_ws_round(sizeof(uint32_t) * (size_t)S.nwords) + spc_ws_round(sizeof(uint32_t) * MM_BATCH) + 256;
}

int spc_mask_morph_u8(int device, void* stream, int64_t nz, int64_t ny, int64_t nx,
                      const uint8_t* d_in, int64_t in_row_stride, int64_t in_plane_stride,
                      const uint8_t* d_mask, int64_t mask_row_stride, int64_t mask_plane_stride,
                      int op, const int8_t* h_offsets, int noffsets, int iterations, int border_value,
                      uint8_t* d_out, void* d_workspace, size_t workspace_bytes, int64_t* h_iterations_run) {
    MmShape S;
    SPC_REQUIRE(mm_shape(nz, ny, nx, &S), "mask shape must be positive (got %lld,%lld,%lld)", (long long)nz, (long long)ny,
                (long long)nx);
    SPC_REQUIRE(d_out != nullptr, "d_out is NULL");
    int64_t irs = in_row_stride, ips = in_plane_stride, mrs = mask_row_stride, mps = mask_plane_stride, iext = 0, mext = 0;
    int rc = mm_view("d_in", S, d_in, &irs, &ips, &iext);
    if (rc) return rc;
    if (d_mask != nullptr && (rc = mm_view("d_mask", S, d_mask, &mrs, &mps, &mext)) != SPC_OK) return rc;
    SPC_REQUIRE(op == SPC_MORPH_ERODE || op == SPC_MORPH_DILATE, "unknown op %d (0 = erode, 1 = dilate)", op);
    SPC_REQUIRE(border_value == 0 || border_value == 1, "border_value must be 0 or 1 (got %d)", border_value);
    SPC_REQUIRE(h_offsets != nullptr, "h_offsets is NULL");
    SPC_REQUIRE(noffsets >= 1 && noffsets <= SPC_MORPH_MAX_OFFSETS, "%d offsets: 1 to %d", noffsets, SPC_MORPH_MAX_OFFSETS);
    const int64_t nout = nz * ny * nx;
    SPC_REQUIRE(!mm_overlap(d_out, nout, d_in, iext), "d_out overlaps d_in: the result is never written in place");
    SPC_REQUIRE(d_mask == nullptr || !mm_overlap(d_out, nout, d_mask, mext), "d_out overlaps d_mask");

    // erosion = dilation of the complement with the reflected offsets: a source at p - o' with o' = -o
    const bool erode = op == SPC_MORPH_ERODE;
    uint32_t sets[2 * MM_R + 1][2 * MM_R + 1] = {};
    for (int i = 0; i < noffsets; ++i) {
        int o[3];
        for (int a = 0; a < 3; ++a) {
            o[a] = h_offsets[3 * i + a];
            SPC_REQUIRE(o[a] >= -MM_R && o[a] <= MM_R, "offset %d: component %d beyond +-%d", i, o[a], MM_R);
            if (erode) o[a] = -o[a];
        }
        sets[o[0] + MM_R][o[1] + MM_R] |= 1u << (o[2] + MM_R);
    }
    MmGroups G{};
    for (int a = 0; a <= 2 * MM_R; ++a)
        for (int b = 0; b <= 2 * MM_R; ++b) {
            if (!sets[a][b]) continue;
            G.g[G.n++] = a | (b << 8) | (int32_t)(sets[a][b] << 16);
            const int dz = a > MM_R ? a - MM_R : MM_R - a, dy = b > MM_R ? b - MM_R : MM_R - b;
            if (dz > G.rz) G.rz = dz;
            if (dy > G.ry) G.ry = dy;
        }
    const bool centre = (sets[MM_R][MM_R] >> MM_R) & 1u;

    SpcWorkspace ws(d_workspace, workspace_bytes);
    SPC_WS_TAKE(d_a, ws, uint32_t, S.nwords);
    SPC_WS_TAKE(d_b, ws, uint32_t, S.nwords);
    SPC_WS_TAKE(d_m, ws, uint32_t, S.nwords);
    SPC_WS_TAKE(d_changed, ws, uint32_t, MM_BATCH);
    SPC_REQUIRE(!mm_overlap(d_workspace, (int64_t)ws.used, d_out, nout) && !mm_overlap(d_workspace, (int64_t)ws.used, d_in, iext) &&
                    (d_mask == nullptr || !mm_overlap(d_workspace, (int64_t)ws.used, d_mask, mext)),
                "d_workspace overlaps an input or d_out");

    SPC_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t border = ((border_value != 0) != erode) ? ~0u : 0u;        // of the dilation that runs
    const uint32_t tail = (nx & 31) ? (1u << (int)(nx & 31)) - 1u : ~0u;
    const unsigned gw = mm_grid(S.nwords, MM_BLOCK);

    MmPack P{};
    P.src = d_in; P.rs = irs; P.ps = ips; P.dst = d_a;
    P.ny = ny; P.nx = nx; P.W = S.W; P.nwords = S.nwords;
    P.flip = erode ? ~0u : 0u; P.pad = border;
    hipLaunchKernelGGL(mm_pack_kernel, dim3(gw), dim3(MM_BLOCK), 0, st, P);
    SPC_LAUNCH_CHECK();
    if (d_mask != nullptr) {
        P.src = d_mask; P.rs = mrs; P.ps = mps; P.dst = d_m;
        P.flip = 0u; P.pad = 0u;
        hipLaunchKernelGGL(mm_pack_kernel, dim3(gw), dim3(MM_BLOCK), 0, st, P);
        SPC_LAUNCH_CHECK();
    }

    MmStep T{};
    T.src = d_a; T.dst = d_b; T.mask = d_mask != nullptr ? d_m : nullptr;
    T.nz = nz; T.ny = ny; T.W = S.W; T.nwords = S.nwords;
    T.tail = tail; T.border = border; T.changed = nullptr; T.G = G;
    int64_t run = 0;
    if (iterations >= 1) {
        for (int it = 0; it < iterations; ++it) {
            hipLaunchKernelGGL(mm_step_kernel, dim3(gw), dim3(MM_BLOCK), 0, st, T);
            SPC_LAUNCH_CHECK();
            const uint32_t* s = T.src;
            T.src = T.dst; T.dst = const_cast<uint32_t*>(s);
        }
        run = iterations;
    } else if (centre) {
        MmSettle E{};
        E.buf = d_a; E.mask = T.mask;
        E.nz = nz; E.ny = ny; E.W = S.W;
        E.tiles_y = (ny + MM_TY - 1) / MM_TY; E.tiles_w = (S.W + MM_TW - 1) / MM_TW;
        E.ntiles = ((nz + MM_TZ - 1) / MM_TZ) * E.tiles_y * E.tiles_w;
        E.tail = tail; E.border = border; E.G = G;
        const unsigned gt = mm_grid(E.ntiles, 1);
        for (bool settled = false; !settled;) {
            SPC_HIP(hipMemsetAsync(d_changed, 0, sizeof(uint32_t) * MM_BATCH, st));
            for (int b = 0; b < MM_BATCH; ++b) {
                E.changed = d_changed + b;
                hipLaunchKernelGGL(mm_settle_kernel, dim3(gt), dim3(MM_BLOCK), 0, st, E);
                SPC_LAUNCH_CHECK();
            }
            uint32_t h[MM_BATCH];
            if ((rc = mm_read_changed(d_changed, h, st)) != SPC_OK) return rc;
            for (int b = 0; b < MM_BATCH && !settled; ++b) {
                ++run;
                settled = h[b] == 0u;
            }
        }
    } else {
        for (bool settled = false; !settled;) {
            if (run >= MM_STEP_LIMIT) {
                spc_set_error("no fixed point after %lld steps (a structure without its centre can cycle)", (long long)run);
                return SPC_ERR_UNSUPPORTED;
            }
            SPC_HIP(hipMemsetAsync(d_changed, 0, sizeof(uint32_t) * MM_BATCH, st));
            for (int b = 0; b < MM_BATCH; ++b) {
                T.changed = d_changed + b;
                hipLaunchKernelGGL(mm_step_kernel, dim3(gw), dim3(MM_BLOCK), 0, st, T);
                SPC_LAUNCH_CHECK();
                const uint32_t* s = T.src;
                T.src = T.dst; T.dst = const_cast<uint32_t*>(s);
            }
            uint32_t h[MM_BATCH];
            if ((rc = mm_read_changed(d_changed, h, st)) != SPC_OK) return rc;
            for (int b = 0; b < MM_BATCH && !settled; ++b) {          // from the first step that changed nothing on, the
                ++run;                                                // two buffers are equal: whichever is last holds it
                settled = h[b] == 0u;
            }
        }
    }

    MmUnpack U{};
    U.src = T.src; U.dst = d_out; U.nx = nx; U.W = S.W; U.nwords = S.nwords;
    U.flip = erode ? ~0u : 0u;
    hipLaunchKernelGGL(mm_unpack_kernel, dim3(gw), dim3(MM_BLOCK), 0, st, U);
    SPC_LAUNCH_CHECK();
    if (h_iterations_run != nullptr) *h_iterations_run = run;
    return SPC_OK;
}

}  // extern "C"
