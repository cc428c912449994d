// The forms in which spc_moments.hip reads a reused mask and cube, built here: the mask array as bits, the list of the lane
// segments the bits include, and the voxel list compacted from that list (layouts and rules: include/spcube_hip.h).  The kernels
// that READ them are instantiations of moments_kernel in spc_moments.hip, which owns the launch plan (spc_moments_list_launch).
#include "spc_moments_forms.h"
#include <algorithm>

namespace {

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
    SPC_REQUIRE(desc_is_a_plan(d) && d.nblocks >= 1 && d.nblocks < (1LL << 31), "the list's desc is not a launch plan");
    *total = d.nblocks * d.nsub;
    SPC_REQUIRE(sublist_blocks(*total) < (1LL << 31), "too many sublists");
    const ArraysBad bad = list_arrays_bad(*list, *total, with_samples);
    SPC_REQUIRE(bad != kBadSublists, "the list's d_off and d_len: %zu entries given, %lld sublists", list->nsublists, (long long)*total);
    SPC_REQUIRE(bad != kBadNull, "the list's d_samples or d_meta is NULL");
    SPC_REQUIRE(bad != kBadSmall, "the list's d_samples / d_meta too small for %llu rows (1024 and 256 bytes each)",
                (unsigned long long)list->rows);
    SPC_REQUIRE(bad != kBadAlign, "the list's d_samples must be 16-byte, d_off 8-byte, d_meta and d_len 4-byte aligned");
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

int spc_moments_list_count_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                               const spc_moment_outputs* out, const void* d_workspace, size_t workspace_bytes,
                               const void* d_mask_bits, size_t bits_bytes, uint32_t* d_len, uint32_t* d_lines,
                               size_t nsublists, spc_moments_list_desc* desc) {
    SPC_REQUIRE(desc != nullptr, "desc is NULL");
    SPC_REQUIRE(d_mask_bits != nullptr, "d_mask_bits is NULL");
    SPC_REQUIRE(d_len != nullptr && d_lines != nullptr, "d_len or d_lines is NULL");
    spc_moments_list_desc d;
    const uint8_t* bits = nullptr;
    const int rc = spc_moments_list_launch(cube, mask, out, d_workspace, workspace_bytes, d_mask_bits, bits_bytes,
                                           "spc_moments_list_count_f32", &d, &bits);
    if (rc) return rc;
    const int64_t total = d.nblocks * d.nsub;
    SPC_REQUIRE(nsublists >= (size_t)total, "d_len and d_lines too small: %zu entries given, %lld sublists", nsublists, (long long)total);
    SPC_REQUIRE(spc_aligned(d_len, 4) && spc_aligned(d_lines, 4), "d_len and d_lines must be 4-byte aligned");
    SPC_REQUIRE(sublist_blocks(total) < (1LL << 31), "too many sublists");
    *desc = d;
    SPC_DEVICE(device);
    ListArgs L{};
    L.bits = bits; L.nz = cube->nz; L.zchunk = d.zchunk; L.nsub = d.nsub; L.total = total; L.zw = d.zw;
    L.len = d_len; L.lines = d_lines;
    hipLaunchKernelGGL(list_count_kernel, dim3((unsigned)sublist_blocks(total)), dim3(kLanes * kListWaves), 0, (hipStream_t)stream, L);
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
    SPC_REQUIRE(desc_is_a_plan(d) && d.nblocks == (ngroups + kLanes - 1) / kLanes, "desc is not a launch plan of this cube");
    // the splits cover [0, nz) and none of them is empty
    SPC_REQUIRE(d.zchunk <= cube->nz && (int64_t)(d.nsplit - 1) * d.zchunk < cube->nz && (int64_t)d.nsplit * d.zchunk >= cube->nz,
                "desc: %d splits of %lld planes do not cover %lld planes", d.nsplit, (long long)d.zchunk, (long long)cube->nz);
    const int64_t total = d.nblocks * d.nsub;
    const ArraysBad bad = list_arrays_bad(*list, total, true);
    SPC_REQUIRE(bad != kBadSublists, "d_off and d_len: %zu entries given, %lld sublists", list->nsublists, (long long)total);
    SPC_REQUIRE(bad != kBadNull, "d_samples or d_meta is NULL");
    SPC_REQUIRE(bad != kBadSmall, "d_samples / d_meta too small for %llu rows (1024 and 256 bytes each)", (unsigned long long)list->rows);
    SPC_REQUIRE(bad != kBadAlign, "d_samples must be 16-byte, d_off 8-byte, d_meta and d_len 4-byte aligned");
    SPC_REQUIRE(sublist_blocks(total) < (1LL << 31), "too many sublists");
    SPC_DEVICE(device);
    ListArgs L{};
    L.bits = (const uint8_t*)d_mask_bits; L.nz = cube->nz; L.zchunk = d.zchunk; L.nsub = d.nsub; L.total = total; L.zw = d.zw;
    L.cube = cube->d_data; L.row_stride = cube->row_stride; L.plane_stride = cube->plane_stride;
    L.groups_per_row = cube->nx / 4; L.ngroups = ngroups;
    L.off = list->d_off; L.flen = list->d_len;
    L.samples = (f32x4*)list->d_samples; L.meta = (uint32_t*)list->d_meta; L.rows = list->rows;
    hipLaunchKernelGGL(list_fill_kernel, dim3((unsigned)sublist_blocks(total)), dim3(kLanes * kListWaves), 0, (hipStream_t)stream, L);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
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
    hipLaunchKernelGGL(vlist_count_kernel, dim3((unsigned)sublist_blocks(total)), dim3(kLanes * kListWaves), 0, (hipStream_t)stream, V);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

int spc_moments_vlist_fill_f32(int device, void* stream, const spc_moments_list* list, const spc_moments_vlist* vlist) {
    int64_t total = 0;
    int rc = vlist_source_check(list, true, &total);
    if (rc) return rc;
    SPC_REQUIRE(vlist != nullptr, "vlist is NULL");
    SPC_REQUIRE(same_desc(list->desc, vlist->desc), "the voxel list's desc is not the list's");
    const ArraysBad bad = vlist_arrays_bad(*vlist, total);
    SPC_REQUIRE(bad != kBadSublists, "d_off and d_len: %zu entries given, %lld sublists", vlist->nsublists, (long long)total);
    SPC_REQUIRE(bad != kBadNull, "d_entries is NULL");
    SPC_REQUIRE(bad != kBadSmall, "d_entries too small for %llu rows (512 bytes each)", (unsigned long long)vlist->rows);
    SPC_REQUIRE(bad != kBadAlign, "d_entries and d_off must be 8-byte, d_len 4-byte aligned");
    SPC_DEVICE(device);
    VlistArgs V{};
    V.meta = (const uint32_t*)list->d_meta; V.samples = (const f32x4*)list->d_samples;
    V.off = list->d_off; V.len = list->d_len; V.rows = list->rows; V.total = total;
    V.voff = vlist->d_off; V.vlen = vlist->d_len; V.entries = (u32x2*)vlist->d_entries; V.vrows = vlist->rows;
    hipLaunchKernelGGL(vlist_fill_kernel, dim3((unsigned)sublist_blocks(total)), dim3(kLanes * kListWaves), 0, (hipStream_t)stream, V);
    SPC_LAUNCH_CHECK();
    return SPC_OK;
}

}  // extern "C"
