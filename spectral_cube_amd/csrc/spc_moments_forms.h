// What spc_moments.hip (the march, its launch plan, the four spc_moments*_f32 entries) and spc_moments_forms.hip (the builders
// of the packed mask, the list and the voxel list) share: the shapes of the forms and the host checks both units make.
#pragma once
#include "spc_common.h"

constexpr int kLanes = 64;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));   // an entry of the voxel list: { bits of v, meta }

constexpr int64_t kListMaxNz = 1LL << 28;      // z shares its meta word with the nibble
constexpr int kListWaves = 4;                  // sublists per block of the count and fill kernels
constexpr int kVlistLongSublist = 128;         // mean rows per sublist from which the sums and count forms keep 16 rows in flight (moments_run)

static inline size_t mask_bits_bytes(int64_t nz, int64_t ny, int64_t nx) {
    if (nz <= 0 || ny <= 0 || nx <= 0 || nx % 4 != 0) return 0;
    const int64_t ngroups = ny * (nx / 4);
    return (size_t)((ngroups + kLanes - 1) / kLanes) * (size_t)nz * 32;
}

static inline bool same_desc(const spc_moments_list_desc& d, const spc_moments_list_desc& l) {
    return d.zw == l.zw && d.nsplit == l.nsplit && d.zchunk == l.zchunk && d.nblocks == l.nblocks && d.nsub == l.nsub;
}

// the desc has the shape of a launch plan (of which cube, its nblocks says: the callers check that)
static inline bool desc_is_a_plan(const spc_moments_list_desc& d) {
    return (d.zw == 1 || d.zw == 4 || d.zw == 8) && d.nsplit >= 1 && d.zchunk >= 1 && d.nsub == (int64_t)d.nsplit * d.zw;
}

// blocks of a kernel that gives one wave to each of `total` sublists; a launch needs fewer than 2^31
static inline int64_t sublist_blocks(int64_t total) { return (total + kListWaves - 1) / kListWaves; }

// Do a list's / a voxel list's arrays hold the rows it names, for `total` sublists, and are they aligned?  The builders name
// the first thing that is wrong; moments_run reads what passes and marches otherwise.  with_samples: d_samples is read too
enum ArraysBad { kArraysOk = 0, kBadSublists, kBadNull, kBadSmall, kBadAlign };

static inline ArraysBad list_arrays_bad(const spc_moments_list& l, int64_t total, bool with_samples) {
    if (!l.d_off || !l.d_len || l.nsublists < (size_t)total) return kBadSublists;
    if (l.rows != 0 && (!l.d_meta || (with_samples && !l.d_samples))) return kBadNull;
    if (l.meta_bytes / 256 < l.rows || (with_samples && l.samples_bytes / 1024 < l.rows)) return kBadSmall;
    if (!spc_aligned(l.d_meta, 4) || !spc_aligned(l.d_off, 8) || !spc_aligned(l.d_len, 4) || (with_samples && !spc_aligned(l.d_samples, 16)))
        return kBadAlign;
    return kArraysOk;
}

static inline ArraysBad vlist_arrays_bad(const spc_moments_vlist& v, int64_t total) {
    if (!v.d_off || !v.d_len || v.nsublists < (size_t)total) return kBadSublists;
    if (v.rows != 0 && !v.d_entries) return kBadNull;
    if (v.entries_bytes / 512 < v.rows) return kBadSmall;
    if (!spc_aligned(v.d_entries, 8) || !spc_aligned(v.d_off, 8) || !spc_aligned(v.d_len, 4)) return kBadAlign;
    return kArraysOk;
}

// spc_moments.hip: the plan of the launch spc_moments_bits_f32 would make of these arguments, as a list is made for it, and in
// *bits (when asked for) the packed mask it reads; d_mask_bits NULL: the plan alone.  SPC_ERR_UNSUPPORTED: no list (says `who`)
int spc_moments_list_launch(const spc_cube_f32* cube, const spc_mask* mask, const spc_moment_outputs* out, const void* d_workspace,
                            size_t workspace_bytes, const void* d_mask_bits, size_t bits_bytes, const char* who,
                            spc_moments_list_desc* desc, const uint8_t** bits);
