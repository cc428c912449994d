/*
 * spcube_hip.h - C ABI of libspcube_hip.so, the MI355X (gfx950) engine behind
 * spectral-cube's dense hot path.
 *
 * The reference (radio-astro-tools/spectral-cube) is pure Python and has no
 * FFI; the operator seams this library is bound at are listed per entry point
 * (paths relative to the reference tree).  INTEGRATION.md shows the ctypes
 * binding a maintainer would add on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success, a negative spc_status otherwise;
 *     spc_last_error() gives a thread-local message; nothing throws;
 *   - the caller owns every buffer, scratch included; "d_" pointers are device (HBM)
 *     addresses obtained from spc_malloc (or any hipMalloc), "h_" pointers are host.
 *     No compute entry point allocates, frees or drains the device: a call that needs
 *     scratch takes (d_workspace, workspace_bytes) - spc_workspace_bytes() gives the
 *     size - and queues everything on the caller's stream.  The host is only made to
 *     wait (for THAT stream) where a result comes back to it: the entry points with
 *     an "h_" output say so;
 *   - cubes are C-contiguous (nz, ny, nx) float32, spectral axis first, x
 *     fastest; row/plane strides are given in ELEMENTS so that a (y) row strip
 *     of a larger cube can be processed in place;
 *   - an axis may be longer than 65535 (the largest launch-grid y / z dimension): the
 *     entry points split such a call into launches of their own, so shapes are limited
 *     by memory and by the int64_t fields, not by the grid.  Known exceptions:
 *     spc_wcs_pixel_map_f64 and spc_resample_spline_f32 take at most 262140 output
 *     rows, and the spline form at most 65535 channels per call;
 *   - every launch takes a device index and a stream handle (hipStream_t as
 *     void*, NULL = default stream); there is no global mutable state, so dask
 *     `threads` workers and one-process-per-GPU drivers may call concurrently;
 *   - no torch / numpy types cross this boundary.
 */
#ifndef SPCUBE_HIP_H
#define SPCUBE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPC_ABI_VERSION 8

typedef enum {
    SPC_OK = 0,
    SPC_ERR_INVALID = -1,     /* bad argument (shape, pointer, flag) */
    SPC_ERR_HIP = -2,         /* HIP runtime error, see spc_last_error() */
    SPC_ERR_UNSUPPORTED = -3, /* valid request this build cannot serve */
    SPC_ERR_NOMEM = -4,
    SPC_ERR_COMM = -5         /* RCCL error */
} spc_status;

/* ---- mask specification ------------------------------------------------
 * Restates MaskBase.include / _filled (spectral_cube/masks.py:105-116,
 * 197-237) for the mask kinds that can be evaluated on the fly:
 *   BooleanArrayMask (masks.py:457-584)  -> SPC_MASK_ARRAY (uint8, !=0 = include)
 *   LazyMask(np.isfinite) (io/fits.py:214) -> SPC_MASK_FINITE
 *   LazyComparisonMask cube > x etc. (masks.py:670-758) -> SPC_MASK_GT/GE/LT/LE
 * Flags are AND-ed (CompositeMask 'and', masks.py:425-435).  Other
 * compositions (or / xor / not, == and !=, thresholds that are maps, spectra
 * or cubes, terms on several cubes) are compiled into a spc_mask_program and
 * evaluated once on the device into a uint8 array (spc_mask_eval_*, below);
 * only what that cannot express (an arbitrary Python function) is
 * materialised by the host.
 * A voxel is "valid" when it is included AND its value is not NaN (NaN-filled
 * data fed to nansum, dask_spectral_cube.py:1083).
 * The include array, for every entry that takes one (d_array here, the uint8
 * operands of a spc_mask_program, the inputs of spc_mask_morph_u8 and
 * spc_label_u8, a keep table):
 *   - ANY non-zero byte includes: 1, 2, 0x80 and 0xFF mean the same, and a
 *     caller may hand in bytes of any origin (a bool array, a bit test, a count);
 *   - a byte is never a weight or a count: it selects, nothing else;
 *   - no entry reads a cube sample that the array excludes in a way that can
 *     reach a result: an excluded sample is dropped by a select in front of the
 *     arithmetic, never by a product with 0, so NaN, +-inf and +-max under
 *     excluded voxels change no bit of any output.  (spc_subcube_* with
 *     filled == 0 copies the raw samples: the one entry that shows them.)
 * Every entry that WRITES a mask (spc_mask_eval_*, spc_mask_include_*, the
 * d_out_mask of spc_downsample_* and spc_subcube_*, the d_footprint of the
 * resamplers, spc_mask_morph_u8, spc_label_select_i32) writes 0 / 1 bytes; none
 * copies the input's bytes.  tests/mask_patterns.py and
 * tests/test_gpu_mask_patterns.py hold every masked entry to this. */
#define SPC_MASK_NONE   0u
#define SPC_MASK_ARRAY  1u
#define SPC_MASK_FINITE 2u
#define SPC_MASK_GT     4u   /* data >  thr_lo */
#define SPC_MASK_GE     8u   /* data >= thr_lo */
#define SPC_MASK_LT     16u  /* data <  thr_hi */
#define SPC_MASK_LE     32u  /* data <= thr_hi */

typedef struct {
    uint32_t flags;
    float thr_lo;
    float thr_hi;
    const uint8_t* d_array;      /* device ptr, may be NULL unless SPC_MASK_ARRAY */
    int64_t row_stride;          /* elements; 0 = same as the cube's */
    int64_t plane_stride;        /* elements; 0 = same as the cube's */
} spc_mask;

/* cube view: d_data points at voxel (0,0,0) of the (sub)cube */
typedef struct {
    const float* d_data;
    int64_t nz, ny, nx;
    int64_t row_stride;          /* elements between (z,y,x) and (z,y+1,x) */
    int64_t plane_stride;        /* elements between (z,y,x) and (z+1,y,x) */
} spc_cube_f32;

/* ---- library / device management -------------------------------------- */
int spc_abi_version(void);
const char* spc_last_error(void);
/* Which form spc_spatial_conv_sep_f32 tries first for a mask ARRAY, as a setting of the CALLING THREAD (like the
 * message of spc_last_error): SPC_SPATIAL_FORM_ENV, the initial value of every thread, follows the environment switch
 * SPC_SPATIAL_RING (1 = ring) read at each call; _SPLIT = the split form on the matrix cores (fp16 hi + lo products,
 * float32 sums), _RING = the ring kernels (float32 multiply-adds).  A thread's setting wins over the environment and
 * is seen by no other thread.  The setter returns the previous value, for the caller to restore; a value that is none
 * of the three is ignored (the setting and the returned previous value are as if the call had been the getter). */
#define SPC_SPATIAL_FORM_ENV   (-1)
#define SPC_SPATIAL_FORM_SPLIT 0
#define SPC_SPATIAL_FORM_RING  1
int spc_set_masked_spatial_form(int form);
int spc_get_masked_spatial_form(void);
int spc_device_count(int* count);
typedef struct {
    char name[128];
    char arch[64];               /* e.g. "gfx950:sramecc+:xnack-" */
    int compute_units;
    int wavefront_size;
    int64_t total_mem;
    int64_t free_mem;
    int clock_khz;
} spc_device_info;
int spc_get_device_info(int device, spc_device_info* info);

/* Device buffers.  spc_free keeps the block in a per-device pool (after draining the device, as
 * hipFree does) and spc_malloc hands idle blocks of nearly the requested size out again: cube-sized
 * hipMalloc calls intermittently take seconds on this stack.  The pool is bounded
 * (SPC_POOL_MAX_BYTES, default half of the device memory; SPC_POOL=0 disables it), is emptied when
 * a real allocation runs out of memory, and by spc_pool_trim.  spc_free also accepts pointers that
 * came from a plain hipMalloc.  Buffers are NOT zeroed (hipMalloc does not promise it either);
 * SPC_POOL_POISON=1 fills every returned block with 0xFF bytes to catch code that assumes so. */
int spc_malloc(int device, size_t bytes, void** d_ptr);
int spc_free(int device, void* d_ptr);
int spc_pool_trim(int device);
int spc_pool_stats(int device, int64_t* live_bytes, int64_t* idle_bytes);
int spc_host_alloc(size_t bytes, void** h_ptr);       /* pinned */
int spc_host_free(void* h_ptr);
int spc_memcpy_h2d(int device, void* d_dst, const void* h_src, size_t bytes, void* stream);
int spc_memcpy_d2h(int device, void* h_dst, const void* d_src, size_t bytes, void* stream);
int spc_memcpy_d2d(int device, void* d_dst, const void* d_src, size_t bytes, void* stream);
/* strided 3-D copies (host chunk (nz,cy,cx) <-> device strip); pitches in bytes */
int spc_memcpy3d_h2d(int device, void* d_dst, size_t d_row_pitch, size_t d_plane_pitch,
                     const void* h_src, size_t h_row_pitch, size_t h_plane_pitch,
                     size_t row_bytes, size_t ny, size_t nz, void* stream);
/* the same between two device buffers (row strips of a cube, tiling a cube from a smaller one) */
int spc_memcpy3d_d2d(int device, void* d_dst, size_t dst_row_pitch, size_t dst_plane_pitch,
                     const void* d_src, size_t src_row_pitch, size_t src_plane_pitch,
                     size_t row_bytes, size_t ny, size_t nz, void* stream);
int spc_memset(int device, void* d_ptr, int value, size_t bytes, void* stream);
int spc_stream_create(int device, void** stream);
int spc_stream_destroy(int device, void* stream);
int spc_stream_sync(int device, void* stream);
int spc_device_sync(int device);
int spc_event_create(int device, void** event);
int spc_event_destroy(int device, void* event);
int spc_event_record(int device, void* event, void* stream);
int spc_event_sync(int device, void* event);
int spc_stream_wait_event(int device, void* stream, void* event);   /* hipStreamWaitEvent */
int spc_event_elapsed_ms(int device, void* start, void* stop, float* ms);

/* ---- device scratch -----------------------------------------------------
 * Bytes of d_workspace an entry point needs for a (nz,ny,nx) cube; p0 / p1 are the
 * kernel extents or the output shape it is called with.  An upper bound that only
 * depends on these numbers (not on the data or the mask kind), so one buffer sized
 * once serves a whole pipeline of equal-sized calls.  Of the environment switches
 * (docs/DESIGN_NOTES.md lists them) two tuning hooks move a size: SPC_WS_MOMENTS
 * grows with SPC_MOMENTS_NSPLIT, and setting it or SPC_MOMENTS_VEC makes small
 * cubes that otherwise need none ask for scratch - size the buffer with the same
 * environment the calls will see.  No other kind reads a switch.  Contents need
 * not be preserved between calls; two calls in flight at the same time (two
 * streams) need two workspaces. */
typedef enum {
    SPC_WS_MOMENTS = 0,               /* spc_moments_f32 (== spc_moments_workspace_bytes) */
    SPC_WS_SPECTRAL_CONV = 1,         /* spc_spectral_conv_f32, p0 = ntaps */
    SPC_WS_SPECTRAL_CONV_MOMENTS = 2, /* spc_spectral_conv_moments_f32, p0 = ntaps */
    SPC_WS_SPATIAL_CONV_SEP = 3,      /* spc_spatial_conv_sep_f32, p0 = nky, p1 = nkx */
    SPC_WS_SPATIAL_CONV2D = 4,        /* spc_spatial_conv2d_f32, p0 = nky, p1 = nkx */
    SPC_WS_RESAMPLE_BILINEAR = 5,     /* spc_resample_bilinear_f32, p0 = ny_out, p1 = nx_out */
    SPC_WS_STATS_GLOBAL = 6,          /* spc_stats_global_f32 */
    SPC_WS_STATS_PLANES = 7,          /* spc_stats_planes_f32 */
    SPC_WS_MAP_CONV2D = 8,            /* spc_map_conv2d_f64, (ny,nx) = map, p0 = nky, p1 = nkx */
    SPC_WS_CLIP_OUTSIDE = 9,          /* spc_clip_outside_f32 */
    SPC_WS_PERCENTILE_GLOBAL = 10,    /* spc_percentile_global_f32 */
    SPC_WS_SPATIAL_CONV_MFMA = 11,    /* spc_spatial_conv_sep_mfma_f32 */
    SPC_WS_SIGMA_CLIP = 12,           /* spc_sigma_clip_axis0_f32 (ABI 7) */
    SPC_WS_RESAMPLE_BILINEAR_LERP = 13, /* spc_resample_bilinear_lerp_f32, nz = INPUT channels, p0 = ny_out, p1 = nx_out (ABI 8) */
    SPC_WS_STATS_GLOBAL_F64 = 14,     /* spc_stats_global_f64 (ABI 8) */
    SPC_WS_SPECTRAL_CONV_F64 = 15,    /* spc_spectral_conv_f64, p0 = ntaps (ABI 8) */
    SPC_WS_SPATIAL_CONV_F64 = 16      /* spc_spatial_conv_f64, p0 = nky, p1 = nkx: the taps + the (num, den) planes of a slab of at
                                       * most 256 MiB (a smaller workspace is accepted as long as one plane fits) (ABI 8) */
} spc_ws_kind;
size_t spc_workspace_bytes(int kind, int64_t nz, int64_t ny, int64_t nx, int64_t p0, int64_t p1);

/* ---- moments ------------------------------------------------------------
 * Replaces DaskSpectralCubeMixin.moment (spectral_cube/dask_spectral_cube.py
 * :1031-1132, arithmetic :1083-1104 and nansum_allbadtonan :54-59),
 * moment_cubewise/_slicewise/_raywise (spectral_cube/_moments.py:30-193),
 * allbadtonan (np_compat.py:3-27) and argmax/argmin
 * (spectral_cube/spectral_cube.py:793-819) for axis 0, in ONE pass:
 *   S0 = sum v, S1 = sum v*c[z], S2 = sum v*c[z]^2 over valid voxels (fp64)
 *   m0 = dv*S0 (NaN when no valid voxel), m1 = S1/S0 + m1_add,
 *   m2 = S2/S0 - (S1/S0)^2
 * d_cen: nz doubles in device memory = pix_cen[z] - c_ref (spectral_cube.py
 * :1473-1475); the host folds c_ref and world(chan 0) into m1_add
 * (dask_spectral_cube.py:1122-1123).  Any output pointer may be NULL.
 * argmax/argmin: first index on ties, 0 for rays without valid voxel.
 * d_workspace: spc_moments_workspace_bytes() bytes (may be NULL if 0). */
typedef struct {
    double* d_m0; double* d_m1; double* d_m2;   /* (ny,nx) float64 */
    double* d_mu;      /* S1/S0 without m1_add (input of spc_moment_order_f32) */
    double* d_s0;      /* raw S0 */
    int64_t* d_argmax; int64_t* d_argmin;       /* (ny,nx) int64 */
    float* d_vmax; float* d_vmin;               /* max/min over valid voxels (NaN if none) */
    int32_t* d_nvalid;
    int64_t out_row_stride;                     /* elements; 0 = nx */
} spc_moment_outputs;

size_t spc_moments_workspace_bytes(int64_t nz, int64_t ny, int64_t nx);
int spc_moments_f32(int device, void* stream, const spc_cube_f32* cube,
                    const spc_mask* mask, const double* d_cen, double dv,
                    double m1_add, const spc_moment_outputs* out,
                    void* d_workspace, size_t workspace_bytes);

/* The uint8 array term of a mask as BITS, for a mask that many launches reuse: an eighth of its bytes per launch.
 * Layout (it follows the moment kernel's lane mapping and nothing of its launch plan): lane group
 * g = y * (nx / 4) + x / 4 over the array as the call sees it (the rows and planes of a view included), block b = g / 64,
 * lane l = g % 64.  The bits of plane z of block b are the 32 bytes at (b * nz + z) * 32; lane l owns the nibble
 * (l & 1) * 4 of byte l >> 1, and bit i of that nibble is "mask byte of voxel x + i != 0".  Lanes past the last group
 * have zero bits.  spc_mask_bits_bytes: ceil(ny * (nx / 4) / 64) * nz * 32, or 0 where the form does not exist
 * (nx % 4 != 0, an empty shape).
 * spc_mask_pack_bits: one streaming kernel on the caller's stream writes every byte of d_bits from mask->d_array
 * (only the array term is packed; thresholds stay in the predicate; row_stride / plane_stride 0 = contiguous).
 * SPC_ERR_UNSUPPORTED where the lanes cannot read dwords: the mask's strides or address are no multiple of 4.
 * spc_moments_bits_f32 is spc_moments_f32 with the packed form of ITS mask array (d_mask_bits NULL: exactly
 * spc_moments_f32).  The bits are read only where the launch is the mask-first march of 16-byte lanes and bits_bytes
 * is large enough; odd widths, unaligned views, SPC_MOMENTS_MASK_FIRST=0 and SPC_MOMENTS_MASK_BITS=0 read the bytes as
 * before.  The maps are bit-identical either way.  The caller answers for the bits being those of the array: pack
 * again after the array's bytes change.  (Added within ABI 8: nothing existing moved.) */
size_t spc_mask_bits_bytes(int64_t nz, int64_t ny, int64_t nx);
int spc_mask_pack_bits(int device, void* stream, int64_t nz, int64_t ny, int64_t nx, const spc_mask* mask,
                       void* d_bits, size_t bits_bytes);
int spc_moments_bits_f32(int device, void* stream, const spc_cube_f32* cube,
                         const spc_mask* mask, const double* d_cen, double dv,
                         double m1_add, const spc_moment_outputs* out,
                         void* d_workspace, size_t workspace_bytes,
                         const void* d_mask_bits, size_t bits_bytes);

/* A cube reduced again under the same mask, read as a LIST of the 16-byte lane segments the mask includes, for one
 * launch plan.  The list is derived from the packed bits (above), so it always agrees with what the bits march reads.
 * Layout: lane groups and blocks are those of the bits (g = y * (nx / 4) + x / 4, b = g / 64, l = g % 64).  A launch
 * plan is (zw, nsplit, zchunk): zw waves per block, nsplit ranges of zchunk planes.  Sublist j = split * zw + w of
 * block b holds the planes wave w of split `split` marches - z = zb + w, zb + w + zw, ... < ze with zb = split * zchunk,
 * ze = min(nz, zb + zchunk) - of which a lane keeps, in ascending order, those where its nibble of the bits is not zero.
 * len[b * nsub + j] (uint32) is the longest lane's count, off[b * nsub + j] (uint64) the exclusive prefix sum of len in
 * ENTRY ROWS.  An entry row is 64 x 16 bytes of samples (the lane's four floats exactly as they lie in the cube, the
 * voxels the mask excludes among them) in d_samples and 64 x 4 bytes of meta (z | nibble << 28) in d_meta, both at row
 * off + k.  Lanes shorter than len, and lanes past the last group, are padded with entries of zero samples and zero
 * meta, which every kernel treats as a plane the mask excludes; every byte of rows [0, sum of len) is written.
 * There is a list only for nz < 2^28, 16-byte lanes (what spc_mask_pack_bits asks for, and a cube whose address and
 * strides are multiples of 4 elements) and the mask-first march (SPC_MOMENTS_MASK_FIRST not 0).
 *   spc_moments_list_plan_f32   (host only, no device) fills desc with the plan spc_moments_list_f32 would launch for
 *       these arguments, after its workspace fallback; SPC_ERR_UNSUPPORTED where there is no list.
 *   spc_moments_list_count_f32  the same desc, and one kernel that reads ONLY the bits: d_len[b * nsub + j] as above and
 *       d_lines[b * nsub + j] = the 128-byte cube lines the bits march fetches for that sublist (the non-zero 32-bit
 *       words of its bits rows).  nsublists = entries of d_len and of d_lines, at least nblocks * nsub.
 *   spc_moments_list_fill_f32   one wave per sublist marches its planes mask-first through the cube (with the strides
 *       the call sees) and writes list->d_samples / d_meta from list->d_off / d_len, padding included.  Nothing is
 *       written past row list->rows or past a sublist's len, whatever d_off / d_len hold.
 *   spc_moments_list_f32        spc_moments_bits_f32 plus the list (NULL: exactly spc_moments_bits_f32).  The list is
 *       read only if the call's plan equals list->desc, the bits are read, the buffers are large enough for
 *       list->rows and SPC_MOMENTS_LIST is not 0; in every other case the call is spc_moments_bits_f32.  The maps are
 *       bit-identical either way: a lane's included planes are added in the order of the march, and the planes left
 *       out only added +0.0.
 * The caller answers for the list being that of the cube's and the mask's present bytes: count and fill again after
 * either changes.  (Added within ABI 8: nothing existing moved.) */
typedef struct {
    int32_t zw, nsplit;          /* waves per block (1, 4, 8) and z ranges of the launch plan */
    int64_t zchunk;              /* planes per z range */
    int64_t nblocks;             /* ceil(ny * (nx / 4) / 64) */
    int64_t nsub;                /* sublists per block: nsplit * zw */
} spc_moments_list_desc;
typedef struct {
    spc_moments_list_desc desc;
    void* d_samples; size_t samples_bytes;       /* rows * 1024 bytes, 16-byte aligned */
    void* d_meta; size_t meta_bytes;             /* rows * 256 bytes */
    const uint64_t* d_off; const uint32_t* d_len; size_t nsublists;   /* >= desc.nblocks * desc.nsub entries each */
    uint64_t rows;               /* sum of len */
} spc_moments_list;
int spc_moments_list_plan_f32(const spc_cube_f32* cube, const spc_mask* mask, const spc_moment_outputs* out,
                              const void* d_workspace, size_t workspace_bytes, spc_moments_list_desc* desc);
int spc_moments_list_count_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                               const spc_moment_outputs* out, const void* d_workspace, size_t workspace_bytes,
                               const void* d_mask_bits, size_t bits_bytes, uint32_t* d_len, uint32_t* d_lines,
                               size_t nsublists, spc_moments_list_desc* desc);
int spc_moments_list_fill_f32(int device, void* stream, const spc_cube_f32* cube, const void* d_mask_bits,
                              size_t bits_bytes, const spc_moments_list* list);
int spc_moments_list_f32(int device, void* stream, const spc_cube_f32* cube,
                         const spc_mask* mask, const double* d_cen, double dv,
                         double m1_add, const spc_moment_outputs* out,
                         void* d_workspace, size_t workspace_bytes,
                         const void* d_mask_bits, size_t bits_bytes, const spc_moments_list* list);

/* One tier above the list: the VOXEL list, one 8-byte entry per included voxel, made FROM a list (above) for the same
 * launch plan and the same sublists (block, split * zw + w); it reuses the list's desc.  Where the mask keeps about one
 * voxel of a lane segment, an entry row of the list carries 16 sample bytes of which four are needed; the voxel list
 * carries those four.
 * Layout: an entry is { float v; uint32_t meta; } with meta = z | col << 28 | 1u << 30: z < 2^28 the plane, col in 0..3 the
 * voxel's place in the lane's 16-byte segment, bit 30 "an entry".  A lane's entries are the voxels whose bit is set in the
 * nibbles of its list entries, in the list's order and in ascending col within a list entry, which keeps every column's
 * samples in the order of the march.  An entry row is 64 lanes x 8 bytes = 512 bytes.  vlen[sub] (uint32, d_len) is the
 * longest lane's count, voff[sub] (uint64, d_off) its exclusive prefix sum in rows.  Shorter and dead lanes are padded
 * with written all-zero entries (bit 30 clear); every byte of rows [0, sum of vlen) is written.
 *   spc_moments_vlist_count_f32  one wave per sublist reads ONLY the list's metas: d_vlen[sub] = the maximum over the
 *       lanes of the sum of popcount(meta >> 28) over the sublist's rows.  nsublists = entries of d_vlen, at least
 *       list->desc.nblocks * list->desc.nsub.
 *   spc_moments_vlist_fill_f32   one wave per sublist walks the list's rows and stores every included voxel's entry at its
 *       lane's own running row of vlist->d_entries, then pads.  It reads neither the cube nor the bits: the list is the
 *       cube's snapshot already.  vlist->desc must equal list->desc.  Nothing is written past row vlist->rows or past a
 *       sublist's vlen, and nothing is read past row list->rows, whatever the offsets and lengths hold.
 *   spc_moments_vlist_f32        spc_moments_list_f32 plus the voxel list (NULL: exactly spc_moments_list_f32).  The voxel
 *       list is read only if the call's final plan equals vlist->desc, the bits are read (as the list asks), the buffers
 *       hold vlist->rows, neither SPC_MOMENTS_VLIST nor SPC_MOMENTS_LIST is 0; in every other case the call is
 *       spc_moments_list_f32.  Where the voxel list is read, `list` is not looked at: it may be NULL or stale,
 *       and the voxel list is read whatever it holds.  The maps are bit-identical either way: per column the included
 *       samples are added in the order of the march, and everything else only adds +0.0.
 * The caller answers for the voxel list being that of the list it was made from.  (Added within ABI 8: nothing existing
 * moved.) */
typedef struct {
    spc_moments_list_desc desc;
    void* d_entries; size_t entries_bytes;       /* rows * 512 bytes, 8-byte aligned */
    const uint64_t* d_off; const uint32_t* d_len; size_t nsublists;   /* >= desc.nblocks * desc.nsub entries each */
    uint64_t rows;               /* sum of vlen */
} spc_moments_vlist;
int spc_moments_vlist_count_f32(int device, void* stream, const spc_moments_list* list, uint32_t* d_vlen, size_t nsublists);
int spc_moments_vlist_fill_f32(int device, void* stream, const spc_moments_list* list, const spc_moments_vlist* vlist);
int spc_moments_vlist_f32(int device, void* stream, const spc_cube_f32* cube,
                          const spc_mask* mask, const double* d_cen, double dv,
                          double m1_add, const spc_moment_outputs* out,
                          void* d_workspace, size_t workspace_bytes,
                          const void* d_mask_bits, size_t bits_bytes, const spc_moments_list* list,
                          const spc_moments_vlist* vlist);

/* general order N >= 2 second pass:  out = sum v*(c - mu)^N / S0
 * (dask_spectral_cube.py:1094-1099; _moments.py:185-193).  d_mu, d_s0 come
 * from spc_moments_f32. */
int spc_moment_order_f32(int device, void* stream, const spc_cube_f32* cube,
                         const spc_mask* mask, const double* d_cen, int order,
                         const double* d_mu, const double* d_s0, double* d_out,
                         int64_t out_row_stride);

/* ---- float64 cubes: moments along the spectral axis in the SOURCE's precision ------------------
 * The reference keeps a float64 source in float64 (np.result_type(dtype, 0.0), spectral_cube/masks.py:225; a
 * BITPIX = -64 / 32 / 64 FITS image arrives as float64 through astropy, io/fits.py:63-172) and so are its moment maps
 * (spectral_cube/_moments.py:30-193, dask_spectral_cube.py:1083-1104).  Same arguments and outputs as spc_moments_f32 /
 * spc_moment_order_f32 with 8-byte samples, float64 thresholds and float64 extrema; no workspace.  There is no d_m2:
 * moment 2 is spc_moment_order_f64(order = 2) about the first pass's d_mu - the reference's own two-pass form
 * (_moments.py:185-193), which keeps float64 precision where S2 / S0 - mu^2 would not.  nz < 2^21. */
typedef struct {
    const double* d_data;
    int64_t nz, ny, nx;
    int64_t row_stride;          /* elements */
    int64_t plane_stride;        /* elements */
} spc_cube_f64;

typedef struct {
    uint32_t flags;              /* SPC_MASK_* */
    double thr_lo;
    double thr_hi;
    const uint8_t* d_array;
    int64_t row_stride;          /* elements; 0 = same as the cube's */
    int64_t plane_stride;        /* elements; 0 = same as the cube's */
} spc_mask_f64;

typedef struct {
    double* d_m0; double* d_m1;                 /* (ny,nx) float64 */
    double* d_mu;      /* S1/S0 without m1_add (input of spc_moment_order_f64) */
    double* d_s0;      /* raw S0 */
    int64_t* d_argmax; int64_t* d_argmin;       /* (ny,nx) int64 */
    double* d_vmax; double* d_vmin;             /* max/min over valid voxels (NaN if none) */
    int32_t* d_nvalid;
    int64_t out_row_stride;                     /* elements; 0 = nx */
} spc_moment_outputs_f64;

int spc_moments_f64(int device, void* stream, const spc_cube_f64* cube,
                    const spc_mask_f64* mask, const double* d_cen, double dv,
                    double m1_add, const spc_moment_outputs_f64* out);

int spc_moment_order_f64(int device, void* stream, const spc_cube_f64* cube,
                         const spc_mask_f64* mask, const double* d_cen, int order,
                         const double* d_mu, const double* d_s0, double* d_out,
                         int64_t out_row_stride);

/* ---- the other operators for float64 cubes (ABI 8) ---------------------------
 * The reference keeps a float64 source in float64 through every operator (np.result_type(dtype, 0.0),
 * spectral_cube/masks.py:225; the Dask class keeps the chunk dtype, dask_spectral_cube.py:829).  Same semantics and
 * arithmetic as the float32 entry points of the same name - astropy's convolve (float64 top / bot, one division),
 * scipy's interp1d slope form, nansum_allbadtonan - without the rounding of samples or results to float32; mask
 * thresholds are compared in float64.  Plain HBM streams, not tuned like the float32 kernels.
 *   spc_stats_global_f64: h_stats (HOST, 5 doubles) = {npts, min, max, sum, sumsq} (dask_spectral_cube.py:769-814);
 *                         synchronises the stream.  Workspace SPC_WS_STATS_GLOBAL_F64.
 *   spc_stats_axis_f64:   maps with the reduced axis removed, (ny,nx) / (nz,nx) / (nz,ny); NULL outputs are skipped; a
 *                         ray without an included sample gives count 0 and NaN (:641-767).
 *   spc_spectral_conv_f64 / spc_spatial_conv_f64: spectral_smooth / spatial_smooth (:880-917, :962-993); host taps.
 *                         spatial: separable != 0 takes the two factors h_ky (nky) and h_kx (nkx) of an outer-product
 *                         kernel; separable == 0 takes h_ky = the (nky, nkx) table, row-major, and ignores h_kx.
 *   spc_spectral_lerp_f64: spectral_interpolate (:1342-1353), the plan of spc_spectral_lerp_f32.
 *   spc_narrow_f64_to_f32: the float32 copy of a float64 cube (what an operator without a float64 form is given).
 *   spc_mask_include_f64: spc_mask_include_u8 on a float64 cube. */
typedef struct spc_stats_outputs_f64 {
    int32_t* d_count;
    double* d_min;
    double* d_max;
    double* d_sum;
    double* d_sumsq;
} spc_stats_outputs_f64;
int spc_stats_global_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask,
                         double* h_stats, void* d_workspace, size_t workspace_bytes);
int spc_stats_axis_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask,
                       int axis, const spc_stats_outputs_f64* out);
int spc_spectral_conv_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask,
                          const double* h_kernel, int ntaps, double* d_out, int64_t out_row_stride,
                          int64_t out_plane_stride, void* d_workspace, size_t workspace_bytes);
int spc_spatial_conv_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask,
                         const double* h_ky, int nky, const double* h_kx, int nkx, int separable,
                         double* d_out, int64_t out_row_stride, int64_t out_plane_stride,
                         void* d_workspace, size_t workspace_bytes);
int spc_spectral_lerp_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask,
                          int64_t nz_out, const int32_t* d_lo, const double* d_t, const double* d_inv_dx,
                          double fill, double* d_out, int64_t out_row_stride, int64_t out_plane_stride);
/* spc_resample_bilinear_f32 on a float64 cube: float64 weights and results (reproject_interp computes in float64), gather
 * form; spc_scale_f64: d_data[i] *= factor (the Jy/beam area ratio of convolve_to, dask_spectral_cube.py:1445-1464). */
int spc_resample_bilinear_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask,
                              double fill, int64_t ny_out, int64_t nx_out, const double* d_xs, const double* d_ys,
                              double* d_out, int64_t out_row_stride, int64_t out_plane_stride,
                              uint8_t* d_footprint, int order, uint32_t* d_any_valid);
int spc_scale_f64(int device, void* stream, double* d_data, int64_t n, double factor);
/* Order statistics of float64 rays along the first axis of the view (spc_percentile_axis0_f32 / spc_sigma_clip_axis0_f32 on the
 * float64 samples; dask_spectral_cube.py:657-731, :851-878): q-th percentile with numpy's linear rule (q = 50: the median, the
 * mean of two middle samples), of |x - d_center| when d_center (a (ny,nx) float64 map) is given, times scale (mad_std); and the
 * whole sigma-clip loop for centre = median | mean and spread = std | mad_std (float64 centre and bounds; d_out (nz,ny,nx) C-contiguous
 * float64, masked and clipped samples NaN).  Rays of up to 4096 samples (sorted in LDS), else SPC_ERR_UNSUPPORTED. */
int spc_percentile_axis0_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask,
                             double q, const double* d_center, double scale, double* d_out);
int spc_sigma_clip_axis0_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask,
                             double sigma_lower, double sigma_upper, int maxiters, int center_is_mean,
                             int spread_is_mad, double* d_out);
int spc_narrow_f64_to_f32(int device, void* stream, const spc_cube_f64* cube, float* d_out,
                          int64_t out_row_stride, int64_t out_plane_stride);
int spc_mask_include_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask,
                         int nan_excluded, uint8_t* d_out);

/* ---- block downsampling along one axis (SpectralCube.downsample_axis, spectral_cube.py:3421-3557) ----
 * The in-memory form (use_memmap=False, :3466-3497) in one pass: along `axis` (0 = spectral, 1 = y, 2 = x) every run of
 * `factor` samples of the FILLED data (masked voxels -> fill) becomes one output sample, estimator(run), and one mask
 * byte, any(include) over the run's real voxels (:3491-3495).  A last run shorter than `factor` is dropped when
 * truncate != 0 (:3468-3473), otherwise it is padded with NaN as the reference pads it (:3474-3480): the nan-estimators
 * skip the padding, SPC_DS_MEAN / SUM / MAX / MIN give NaN for that run.  Output length ceil(n / factor), or
 * floor(n / factor) when truncating (at least one, else SPC_ERR_INVALID).
 * Sums are carried in float64 with an integer count and rounded once to the sample type (nanmean = sum / count, NaN
 * when the count is 0; nansum of nothing = 0); extrema are compared in the sample type; the non-nan estimators return
 * NaN when any sample of the run is NaN.
 * nan_excluded != 0: a NaN sample counts as excluded whatever the mask terms say - what a ~isnan mask of the cube's own
 * data means (NotNaNMask, the mask spectral_interpolate attaches, lowers to no term: a reduction skips NaN anyway, but
 * here excluded voxels become `fill` and drop out of the include map).
 * d_out: the output view, strides in elements (0 = C-contiguous), so that strips of a larger output are written in
 * place; d_out_mask (uint8, written as 0 / 1; may be NULL) has the same strides.  Every input byte is read once, with 16-byte
 * loads (4-byte for the mask array) when every input row and plane starts 16-byte aligned - for axes 0 / 1 the outputs'
 * rows and planes as well, for axis 2 with factor > 512 a factor that is a multiple of 4 samples - and with one load
 * per sample otherwise (e.g. float32 rows with nx % 4 != 0).  No workspace. */
typedef enum {
    SPC_DS_NANMEAN = 0, SPC_DS_NANSUM = 1, SPC_DS_NANMAX = 2, SPC_DS_NANMIN = 3,
    SPC_DS_MEAN = 4, SPC_DS_SUM = 5, SPC_DS_MAX = 6, SPC_DS_MIN = 7
} spc_ds_estimator;
int spc_downsample_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded,
                       float fill, int axis, int64_t factor, int truncate, int estimator,
                       float* d_out, int64_t out_row_stride, int64_t out_plane_stride, uint8_t* d_out_mask);
int spc_downsample_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded,
                       double fill, int axis, int64_t factor, int truncate, int estimator,
                       double* d_out, int64_t out_row_stride, int64_t out_plane_stride, uint8_t* d_out_mask);

/* ---- cutting a cube (SpectralCube.__getitem__, spectral_cube.py:1308-1381; spectral_slab :1823-1879; subcube :1947-2036) ----
 * Gathers a view of the parent into a compact cube, data and mask in one pass: output sample (k, j, i) is parent sample
 * (start[0] + k * step[0], start[1] + j * step[1], start[2] + i * step[2]).  start / step are HOST arrays of 3 int64 in
 * numpy axis order (spectral, y, x); step != 0, a negative step walks downwards from start; every selected sample must
 * lie inside the parent and every output length be >= 1 (there is no zero-size form), else SPC_ERR_INVALID.
 * filled == 0: the samples are copied bit for bit (the new cube's unmasked data, NaN payloads included); filled != 0:
 * `fill` is written where the voxel is excluded (the FILLED 2-D / 1-D results of integer indices, :1362-1370).
 * d_out_mask (uint8, may be NULL): include of the parent's lowered mask at the source voxel, with the nan_excluded rule
 * of spc_downsample_*, written as 0 / 1 (the byte of the parent's array is evaluated, not copied).  d_out / d_out_mask
 * share the output strides (elements, 0 = C-contiguous), so that strips of a larger result are written in place.  Only selected rows are addressed: skipped planes and rows are never read.
 * Along x a step of 1 uses 16-byte loads and stores (4-byte for the mask bytes) when the selected source rows, start[2]
 * and the output rows are 16-byte aligned, one load per sample otherwise; any other x step one load per selected sample.
 * Launches are split inside: no limit on any axis.  No workspace. */
int spc_subcube_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded,
                    const int64_t* start, const int64_t* step, int64_t nz_out, int64_t ny_out, int64_t nx_out,
                    float* d_out, int64_t out_row_stride, int64_t out_plane_stride, uint8_t* d_out_mask,
                    int filled, float fill);
int spc_subcube_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded,
                    const int64_t* start, const int64_t* step, int64_t nz_out, int64_t ny_out, int64_t nx_out,
                    double* d_out, int64_t out_row_stride, int64_t out_plane_stride, uint8_t* d_out_mask,
                    int filled, double fill);

/* ---- bounding box of a mask (subcube_slices_from_mask / minimal_subcube, spectral_cube.py:1881-1945) ----
 * What ndimage.find_objects(include.astype(int))[0] returns at :1925-1938: d_box (6 int64 in device memory, 8-byte
 * aligned) receives {zmin, zmax, ymin, ymax, xmin, xmax} of the included voxels, bounds inclusive.  The entry point
 * initialises it on the stream; a mask that includes nothing leaves min > max (INT64_MAX, -1).  The samples are read
 * only when a predicate term or nan_excluded needs them: a pure array mask costs one byte per voxel.  Bounds are reduced
 * per wave and per block before one atomicMin / atomicMax per block and bound.  The caller reads d_box after the stream
 * has drained.  No workspace. */
int spc_mask_bbox_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded,
                      int64_t* d_box);
int spc_mask_bbox_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded,
                      int64_t* d_box);

/* ---- position-velocity diagrams: the spectrum at every point of a path on the sky ----
 * Replaces SpectralCube.to_pvextractor (spectral_cube.py:2506-2513: the hand-over to pvextractor.extract_pv_slice(cube,
 * path), which pulls the cube to the host) and the axis-aligned cube[:, j, :] Slice: d_out[k, p] (nz x npts, the cube's
 * dtype, out_row_stride elements between channels, 0 = npts) is the mean over nlines parallel lines of the FILLED cube
 * interpolated at the pixel position (d_xs[l * npts + p], d_ys[l * npts + p]) (device arrays of nlines x npts float64,
 * 0-based) of channel k.  The cube is read in place (any view spc_check_cube accepts); there is no workspace and no
 * (nz, nlines, npts) intermediate.
 *   sample: the cube's value where the mask includes the voxel, `fill` where it does not (nan_excluded: the rule of
 *     spc_subcube_*, a NaN sample counts as excluded).  The mask byte is read first; an excluded sample is not fetched
 *     (a predicate term needs the sample and fetches it).
 *   domain: a point is inside when 0 <= x <= nx - 1 and 0 <= y <= ny - 1, anything else (-1e-9, nx - 1 + 1e-9, NaN)
 *     gives NaN: scipy.ndimage.map_coordinates(mode='constant', cval=nan).
 *   order 0: the sample at (floor(y + 0.5), floor(x + 0.5)); with one line and respect_nan it is copied bit for bit.
 *   order 1: x0 = floor(x), fx = x - x0 (likewise y); the weights (1-fy)(1-fx), (1-fy)fx, fy(1-fx), fy fx of the
 *     neighbours (y0, x0), (y0, x0+1), (y0+1, x0), (y0+1, x0+1) in float64.  A neighbour whose weight is exactly 0 is not
 *     read and does not count (x = nx - 1 is inside: its right-hand neighbours weigh 0).  The line's value is
 *     0 + w v + w v ... in float64 in that order, each product and each sum rounded on its own (no fused multiply-add).
 *   respect_nan != 0: the line's value is NaN when a neighbour of non-zero weight is NaN; == 0: such a neighbour adds
 *     0 (at order 0 a NaN sample becomes 0, as map_coordinates on nan_to_num'd data gives).
 *   width: d_out = (v_0 + v_1 + ...) / n over the n lines whose value is not NaN, added in line order in float64 and
 *     rounded once to the cube's dtype; NaN when n = 0.  No atomics: the same call gives the same bits.
 *   d_count (int32, nz x npts, count_row_stride elements between channels, 0 = npts; may be NULL): n.
 * Lanes run along the path, blocks split the channels in batches whose loads are issued together; launches cover any
 * npts and nz.  SPC_ERR_INVALID for npts < 1, nlines < 1, an order other than 0 / 1, NULL arrays, strides below npts. */
int spc_pv_extract_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded, float fill,
                       int64_t npts, int64_t nlines, const double* d_xs, const double* d_ys, int order, int respect_nan,
                       float* d_out, int64_t out_row_stride, int32_t* d_count, int64_t count_row_stride);
int spc_pv_extract_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded, double fill,
                       int64_t npts, int64_t nlines, const double* d_xs, const double* d_ys, int order, int respect_nan,
                       double* d_out, int64_t out_row_stride, int32_t* d_count, int64_t count_row_stride);

/* ---- polynomial baselines: fit every spectrum on its line-free channels, subtract the model ----
 * The step docs/continuum_subtraction.rst does for a constant (mask the line channels, median(axis=0), subtract) and
 * apply_function_parallel_spectral (spectral_cube.py:3103) does for anything else by handing every spectrum to a
 * Python function on the host (CASA: imcontsub fitorder=n).  Two entries: the fit, a masked streaming reduction along z
 * into a small normal-equation system per spaxel, and the apply, one element-wise pass.
 *   abscissa: the channel index mapped to [-1, 1], t_k = (2k - (nz - 1)) / (nz - 1); t_0 = 0 when nz == 1.
 *   basis: Legendre, P_0 ... P_p with p = order, 0 <= order <= SPC_BASELINE_MAX_ORDER.  The CALLER computes the table
 *     d_basis[k * (p + 1) + j] = P_j(t_k) for all nz channels in float64 (numpy.polynomial.legendre.legvander(t, p)) and
 *     uploads it; the device never recomputes a basis value.  (A power basis in the channel number has a Gram matrix of
 *     condition 4e24 at nz = 257, order 5; Legendre's is 11.)
 *   fit set of spectrum (y, x): every channel k that is in the channel list (d_channels: nfit int32 channel numbers in
 *     increasing order; NULL: all channels, nfit == nz), whose voxel (k, y, x) the mask includes and whose sample is not
 *     NaN; n is its size.  Channels outside the list are not read, neither their mask bytes nor their samples (a list
 *     entry outside 0 ... nz - 1 is skipped).  Inside the list the mask byte is read first and an excluded sample is not
 *     fetched (a predicate term needs the sample and fetches it): the include-array rule above.
 *   solve: G_ij = sum P_i(t_k) P_j(t_k) and b_i = sum P_i(t_k) v_k over the fit set, in float64 for float32 cubes too,
 *     added in list order from 0, each product and each sum rounded on its own (no fused multiply-add).  A long list is
 *     cut into spc_baseline_segments() segments of ceil(nfit / segments) list entries, each summed from 0 on its own, and
 *     the segments are added in index order: the result depends on the shape and nfit only, never on timing.
 *     n >= p + 1: c = G^-1 b by the root-free Cholesky factorisation G = L D L^T in float64, in this order -
 *       D_j = G_jj - sum_{k<j} L_jk (L_jk D_k);  L_ij = (G_ij - sum_{k<j} L_ik (L_jk D_k)) / D_j   (i > j; k ascending)
 *       z_i = b_i - sum_{k<i} L_ik z_k;  w_i = z_i / D_i;  c_i = w_i - sum_{k>i} L_ki c_k          (i descending, k ascending)
 *     n < p + 1, or a pivot D_j that is not > 0: all p + 1 coefficients are NaN.
 *   outputs of the fit: d_coef float64 (p + 1, ny, nx) contiguous; d_npts int32 (ny, nx) contiguous, n; may be NULL.
 *   apply: model_k = c_0 P[k,0] + c_1 P[k,1] + ... + c_p P[k,p], added in that order in float64, for EVERY channel and
 *     every voxel of the cube whatever any mask says (as cube - map treats the unmasked data).  mode 0: d_out =
 *     (T)((double)v - model) - a NaN sample stays NaN; mode 1: d_out = (T)model, the cube's samples are not read.  NaN
 *     coefficients give a NaN spectrum in both modes.  d_out has the cube's shape and its own strides (0 = contiguous).
 *   No atomics: two identical calls give identical bits.
 * Lanes run along x, each owns a spaxel and keeps its (p+1)(p+2)/2 + (p+1) float64 sums in registers (the kernels are
 * templated on the order); a batch of channels' mask bytes is loaded, then the included samples, then the arithmetic.
 * With more than one segment the partial sums go to d_workspace (spc_baseline_workspace_bytes(); 0 bytes for one
 * segment) and a second small kernel adds them and solves.  Launches cover any ny, nx, nz.  Outputs and workspace may
 * hold anything.  SPC_ERR_INVALID for an order outside 0 ... 5, NULL arrays, nfit < 1, nfit != nz without a list, bad
 * strides, a mode other than 0 / 1, and outputs or workspace that overlap an input or each other. */
#define SPC_BASELINE_MAX_ORDER 5
int64_t spc_baseline_segments(int64_t nz, int64_t ny, int64_t nx, int64_t nfit);
size_t spc_baseline_workspace_bytes(int64_t nz, int64_t ny, int64_t nx, int64_t nfit, int order);
int spc_baseline_fit_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int order,
                         const int32_t* d_channels, int64_t nfit, const double* d_basis, double* d_coef, int32_t* d_npts,
                         void* d_workspace, size_t workspace_bytes);
int spc_baseline_fit_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int order,
                         const int32_t* d_channels, int64_t nfit, const double* d_basis, double* d_coef, int32_t* d_npts,
                         void* d_workspace, size_t workspace_bytes);
int spc_baseline_apply_f32(int device, void* stream, const spc_cube_f32* cube, int order, const double* d_basis,
                           const double* d_coef, int mode, float* d_out, int64_t out_row_stride, int64_t out_plane_stride);
int spc_baseline_apply_f64(int device, void* stream, const spc_cube_f64* cube, int order, const double* d_basis,
                           const double* d_coef, int mode, double* d_out, int64_t out_row_stride, int64_t out_plane_stride);

/* ---- mask expressions evaluated once on the device (masks.py:239-250 composition, :399-455 CompositeMask / InvertedMask,
 * :670-758 LazyComparisonMask) ----
 * A mask tree that is not an AND of spc_mask terms - a threshold that is a map, a spectrum or a cube, `|` `^` `~`, == and
 * !=, terms on several cubes - is compiled by the host into a postfix program; one kernel runs it over the cube and writes
 * the uint8 include array (1 / 0), which every other entry point then takes as SPC_MASK_ARRAY.
 *   data slots: the cubes comparison terms read, all (nz, ny, nx) samples of the entry point's type (float for _f32, double
 *     for _f64); strides in elements, 0 = C-contiguous.  Only z * plane_stride + y * row_stride + x is ever formed, so the
 *     views of rows / planes / exchanged first axes are accepted.
 *   operands: arrays a term is compared with or loaded from: float, double or uint8 elements and one ELEMENT stride per
 *     axis, 0 = broadcast along that axis (a (ny, nx) map has stride_z 0, a spectrum stride_y = stride_x = 0).
 *   instructions, postfix, over a stack of include bits:
 *     SPC_MOP_CMP     push  slot[slot] <cmp> (operand >= 0 ? operands[operand] : imm); a uint8 operand is invalid
 *     SPC_MOP_FINITE  push  isfinite(slot[slot])
 *     SPC_MOP_LOAD    push  operands[operand] != 0; the operand must be uint8
 *     SPC_MOP_NOT     negate the top;  SPC_MOP_AND / _OR / _XOR  pop two, push the result
 * A comparison converts the sample to double (exact) and compares it with the double threshold under IEEE rules: a NaN
 * on either side is false, true for SPC_CMP_NE - numpy's result for a Python scalar rounded to the sample type by the
 * host, a typed scalar, and bool / integer / float16 / float32 / float64 arrays (all but float32 converted to float64).
 * The program travels as kernel arguments: wave-uniform, the interpreter loop does not diverge.  A lane owns 4 consecutive
 * x: slots and unit-stride operands are read with 16-byte loads and the 4 include bytes leave in one 4-byte store wherever
 * a row's addresses allow, sample by sample at the ends of a row and in rows that are not aligned; every slot is read once
 * however many terms name it.  No LDS, no atomics, no workspace; launches are split inside: no limit on any axis.
 * SPC_ERR_INVALID, before anything is queued and with d_out untouched: a NULL pointer, a count beyond the limits below, an
 * unknown opcode / comparison / element type, a slot or operand index out of range, a float operand under SPC_MOP_LOAD or
 * a uint8 one under SPC_MOP_CMP, a stack that underflows or grows past SPC_MASK_PROG_MAX_STACK, a program that does not
 * leave exactly one value.  d_out: uint8, strides in elements (0 = C-contiguous). */
#define SPC_MASK_PROG_MAX_SLOTS    4
#define SPC_MASK_PROG_MAX_OPERANDS 8
#define SPC_MASK_PROG_MAX_INSTR    16
#define SPC_MASK_PROG_MAX_STACK    8
typedef enum {
    SPC_MOP_CMP = 0, SPC_MOP_FINITE = 1, SPC_MOP_LOAD = 2, SPC_MOP_NOT = 3, SPC_MOP_AND = 4, SPC_MOP_OR = 5, SPC_MOP_XOR = 6
} spc_mask_opcode;
typedef enum {
    SPC_CMP_GT = 0, SPC_CMP_GE = 1, SPC_CMP_LT = 2, SPC_CMP_LE = 3, SPC_CMP_EQ = 4, SPC_CMP_NE = 5
} spc_mask_cmp;
typedef enum { SPC_ELEM_F32 = 0, SPC_ELEM_F64 = 1, SPC_ELEM_U8 = 2 } spc_mask_elem;
typedef struct {
    const void* d_data;          /* float (_f32) or double (_f64) samples of a (nz, ny, nx) cube */
    int64_t row_stride;          /* elements; 0 = nx */
    int64_t plane_stride;        /* elements; 0 = ny * row_stride */
} spc_mask_slot;
typedef struct {
    const void* d_data;
    int32_t elem;                /* spc_mask_elem */
    int32_t reserved;
    int64_t stride_z, stride_y, stride_x;   /* elements, >= 0; 0 = broadcast along that axis */
} spc_mask_operand;
typedef struct {
    int32_t opcode;              /* spc_mask_opcode */
    int32_t slot;                /* CMP, FINITE */
    int32_t cmp;                 /* CMP: spc_mask_cmp */
    int32_t operand;             /* CMP: operand index, or -1 = compare with imm; LOAD: operand index */
    double imm;
} spc_mask_instr;
typedef struct {
    int32_t n_slots, n_operands, n_instr, reserved;
    spc_mask_slot slots[SPC_MASK_PROG_MAX_SLOTS];
    spc_mask_operand operands[SPC_MASK_PROG_MAX_OPERANDS];
    spc_mask_instr instr[SPC_MASK_PROG_MAX_INSTR];
} spc_mask_program;
int spc_mask_eval_f32(int device, void* stream, int64_t nz, int64_t ny, int64_t nx, const spc_mask_program* prog,
                      uint8_t* d_out, int64_t out_row_stride, int64_t out_plane_stride);
int spc_mask_eval_f64(int device, void* stream, int64_t nz, int64_t ny, int64_t nx, const spc_mask_program* prog,
                      uint8_t* d_out, int64_t out_row_stride, int64_t out_plane_stride);

/* ---- binary morphology of an include array: erosion, dilation, and either one repeated to its fixed point ----
 * What users of the reference do on the host with scipy.ndimage.binary_erosion / binary_dilation / binary_propagation on
 * cube.get_mask_array() (spectral_cube.py:552), here on the uint8 include array where it lives.  d_in (and d_mask, or NULL)
 * are (nz, ny, nx) uint8 arrays, any non-zero byte = True, strides in elements (0 = C-contiguous; only z * plane_stride +
 * y * row_stride + x is formed, so rows / planes views are accepted); d_out is (nz, ny, nx) uint8, C-contiguous, written
 * with 0 / 1, and may not overlap d_in or d_mask.
 * The structuring element travels as a HOST list of noffsets triples (dz, dy, dx) of int8, each component within
 * +-SPC_MORPH_MAX_REACH: the offsets index - size / 2 of its True entries, scipy's centre for even and odd extents alike.
 * With samples outside the array equal to border_value (0 or 1), one step is
 *     op = SPC_MORPH_DILATE:  r[p] = OR  over the offsets o of in[p - o]
 *     op = SPC_MORPH_ERODE:   r[p] = AND over the offsets o of in[p + o]
 *     out[p] = mask ? (mask[p] ? r[p] : in[p]) : r[p]
 * iterations >= 1: exactly that many synchronous steps, each on the result of the one before.  iterations < 1: until a
 * step changes nothing.  Dilation to the fixed point under a mask (binary_propagation) is the least fixed point of a
 * monotone operator and does not depend on the order of the updates, so it is swept in place: a block settles its tile
 * in LDS before it publishes it and the sweeps end when one leaves a device-side change word at 0; the host reads that
 * word (4 bytes) after every batch of sweeps, the one synchronisation of these calls.  *h_iterations_run (optional)
 * receives the number of steps / sweeps run; it is not part of the result.  The repetition of a structure WITHOUT its
 * centre is not monotone and stays synchronous; it may cycle for ever (in scipy too): SPC_ERR_UNSUPPORTED after 65536 steps.
 * The voxels are packed to one bit each, 32 consecutive x to a word, rows padded to a word; every step runs on two packed
 * buffers in the workspace and the bytes are written once, at the end.  d_workspace: the number of bytes the query below
 * returns for the same shape.  SPC_ERR_INVALID before any device work: a NULL pointer, a shape that is not positive, a
 * stride too small, noffsets outside 1 ... SPC_MORPH_MAX_OFFSETS, an offset beyond the reach, an unknown op, a
 * border_value that is not 0 or 1, d_out overlapping an input, a workspace too small.  No limit on any axis. */
#define SPC_MORPH_MAX_REACH   3
#define SPC_MORPH_MAX_OFFSETS 343
typedef enum { SPC_MORPH_ERODE = 0, SPC_MORPH_DILATE = 1 } spc_morph_op;
size_t spc_mask_morph_workspace_bytes(int64_t nz, int64_t ny, int64_t nx);
int spc_mask_morph_u8(int device, void* stream, int64_t nz, int64_t ny, int64_t nx,
                      const uint8_t* d_in, int64_t in_row_stride, int64_t in_plane_stride,
                      const uint8_t* d_mask, int64_t mask_row_stride, int64_t mask_plane_stride,
                      int op, const int8_t* h_offsets, int noffsets, int iterations, int border_value,
                      uint8_t* d_out, void* d_workspace, size_t workspace_bytes, int64_t* h_iterations_run);

/* ---- connected components of an include array: labels, sizes and bounding boxes, selection by label ----
 * What users of the reference do on the host with scipy.ndimage.label, np.bincount and scipy.ndimage.find_objects on
 * cube.get_mask_array() (spectral_cube.py:552), here on the uint8 include array where it lives.
 *
 * spc_label_u8: d_in is a (nz, ny, nx) uint8 array, any non-zero byte = True, strides in elements as for
 * spc_mask_morph_u8 (0 = C-contiguous; rows / planes views are read in place).  h_structure: 27 HOST bytes, the 3x3x3
 * structure in C order, any non-zero byte = True.  Two True voxels p and p + o belong together when entry o + (1, 1, 1) is
 * True.  The structure must be centrosymmetric (entry t and entry 26 - t agree for every t; scipy raises on any other):
 * SPC_ERR_INVALID.  Its centre (entry 13) is ignored, an all-False structure makes every True voxel a component of its
 * own: the connectivity is 13 bits, one per pair of opposite neighbours.
 * d_labels: (nz, ny, nx) int32, C-contiguous, not overlapping d_in: 0 for a False voxel, else the number of the voxel's
 * component, 1 ... *h_nlabels, components numbered in raster order of their first voxel (smallest linear index) - the
 * array scipy.ndimage.label(in != 0, structure) returns, numbering included.  *h_nlabels receives the number of
 * components: these 8 bytes and the status are all that reach the host, and the call waits for its stream to read them.
 * The labels are made by a union-find on d_labels itself in a fixed sequence of at most six launches, whatever the shape of the
 * components; nothing is repeated until it settles (csrc/spc_label.hip).  d_workspace: the number of bytes the query
 * returns for the same shape (a few hundred KiB at most); the query is 0 for a shape that is not positive and never
 * decreases when an axis grows.
 * Linear indices are int32: nz * ny * nx > 2^31 - 1 is refused with SPC_ERR_UNSUPPORTED (1024^3 fits).  No other limit on
 * any axis.  SPC_ERR_INVALID before any device work: a NULL pointer, a shape that is not positive, a stride too small,
 * d_labels overlapping d_in, a workspace too small or overlapping an array.
 *
 * spc_label_objects_i32: d_labels as above with labels 0 ... nlabels.  d_sizes: int64[nlabels + 1], d_sizes[k] = the number
 * of voxels with label k, entry 0 the background (np.bincount(labels, minlength = nlabels + 1)).  d_bbox:
 * int32[(nlabels + 1) x 6] = zlo, zhi, ylo, yhi, xlo, xhi of label k with hi exclusive: the slices of
 * scipy.ndimage.find_objects (a label without a voxel keeps lo = INT32_MAX, hi = 0).  The entry initialises both tables.
 * A label outside 0 ... nlabels never indexes the tables: the voxel is skipped and the call returns SPC_ERR_INVALID,
 * through a device flag that is read with the status (the call waits for its stream).  d_workspace holds that flag:
 * SPC_LABEL_OBJECTS_WORKSPACE_BYTES, or what the query above returns, which is never less.
 *
 * spc_label_select_i32: d_out[p] = d_keep[d_labels[p]] != 0, written as 0 / 1; d_keep: uint8[nlabels + 1] on the
 * device (a label outside 0 ... nlabels gives 0).  The table is staged in LDS when it fits.  d_out: (nz, ny, nx) uint8,
 * C-contiguous, overlapping neither d_labels nor d_keep.  Nothing reaches the host.
 *
 * All three: the same shape checks and limit; outputs, tables and workspace may hold anything when the call begins. */
#define SPC_LABEL_OBJECTS_WORKSPACE_BYTES 256
size_t spc_label_workspace_bytes(int64_t nz, int64_t ny, int64_t nx);
int spc_label_u8(int device, void* stream, int64_t nz, int64_t ny, int64_t nx,
                 const uint8_t* d_in, int64_t in_row_stride, int64_t in_plane_stride, const uint8_t* h_structure,
                 int32_t* d_labels, void* d_workspace, size_t workspace_bytes, int64_t* h_nlabels);
int spc_label_objects_i32(int device, void* stream, int64_t nz, int64_t ny, int64_t nx, const int32_t* d_labels, int64_t nlabels,
                          int64_t* d_sizes, int32_t* d_bbox, void* d_workspace, size_t workspace_bytes);
int spc_label_select_i32(int device, void* stream, int64_t nz, int64_t ny, int64_t nx, const int32_t* d_labels, int64_t nlabels,
                         const uint8_t* d_keep, uint8_t* d_out);

/* ---- per-label measurements of a cube: sums, extrema with their positions, first and second moments ----
 * The scipy.ndimage measurement family (sum_labels, mean, variance, minimum, maximum, their positions, center_of_mass)
 * over the labels of spc_label_u8, which users of the reference run on the host on the label array and the cube: one
 * streaming segmented reduction of the cube through its labels; only the per-label tables ever travel.
 *
 * cube: the samples, a strided view is read in place.  mask: the cube's mask, or NULL.  d_labels: (nz, ny, nx) int32,
 * C-contiguous, labels 0 ... nlabels.  d_origin: double[(nlabels + 1) x 4] on the device, v0, z0, y0, x0 of every label,
 * or NULL for all zero.  want: which groups of tables are computed (SPC_MEASURE_*); a group that is not wanted is neither
 * computed nor written and its pointers are not read.
 * A voxel is measured when its label is above 0, the mask includes it and its sample is not NaN; +-inf samples take part
 * as IEEE arithmetic gives.  Label 0, the background, is never measured: entry 0 of every table is that of a label
 * without a measured voxel.  With dz = z - z0, dy = y - y0, dx = x - x0 over the measured voxels of label k:
 *     SPC_MEASURE_SUMS     d_count[k] (int64), d_sums[2 k] = sum (v - v0), d_sums[2 k + 1] = sum (v - v0)^2
 *     SPC_MEASURE_EXTREMA  d_min[k], d_max[k] (the cube's sample type), d_min_pos[k], d_max_pos[k] (int64): the linear
 *                          C-order index of the FIRST minimum / maximum (the smallest index on ties, scipy's
 *                          minimum_position / maximum_position); -0.0 and +0.0 compare equal and a zero extreme is
 *                          written as +0.0; a label without a measured voxel gets NaN and -1
 *     SPC_MEASURE_FIRST    d_first[4 k ...] = sum v, sum v dz, sum v dy, sum v dx
 *     SPC_MEASURE_SECOND   d_second[6 k ...] = sum v dz^2, v dy^2, v dx^2, v dz dy, v dz dx, v dy dx
 * Every sum is accumulated in float64 whatever the cube's type.  Lanes run along x; a wave reduces each run of one label
 * among its 64 voxels before anything leaves it and carries a run that goes on into its next 64 voxels, so a run costs
 * at most one global atomic per quantity (csrc/spc_label_measure.hip).  The sample and the mask byte are fetched only
 * where the label is above 0.  THE ORDER OF THE ATOMIC ADDS IS NOT FIXED: counts, extrema and positions are the same on
 * every call, the float64 sums are reproducible only to float64 rounding, |difference| <= 2 (m - 1) 2^-53 sum |term| for
 * a label of m measured voxels.  (The first floating-point atomics of this library; every other result is bit-stable.)
 * The positions of a float64 cube take a second launch over the labels.
 * The entry initialises every table it writes: tables and workspace may hold anything when the call begins.  A label
 * outside 0 ... nlabels never indexes a table: the voxel is skipped and the call returns SPC_ERR_INVALID through a device
 * flag read with the status (the call waits for its stream); nothing else reaches the host.  d_workspace: what the query
 * returns for the same nlabels and want (the flag, and two 64-bit keys per label for the extrema).
 * Limits as for spc_label_objects_i32: more than 2^31 - 1 voxels SPC_ERR_UNSUPPORTED; SPC_ERR_INVALID before any device
 * work for a NULL pointer of a wanted group, a shape that is not positive, a stride too small, nlabels outside
 * 0 ... 2^31 - 1, want 0 or with an unknown bit, buffers that overlap, a workspace too small. */
#define SPC_MEASURE_SUMS    1u
#define SPC_MEASURE_EXTREMA 2u
#define SPC_MEASURE_FIRST   4u
#define SPC_MEASURE_SECOND  8u
typedef struct {
    int64_t* d_count;      /* SUMS */
    double* d_sums;        /* SUMS: (nlabels + 1) x 2 */
    void* d_min;           /* EXTREMA: float / double (nlabels + 1) */
    void* d_max;
    int64_t* d_min_pos;
    int64_t* d_max_pos;
    double* d_first;       /* FIRST: (nlabels + 1) x 4 */
    double* d_second;      /* SECOND: (nlabels + 1) x 6 */
} spc_label_measure_outputs;
size_t spc_label_measure_workspace_bytes(int64_t nlabels, uint32_t want);
int spc_label_measure_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, const int32_t* d_labels,
                          int64_t nlabels, const double* d_origin, uint32_t want, const spc_label_measure_outputs* out,
                          void* d_workspace, size_t workspace_bytes);
int spc_label_measure_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, const int32_t* d_labels,
                          int64_t nlabels, const double* d_origin, uint32_t want, const spc_label_measure_outputs* out,
                          void* d_workspace, size_t workspace_bytes);

/* ---- rank filters: median / minimum / maximum / percentile / rank over a sliding window ----
 * spectral_smooth_median / spectral_filter (spectral_cube.py:2844-2898, dask_spectral_cube.py:920-960) and
 * spatial_smooth_median / spatial_filter (spectral_cube.py:2749-2806, dask_spectral_cube.py:995-1029) with a filter of
 * scipy.ndimage's rank family: every output sample is element `rank` (0 = smallest) of the sorted window of FILLED
 * samples (masked voxels -> fill; nan_excluded as for spc_downsample_*) around it.  _axis0: a window of `ksize` samples
 * along the spectral axis of every spaxel; _plane: ky x kx samples of every image plane.  As in scipy (origin 0) a
 * window reaches size / 2 samples back and size - 1 - size / 2 forward, so an even size is allowed.
 * mode: how a window is continued past an edge, scipy's names (spc_rank_mode); cval is the sample of SPC_RANK_CONSTANT.
 * NaN ranks LAST, numpy's sort order: the result is np.sort(window)[rank] for every window (scipy's own result with a
 * NaN in the window depends on its version).  The result is one of the window's samples, bit for bit (a NaN result is
 * the quiet NaN; which of -0.0 / +0.0 comes out of a window holding both is by their sign bit).
 * mode SPC_RANK_CONSTANT with a mask: a spaxel (_axis0) / plane (_plane) without one included sample is written as
 * fill, not filtered (_apply_spectral_function / _apply_spatial_function, spectral_cube.py:147-172); a second pass over
 * the input finds them.  In every other mode each input byte is read once per window it is staged for.
 * Limits: ksize 1 ... SPC_RANK_FILTER_MAX_KSIZE, ky / kx 1 ... SPC_RANK_FILTER_MAX_KSIZE_SPATIAL, and a window may
 * reach at most one axis length past an edge (size / 2 <= n), else SPC_ERR_INVALID.  d_out: the output view, strides in
 * elements (0 = C-contiguous), never the input.  Launches are split inside: no limit on any axis.  No workspace. */
typedef enum {
    SPC_RANK_REFLECT = 0, SPC_RANK_CONSTANT = 1, SPC_RANK_NEAREST = 2, SPC_RANK_MIRROR = 3, SPC_RANK_WRAP = 4
} spc_rank_mode;
#define SPC_RANK_FILTER_MAX_KSIZE 129
#define SPC_RANK_FILTER_MAX_KSIZE_SPATIAL 15
int spc_rank_filter_axis0_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded,
                              float fill, int ksize, int rank, int mode, float cval,
                              float* d_out, int64_t out_row_stride, int64_t out_plane_stride);
int spc_rank_filter_axis0_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded,
                              double fill, int ksize, int rank, int mode, double cval,
                              double* d_out, int64_t out_row_stride, int64_t out_plane_stride);
int spc_rank_filter_plane_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded,
                              float fill, int ky, int kx, int rank, int mode, float cval,
                              float* d_out, int64_t out_row_stride, int64_t out_plane_stride);
int spc_rank_filter_plane_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded,
                              double fill, int ky, int kx, int rank, int mode, double cval,
                              double* d_out, int64_t out_row_stride, int64_t out_plane_stride);

/* ---- stack_spectra: Fourier-shift every spectrum by its own number of channels, and stack ----
 * spectral_cube.analysis_utilities: stack_spectra (analysis_utilities.py:134-318), fourier_shift (:14-78) and
 * _fourier_shifter (:81-94).  For each of the npos positions d_idx[p] (int32, the flat spaxel index y * nx + x of the
 * cube view) the FILLED spectrum (masked voxels -> fill; nan_excluded as for the downsample entry points) is zero-padded
 * by pad_lo channels in front and pad_hi behind (M = nz + pad_lo + pad_hi) and shifted by d_shift[p] channels (float64,
 * any sign, fractional) exactly as the reference's fft / phase ramp / ifft does: the circular convolution
 *     out[n] = sum_j x[j] h_M(n - j - s),   h_M(t) = sin(pi t) / (M sin(pi t / M))  (M odd),
 *                                            h_M(t) = sin(pi t) / (M tan(pi t / M))  (M even),   1 where M divides t
 * summed directly in float64 for float32 and float64 cubes alike.  NaN as in fourier_shift (:35-78): non-finite samples
 * count as 0; a spectrum that has some also has its indicator (1 / 0) shifted, and output samples where that exceeds 0.5
 * are NaN; a spectrum without one finite sample, a non-finite shift or a position outside the map gives an all-NaN row.
 *   _shift: d_out (M, npos) float64, C-contiguous, receives the shifted spectra, one per column.
 *   _sum:   the shifted spectra are never written; d_sum[M] receives the sum over the rows that are not NaN at that
 *           channel, d_count[M] their number and d_nan[M] the number of rows that are NaN there (int64 both), from which
 *           the host finishes np.nanmean / np.mean / np.nansum / np.sum.  Partial sums are kept per block in the workspace
 *           and added in a fixed order by a second kernel: no floating-point atomics, the split depends on the sizes
 *           alone, two runs agree bit for bit.
 * M up to SPC_STACK_MAX_CHANNELS, else SPC_ERR_UNSUPPORTED; no limit on npos or on any axis.  d_workspace: the number
 * of bytes the workspace query below returns for the same sizes (fused = 1 for _sum).  Everything is queued on the stream. */
#define SPC_STACK_MAX_CHANNELS 8192
size_t spc_stack_workspace_bytes(int64_t nz, int64_t npos, int pad_lo, int pad_hi, int fused);
int spc_stack_shift_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded, float fill,
                        const int32_t* d_idx, const double* d_shift, int64_t npos, int pad_lo, int pad_hi, double* d_out,
                        void* d_workspace, size_t workspace_bytes);
int spc_stack_shift_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded, double fill,
                        const int32_t* d_idx, const double* d_shift, int64_t npos, int pad_lo, int pad_hi, double* d_out,
                        void* d_workspace, size_t workspace_bytes);
int spc_stack_sum_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded, float fill,
                      const int32_t* d_idx, const double* d_shift, int64_t npos, int pad_lo, int pad_hi, double* d_sum,
                      int64_t* d_count, int64_t* d_nan, void* d_workspace, size_t workspace_bytes);
int spc_stack_sum_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded, double fill,
                      const int32_t* d_idx, const double* d_shift, int64_t npos, int pad_lo, int pad_hi, double* d_sum,
                      int64_t* d_count, int64_t* d_nan, void* d_workspace, size_t workspace_bytes);

/* ---- stack_cube: the slabs of many lines of one cube, interpolated onto one velocity grid and averaged ----
 * spectral_cube.analysis_utilities: stack_cube (analysis_utilities.py:321-432): spectral_slab per line (spectral_cube.py:
 * 1823-1879), the first surviving slab as it is (:406-407), every other one through spectral_interpolate onto the first
 * one's axis (:408-410; the Dask class, dask_spectral_cube.py:1291-1373: NaN outside the slab, NaN where a bracketing
 * sample is NaN or excluded), then average(cutouts, axis=0) (:412).  One kernel, no cutout written.
 * Per source s < nsrc and output channel j < n0 the HOST tables (row s, column j; the plan of ops.lerp_plan in absolute
 * channels of the cube view) give h_lo = the lower bracketing channel, -1 = outside the slab; h_t and h_inv_dx = its weight:
 * sample = a + (b - a) * (h_inv_dx * h_t), a / b = the samples h_lo and h_lo + 1 with excluded ones NaN (nan_excluded as
 * for the downsample entry points), a NaN result replaced by fill (the filled data of the interpolated slab).  A source
 * with h_exact[s] != 0 (the reference slab) contributes the FILLED sample h_lo itself: no arithmetic touches it.
 * mode: np.nanmean (NaN where no source is finite) / np.mean / np.nansum (0 there) / np.sum (NaN where any source is NaN).
 * Interpolation and the sum over the sources run in float64 in source order, rounded once at the store; every output
 * voxel is owned by one lane: no atomics, two runs agree bit for bit.  d_out: (n0, ny, nx), C-contiguous, the cube's type.
 * The tables are checked before anything is queued: nsrc >= 1, n0 >= 2, every h_lo -1 or a channel of the cube whose upper
 * neighbour exists (SPC_ERR_INVALID); nsrc above SPC_STACK_CUBE_MAX_LINES is SPC_ERR_UNSUPPORTED.  They may be freed when
 * the call returns (they travel as kernel arguments into d_workspace: spc_stack_cube_workspace_bytes).  No limit on an axis. */
#define SPC_STACK_CUBE_MAX_LINES 64
typedef enum {
    SPC_STACK_CUBE_NANMEAN = 0, SPC_STACK_CUBE_MEAN = 1, SPC_STACK_CUBE_NANSUM = 2, SPC_STACK_CUBE_SUM = 3
} spc_stack_cube_mode;
size_t spc_stack_cube_workspace_bytes(int nsrc, int64_t n0);
int spc_stack_cube_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded, float fill,
                       int nsrc, const int32_t* h_lo, const double* h_t, const double* h_inv_dx, const int32_t* h_exact, int mode,
                       int64_t n0, float* d_out, void* d_workspace, size_t workspace_bytes);
int spc_stack_cube_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded, double fill,
                       int nsrc, const int32_t* h_lo, const double* h_t, const double* h_inv_dx, const int32_t* h_exact, int mode,
                       int64_t n0, double* d_out, void* d_workspace, size_t workspace_bytes);

/* ---- mosaic_cubes: many cubes reprojected onto one sky grid and averaged where they overlap, in one pass ----
 * spectral_cube.cube_utils: mosaic_cubes (cube_utils.py:810-856): per cube, in list order, SpectralCube.reproject onto the
 * common header (:826-836; reproject_interp of the FILLED data, order 0 | 1), weight += the 2-D footprint (:839-840),
 * final += nan_to_num(filled data of the reprojected cube) in float64 (:843-845; NaN -> 0, +-inf -> +-DBL_MAX, and the
 * cube's fill value outside its footprint), then final /= weight (:848-852; 0 / 0 = NaN where no cube reaches).
 * One kernel: no reprojected cube is written, every output value is stored once, by the one lane that owns it (no atomics:
 * two runs agree bit for bit).  The value a source gives at an output voxel has the bits of spc_resample_bilinear_f32 / _f64
 * with the same mask, fill, maps and order; the sum and the division run in float64, rounded once at the store.
 * h_sources: a HOST table of nsrc descriptors (any nsrc >= 1: it travels as kernel arguments into d_workspace,
 * spc_mosaic_workspace_bytes, and may be freed when the call returns).  Per source: the cube view (nz channels, like the
 * output), its mask (flags = 0: none) and fill value, and its float64 (ny_out, nx_out) DEVICE maps d_xs / d_ys of source pixel
 * coordinates (spc_wcs_pixel_map_f64; -1e30 or a non-finite entry = not on the source).  d_out: (nz, ny_out, nx_out),
 * C-contiguous, the cubes' type.  d_weight: optional int32 (ny_out, nx_out), the number of sources that reach each pixel.
 * No limit on an axis or on nsrc. */
typedef struct {
    spc_cube_f32 cube;
    spc_mask mask;
    float fill;
    const double* d_xs;
    const double* d_ys;
} spc_mosaic_source_f32;
typedef struct {
    spc_cube_f64 cube;
    spc_mask_f64 mask;
    double fill;
    const double* d_xs;
    const double* d_ys;
} spc_mosaic_source_f64;
size_t spc_mosaic_workspace_bytes(int nsrc);
int spc_mosaic_f32(int device, void* stream, int nsrc, const spc_mosaic_source_f32* h_sources, int64_t nz, int64_t ny_out,
                   int64_t nx_out, int order, float* d_out, int32_t* d_weight, void* d_workspace, size_t workspace_bytes);
int spc_mosaic_f64(int device, void* stream, int nsrc, const spc_mosaic_source_f64* h_sources, int64_t nz, int64_t ny_out,
                   int64_t nx_out, int order, double* d_out, int32_t* d_weight, void* d_workspace, size_t workspace_bytes);

/* ---- cube arithmetic: + - * / ** with scalars, maps, spectra and cubes, a chain of them in one pass ----
 * SpectralCube.__add__ / __sub__ / __mul__ / __truediv__ / __pow__ (spectral_cube.py:2237-2361): _apply_everywhere
 * (:912-942, op(filled_data, value)) for a value that is not a cube, _cube_on_cube_operation (:944-1003, op of the raw
 * samples of both cubes) for one that is.  The reference makes one pass and one temporary per operator; here a chain of
 * up to SPC_ARITH_MAX_STEPS operators is a program that reads the cube once and writes once.  Per voxel:
 *     a = sample;  inc = include(a, mask)  (once, on the SOURCE sample; nan_excluded as for spc_downsample_*);  v = a
 *     for every step:  if (step.refill) v = inc ? v : fill;   v = op(v, b)
 *     store v
 * which is the reference step by step: every _apply_everywhere refills the excluded voxels of its input (refill = 1; they
 * hold op(fill, b) afterwards, whatever earlier steps left there), a cube-on-cube step reads the raw samples (refill = 0).
 * b is the step's scalar (is_scalar != 0, d_data NULL; given as double, rounded to the sample type) or an array of the
 * entry point's sample type with one ELEMENT stride per axis, 0 = broadcast along it; stride_x is 0 or 1.  SQUARE, SQRT,
 * RECIP and ONE take no operand (is_scalar != 0): numpy's fast paths of ** 2, ** 0.5, ** -1 and ** 0 (x * x, sqrt(x),
 * 1 / x, 1), to which the host maps those exponents (** 1 is no step at all, or MUL by 1 in a chain).
 * ADD SUB MUL DIV SQUARE SQRT RECIP are single correctly rounded IEEE operations in the sample type - the unit is
 * compiled with contraction off, a MUL followed by an ADD is never fused, division and sqrt are the IEEE ones - so a
 * chain equals numpy's stepwise result bit for bit; POW is the device pow / powf (a few ulp from a host libm).
 * A lane owns 4 consecutive x of a row: 16-byte loads and stores (4-byte for the mask bytes) where a row's addresses
 * allow, sample by sample at a misaligned head, at the tail and in rows whose arrays disagree about alignment; an operand
 * that is broadcast along x costs one load per row and lane.  64-bit indexing; rows and planes are strided over the grid:
 * no limit on any axis.  No LDS, no atomics, no workspace.  d_out strides in elements (0 = C-contiguous).
 * SPC_ERR_INVALID before anything is queued: a NULL pointer, n_steps outside 1 ... SPC_ARITH_MAX_STEPS, an unknown opcode,
 * is_scalar != 0 with a d_data pointer or is_scalar == 0 without one, an array operand of an opcode that takes none, a
 * negative stride or stride_x > 1, d_out overlapping the cube, the mask array or an operand. */
#define SPC_ARITH_MAX_STEPS 4
typedef enum {
    SPC_AOP_ADD = 0, SPC_AOP_SUB = 1, SPC_AOP_MUL = 2, SPC_AOP_DIV = 3, SPC_AOP_POW = 4,
    SPC_AOP_SQUARE = 5, SPC_AOP_SQRT = 6, SPC_AOP_RECIP = 7, SPC_AOP_ONE = 8
} spc_arith_opcode;
typedef struct {
    int32_t opcode;              /* spc_arith_opcode */
    int32_t refill;              /* != 0: excluded voxels are set to fill before the operation */
    int32_t is_scalar;           /* != 0: the operand is `scalar` and d_data must be NULL */
    int32_t reserved;
    double scalar;
    const void* d_data;          /* float (_f32) or double (_f64) */
    int64_t stride_z, stride_y, stride_x;   /* elements, >= 0; 0 = broadcast along that axis; stride_x 0 or 1 */
} spc_arith_step;
typedef struct {
    int32_t n_steps, reserved;
    spc_arith_step steps[SPC_ARITH_MAX_STEPS];
} spc_arith_program;
int spc_arith_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int nan_excluded, float fill,
                  const spc_arith_program* prog, float* d_out, int64_t out_row_stride, int64_t out_plane_stride);
int spc_arith_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int nan_excluded, double fill,
                  const spc_arith_program* prog, double* d_out, int64_t out_row_stride, int64_t out_plane_stride);

/* ---- FITS payload -> float32 -------------------
 * Converts n raw big-endian FITS image samples (already in HBM) to native
 * float32: what astropy.io.fits does on the host behind
 * spectral_cube/io/fits.py:63-172 (read_data_fits) / :171-260 (load_fits_cube).
 * bitpix in {8, 16, 32, 64, -32, -64}.  Scaling follows astropy: BITPIX 8/16 in
 * float32 (raw * BSCALE + BZERO), 32/64 in float64 then rounded, floating types
 * in their own precision; has_blank/blank: integer BLANK value -> NaN.
 * The multiply and the add are two roundings; the multiply is left out for
 * BSCALE 1 and the add for BZERO 0, as astropy leaves them out (-1 * 0 stays -0).
 * BITPIX 32/64 reach float32 through float64 also when unscaled (two roundings:
 * the reference's cube of an integer image is float64).  BITPIX 64 with BSCALE 1,
 * BZERO 2^63 is converted as the uint64 it means, in one rounding, as astropy does.
 * An unscaled BITPIX -32 image comes back bit for bit (NaN payloads, -0, denormals),
 * which makes the call its own inverse (the writers use it).
 * Where this follows the FITS standard and astropy 4.3.1 does not:
 *   1. BLANK = 0 blanks (astropy tests the truth of the value and skips it);
 *   2. BLANK on a pseudo-unsigned image (BSCALE 1, BZERO 2^15 / 2^31 / 2^63, or
 *      -128 for BITPIX 8) blanks: BLANK is a value of the raw integers and is
 *      compared with them whenever bitpix > 0 (astropy returns the unsigned
 *      array and forgets BLANK).
 * (A third one, up to three roundings for BITPIX 64 with BZERO 2^63, is gone: see
 * above.)  has_blank is ignored for bitpix < 0, as astropy ignores the card.
 * d_raw and d_out must be aligned to their own sample size (1 / 2 / 4 / 8 bytes
 * for d_raw, 4 for d_out) and need no more: 16-byte aligned pairs of an
 * unscaled BITPIX -32 image take a faster path, nothing else depends on it.
 * Refused (SPC_ERR_INVALID, nothing written): another bitpix, NULL, n < 0. */
int spc_fits_to_f32(int device, void* stream, const void* d_raw, int bitpix,
                    double bscale, double bzero, int has_blank, int64_t blank,
                    int64_t n, float* d_out);

/* The wide sample types in their own precision: bitpix in {-64, 32, 64} -> native float64 (what astropy hands the
 * reference for such an image, spectral_cube/io/fits.py:63-172); feeds spc_moments_f64.  Scaling, BLANK, the uint64 of
 * BZERO 2^63 and the alignment rule (d_raw 4 / 8 bytes, d_out 8) as above; any other bitpix is refused. */
int spc_fits_to_f64(int device, void* stream, const void* d_raw, int bitpix,
                    double bscale, double bzero, int has_blank, int64_t blank,
                    int64_t n, double* d_out);

/* d_data[i] *= factor over n contiguous floats: the Jy/beam rescaling by the ratio of beam
 * areas in convolve_to (spectral_cube/dask_spectral_cube.py:1450-1457). */
int spc_scale_f32(int device, void* stream, float* d_data, int64_t n, double factor);

/* ---- statistics ------------------------------
 * One read of the cube gives count / min / max / sum / sum of squares of the
 * included, non-NaN samples, accumulated in float64.
 *
 * spc_stats_global_f32 replaces the per-chunk compute_stats + aggregation of
 * DaskSpectralCubeMixin.statistics (spectral_cube/dask_spectral_cube.py:769-814)
 * and the axis=None forms of sum / mean / std / max / min (:641-767).
 * h_stats (HOST, 5 doubles) = {npts, min, max, sum, sumsq}; min / max are NaN
 * when nothing is included.  Synchronises the stream. */
int spc_stats_global_f32(int device, void* stream, const spc_cube_f32* cube,
                         const spc_mask* mask, double* h_stats, void* d_workspace, size_t workspace_bytes);

/* Reductions along one axis (0, 1 or 2) behind sum / mean / std / max / min with
 * axis given (dask_spectral_cube.py:641-767; spectral_cube.py:578-791).  Output
 * maps are C-contiguous with the reduced axis removed: (ny,nx), (nz,nx), (nz,ny).
 * NULL outputs are skipped.  A ray without included samples gives count 0 and
 * NaN in the four floating maps (nansum_allbadtonan, nanmin / nanmax of all-NaN). */
/* The same five numbers for every channel: h_stats (HOST) = nz records {npts, min, max, sum, sumsq}
 * of the (ny,nx) planes - the nan-reductions with axis=(1, 2), e.g. the mean spectrum cube.mean(axis=(1, 2)). */
int spc_stats_planes_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                         double* h_stats, void* d_workspace, size_t workspace_bytes);

typedef struct spc_stats_outputs {
    int32_t* d_count;
    float* d_min;
    float* d_max;
    double* d_sum;
    double* d_sumsq;
} spc_stats_outputs;
int spc_stats_axis_f32(int device, void* stream, const spc_cube_f32* cube,
                       const spc_mask* mask, int axis, const spc_stats_outputs* out);

/* The second pass of std (nanstd, dask_spectral_cube.py:699-710): d_m2 = sum (x - mean)^2 of every ray along *axis*
 * about that ray's OWN mean d_sum / d_count, from the count and sum maps spc_stats_axis_* wrote for the same cube, mask
 * and axis (same shapes; d_m2 may not alias them).  sumsq / n - mean^2 loses (mean / sigma)^2 ulps on a pedestal, this
 * about n ulps.  NaN for a ray without included samples.  Rays merge as m2_a + m2_b + (mean_a - mean_b)^2 n_a n_b / n. */
int spc_stats_m2_axis_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int axis,
                          const int32_t* d_count, const double* d_sum, double* d_m2);
int spc_stats_m2_axis_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int axis,
                          const int32_t* d_count, const double* d_sum, double* d_m2);
/* The same pass about ONE centre for every ray (the mean of the whole cube, from spc_stats_global_*): d_s1 = sum (x - center),
 * d_s2 = sum (x - center)^2 per ray along *axis*, 0 for a ray without included samples.  The caller adds the rays:
 * sum (x - mean)^2 of the cube = S2 - S1^2 / npts. */
int spc_stats_dev_axis_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int axis,
                           double center, double* d_s1, double* d_s2);
int spc_stats_dev_axis_f64(int device, void* stream, const spc_cube_f64* cube, const spc_mask_f64* mask, int axis,
                           double center, double* d_s1, double* d_s2);

/* argmax / argmin along a SPATIAL axis (BaseSpectralCube.argmax / argmin with axis = 1 or 2,
 * spectral_cube/spectral_cube.py:793-819; axis 0 is an output of spc_moments_f32): nanargmax of
 * the data filled with -inf (argmin: +inf) - excluded and NaN samples take the fill, the first
 * index wins ties, rays without an included sample give 0.  int64 maps (nz,nx) / (nz,ny),
 * C-contiguous; a NULL output is skipped. */
int spc_argextrema_axis_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                            int axis, int64_t* d_argmin, int64_t* d_argmax);

/* ---- order statistics along the spectral axis ---
 * q-th percentile (numpy 'linear' interpolation; q = 50: the median) of the
 * included, non-NaN samples of every ray: DaskSpectralCubeMixin.median /
 * percentile (spectral_cube/dask_spectral_cube.py:657-693).  With d_center (a
 * (ny,nx) float32 map) the statistic is taken of |x - center|, and the result is
 * multiplied by scale: median absolute deviation -> mad_std (:711-731, astropy
 * stats.mad_std: scale = 1.482602218505602).  Rays without a valid sample give
 * NaN.  d_out: (ny,nx) float32, C-contiguous.
 * The rays run along the FIRST axis of the view that is passed in: for a selection along y
 * of a (nz, ny, nx) cube hand over the same buffer as {nz' = ny, ny' = nz, row_stride' =
 * plane_stride, plane_stride' = row_stride} (mask strides likewise); the result is (nz, nx). */
int spc_percentile_axis0_f32(int device, void* stream, const spc_cube_f32* cube,
                             const spc_mask* mask, double q, const float* d_center,
                             float scale, float* d_out);
/* The same along x (axis 2) without a transposed copy: rays = the rows of the cube, which are contiguous; d_center and
 * d_out are (nz, ny).  Rows of more than 4096 samples: SPC_ERR_UNSUPPORTED (transpose with
 * spc_fill_masked_transpose_f32 and use the exchanged-stride form above). */
int spc_percentile_axis2_f32(int device, void* stream, const spc_cube_f32* cube,
                             const spc_mask* mask, double q, const float* d_center,
                             float scale, float* d_out);

/* The same statistic over the WHOLE cube (median / percentile / mad_std with axis=None): four
 * histogram passes over the key bytes.  With has_center the statistic is taken of
 * |x - center| (float32 arithmetic, as numpy does for a float32 cube).  *h_out (HOST) gets the
 * value in double; NaN when nothing is included. */
int spc_percentile_global_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                              double q, int has_center, float center, double* h_out,
                              void* d_workspace, size_t workspace_bytes);

/* The same statistic over TWO axes at once, one result per index of the axis that is kept: median / percentile with
 * axis=(1, 2) or (0, 2) (BaseSpectralCube.median / percentile, spectral_cube/spectral_cube.py:1172-1257:
 * apply_numpy_function(np.nanmedian / np.nanpercentile, axis=pair)) and mad_std over a pair (:730-764, how='slice' with a
 * two-axis tuple; astropy stats.mad_std).  A group is every sample that shares the index along keep_axis:
 *   keep_axis = 0: the plane z (ny * nx samples), nz groups - the per-channel statistic;
 *   keep_axis = 1: the rows (z, y) of one y (nz * nx samples), ny groups.
 * The selection is spc_percentile_global_f32's, for all groups at once: four passes count one key byte each into
 * per-group histograms (64-bit counters), a small kernel walks every group's 256 counters on the device after each pass, a
 * fifth pass finds the next larger key - it is always launched and reads only the groups whose two order statistics are
 * different values - and the last kernel applies that entry's interpolation rule per group.  With d_center (ngroups float32,
 * DEVICE) the statistic is taken of |x - d_center[group]| in float32 arithmetic (a NaN centre: NaN); the result is
 * multiplied by scale as in spc_percentile_axis0_f32 (1.482602218505602: mad_std).  A group without an included,
 * non-NaN sample gives NaN.  d_out: ngroups float32, DEVICE.
 * The cube is read at most five times; everything is queued on `stream` and the call returns without synchronising: no
 * counter and no flag comes back to the host.  Any view spc_check_cube accepts and every mask form.  d_workspace:
 * spc_percentile_groups_workspace_bytes(ngroups) bytes of caller-owned scratch (2 KiB of counters and a small state
 * record per group); nothing is assumed of its contents. */
size_t spc_percentile_groups_workspace_bytes(int64_t ngroups);
int spc_percentile_groups_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask, int keep_axis,
                              double q, const float* d_center, float scale, float* d_out,
                              void* d_workspace, size_t workspace_bytes);

/* ONE pass of that selection, for a cube that is sharded over ranks (each rank calls this on its strip, the ranks add
 * their counters - or take the minimum of their next keys - and walk them together; the reference's counterpart is
 * the dask reduction tree under dask_spectral_cube.py:657-693).  Samples are compared through their order-preserving
 * 32-bit keys (of |x - center| with has_center); spc_key_to_f32 maps a key back to its float.
 *   h_hist != NULL (HOST, 256 counters): h_hist[d] = included samples whose key agrees with `prefix` on the bits of
 *       `pmask` and carries byte d at bit `shift` (24, 16, 8 or 0);
 *   h_next != NULL (HOST): the smallest key above `prefix`, 0xffffffff when there is none.
 * Exactly one of the two must be given.  Workspace: SPC_WS_PERCENTILE_GLOBAL. */
int spc_key_histogram_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                          uint32_t prefix, uint32_t pmask, int shift, int has_center, float center,
                          uint64_t* h_hist, uint32_t* h_next, void* d_workspace, size_t workspace_bytes);
float spc_key_to_f32(uint32_t key);

/* out[z][x][y] = included ? data[z][y][x] : fill, d_out a C-contiguous (nz, nx, ny) buffer: the
 * filled copy with the spatial axes exchanged, which turns an order statistic along x
 * (median(axis=2)) into one along y for spc_percentile_axis0_f32's exchanged-stride form. */
int spc_fill_masked_transpose_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                                  float fill, float* d_out);

/* ---- sigma clipping along the spectral axis (dask_spectral_cube.py:851-878) ----
 * astropy.stats.sigma_clip(axis=0, masked=False) iterates: per-ray centre and std
 * (spc_percentile_axis0_f32 / spc_stats_axis_f32), then everything outside
 * [centre - sigma_lower*std, centre + sigma_upper*std] becomes NaN, until nothing
 * changes.  These are the two elementwise ends of that loop:
 * spc_fill_masked_f32: out = included ? data : fill   (the NaN-filled working copy,
 *                      MaskBase._filled, masks.py:197-237);
 * spc_clip_outside_f32: in place, contiguous (nz,ny,nx): v < lo[y,x] || v > hi[y,x] -> NaN;
 *                      *h_nchanged (HOST) = number of samples clipped by this call. */
int spc_fill_masked_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                        float fill, float* d_out, int64_t out_row_stride, int64_t out_plane_stride);
/* The whole loop in ONE kernel for centre = median (center_is_mean = 0) or mean and spread = std (spread_is_mad = 0) or
 * mad_std (1.4826 x the median of |x - median|, a second selection per iteration): the rays stay in
 * registers across the iterations, the cube is read once and the clipped copy written once (d_out: (nz,ny,nx)
 * C-contiguous float32; masked and clipped samples NaN).  maxiters < 0: until nothing changes.  Same arithmetic as
 * the pieces above (float64 sums, float32 centre and bounds).  Rays of more than 4096 channels: SPC_ERR_UNSUPPORTED.
 * (ABI 7) d_workspace / workspace_bytes: spc_workspace_bytes(SPC_WS_SIGMA_CLIP, nz, ny, nx, 0, 0) bytes of caller-owned
 * scratch, or NULL / 0.  With it the kernel's block shape follows the mask (a probe counts the valid samples of 64 rays: rays
 * of at most 128 valid samples - signal masks - are packed and clipped by one wave each, in blocks whose runs per plane are
 * twice as wide); without it the shape is the one that suits dense rays. */
int spc_sigma_clip_axis0_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                             double sigma_lower, double sigma_upper, int maxiters, int center_is_mean,
                             int spread_is_mad, float* d_out, void* d_workspace, size_t workspace_bytes);
/* The include map of a mask evaluated on the cube it is bound to, as a uint8 (nz,ny,nx) array in
 * HBM: d_out = included ? 1 : 0 (MaskBase.include, masks.py:105-116).  For masks that belong to
 * ANOTHER cube's data - a smoothed cube keeps its parent's mask object (dask_spectral_cube.py:836-840):
 * the predicate terms run on the parent's device data instead of a host copy of it.  nan_excluded != 0
 * additionally drops NaN samples (~isnan style masks). */
int spc_mask_include_u8(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                        int nan_excluded, uint8_t* d_out);
/* per-ray clipping bounds of one iteration, all on the device: lo = centre - sigma_lower * std,
 * hi = centre + sigma_upper * std over n rays.  centre = d_center (e.g. the median map) or, when
 * NULL, the mean from d_count / d_sum / d_sumsq; std = d_spread (e.g. the mad_std map) or, when
 * NULL, sqrt(max(sumsq / n - mean^2, 0)) - float64 arithmetic, float32 bounds like astropy's. */
int spc_clip_bounds_f32(int device, void* stream, int64_t n, const int32_t* d_count, const double* d_sum,
                        const double* d_sumsq, const float* d_center, const float* d_spread,
                        double sigma_lower, double sigma_upper, float* d_lo, float* d_hi);
int spc_clip_outside_f32(int device, void* stream, float* d_cube, int64_t nz, int64_t ny, int64_t nx,
                         const float* d_lo, const float* d_hi, uint64_t* h_nchanged,
                         void* d_workspace, size_t workspace_bytes);

/* 2-D convolution of one (ny, nx) float64 map with an odd-sized kernel (zero fill outside,
 * kernel normalised by its sum, true convolution, NaN propagates).  Serves the algebraic
 * spatial_smooth -> moment path: when every voxel is valid, astropy's convolution
 * (dask_spectral_cube.py:962-993) commutes with the sums along the spectral axis
 * (:1083-1104), so the moment sums of the smoothed cube are the smoothed moment sums. */
int spc_map_conv2d_f64(int device, void* stream, const double* d_in, int64_t ny, int64_t nx,
                       const double* h_kernel, int nky, int nkx, double* d_out,
                       void* d_workspace, size_t workspace_bytes);

/* Elementwise arithmetic on float64 maps of n elements, so that the algebra around spc_map_conv2d_f64 (moment
 * sums from moments, moments from smoothed sums) stays on the device:
 *   SPC_MAP_MUL                out = a * b
 *   SPC_MAP_SECOND_MOMENT_SUM  out = (a + b*b) * c        S2 = (m2 + mu^2) * S0
 *   SPC_MAP_DIV_ADD            out = a / b + s            mu' = S1' / S0' (+ axis offset)
 *   SPC_MAP_DIV_SUB_SQ         out = a / b - c*c          m2' = S2' / S0' - mu'^2
 * d_out may alias an input. */
typedef enum { SPC_MAP_MUL = 0, SPC_MAP_SECOND_MOMENT_SUM = 1, SPC_MAP_DIV_ADD = 2, SPC_MAP_DIV_SUB_SQ = 3 } spc_map_op;
int spc_map_arith_f64(int device, void* stream, int op, const double* d_a, const double* d_b, const double* d_c,
                      double s, double* d_out, int64_t n);

/* The checks the algebraic smooth -> moment paths make before they trust their shortcut, on the device: *d_flags (one
 * uint32 in HBM, cleared by this call on the same stream) gets bit 0 if any of the n int32 counts differs from
 * `expect` (a spaxel with an invalid voxel), bit 1 if any of the n float64 values is not finite.  Either array may be
 * NULL.  Asynchronous: the caller reads back four bytes instead of two maps. (ABI 4) */
int spc_map_check(int device, void* stream, const int32_t* d_counts, int32_t expect, const double* d_values,
                  int64_t n, uint32_t* d_flags);

/* moments along a spatial axis (axis = 1 or 2), reference golden tables
 * spectral_cube/tests/test_moments.py:19-49.  d_cen is a (ny,nx) float64 map
 * of offsets along that axis (spectral_cube.py:1476-1503), pix_size the pixel
 * scale (spectral_cube.py:1530-1533).  Outputs have shape (nz,nx) for axis 1
 * and (nz,ny) for axis 2, C-contiguous. */
int spc_moments_spatial_f32(int device, void* stream, const spc_cube_f32* cube,
                            const spc_mask* mask, int axis, const double* d_cen,
                            double pix_size, double* d_m0, double* d_m1,
                            double* d_m2);

/* order N >= 2 along a spatial axis, second pass: out = sum v (c - mu)^N / sum v with d_mu = the
 * moment-1 map of spc_moments_spatial_f32 (offsets, no world coordinate added), same output shapes
 * (dask_spectral_cube.py:1094-1099; _moments.py:185-193 with axis != 0). */
int spc_moment_order_spatial_f32(int device, void* stream, const spc_cube_f32* cube,
                                 const spc_mask* mask, int axis, const double* d_cen, int order,
                                 const double* d_mu, double* d_out);

/* ---- NaN-aware convolution (astropy.convolution.convolve semantics:
 * boundary='fill', fill_value=0, nan_treatment='interpolate',
 * normalize_kernel=True) ---------------------------------------------------
 * spectral: replaces the chunk function of DaskSpectralCubeMixin.
 * spectral_smooth (dask_spectral_cube.py:880-917; NumPy twin
 * spectral_cube.py:3186-3222).  h_kernel: ntaps (odd) doubles on the HOST.
 * Input voxels failing the mask are treated as NaN (the reference convolves
 * the NaN-filled chunk).  Output float32, same shape. */
int spc_spectral_conv_f32(int device, void* stream, const spc_cube_f32* cube,
                          const spc_mask* mask, const double* h_kernel, int ntaps,
                          float* d_out, int64_t out_row_stride,
                          int64_t out_plane_stride, void* d_workspace, size_t workspace_bytes);

/* fused spectral_smooth -> moments (legal because the Dask smooth is lazy and
 * keeps the ORIGINAL mask, dask_spectral_cube.py:836-840): the smoothed cube
 * is never written.  Semantics = spc_spectral_conv_f32 followed by
 * spc_moments_f32 with the same mask re-applied to the smoothed values.
 * h_cen: optional HOST copy of d_cen (nz doubles, may be NULL); when it shows
 * the axis is linear the kernel derives the offsets from the channel index
 * instead of loading them (every FITS spectral axis is linear). */
int spc_spectral_conv_moments_f32(int device, void* stream, const spc_cube_f32* cube,
                                  const spc_mask* mask, const double* h_kernel,
                                  int ntaps, const double* d_cen, const double* h_cen,
                                  double dv, double m1_add, const spc_moment_outputs* out,
                                  void* d_workspace, size_t workspace_bytes);

/* spatial: replaces the per-channel 2-D convolution of spatial_smooth
 * (dask_spectral_cube.py:962-993 + :540-547; NumPy twin spectral_cube.py
 * :2808-2842).  Separable form: kernel2d = outer(h_ky, h_kx) (exact for
 * Gaussian2DKernel).  Non-separable kernels: spc_spatial_conv2d_f32. */
int spc_spatial_conv_sep_f32(int device, void* stream, const spc_cube_f32* cube,
                             const spc_mask* mask, const double* h_ky, int nky,
                             const double* h_kx, int nkx, float* d_out,
                             int64_t out_row_stride, int64_t out_plane_stride,
                             void* d_workspace, size_t workspace_bytes);
int spc_spatial_conv2d_f32(int device, void* stream, const spc_cube_f32* cube,
                           const spc_mask* mask, const double* h_kernel, int nky,
                           int nkx, float* d_out, int64_t out_row_stride,
                           int64_t out_plane_stride, void* d_workspace, size_t workspace_bytes);

/* masked separable spatial_smooth with the DENOMINATOR on the matrix cores, optionally fused with moment 0
 * (dask_spectral_cube.py:962-993 then :1083-1104: the Dask graph never materialises the smoothed cube either).
 * out = sum k d [valid] / sum k [valid] like spc_spatial_conv_sep_f32; the numerator is float32 vector arithmetic
 * (two columns per packed FMA), the denominator - a convolution of a 0 / 1 array - is two banded-Toeplitz matrix
 * products per 16 x 16 tile on v_mfma_f32_16x16x32_f16: mask bits are exact in fp16, the (power-of-two scaled) taps and
 * the intermediate go in as fp16 hi + lo pairs with float32 accumulation (<= 1e-6 relative on the denominator).
 * One block = a band of 16 rows x a strip of 480 columns, walking a chunk of channels.
 *   d_out  (may be NULL): the smoothed cube (nz, ny, nx), float32.
 *   d_m0   (may be NULL): moment 0 of the smoothed cube under the ORIGINAL mask, dv * nansum over channels, NaN where no
 *          channel contributes (float64 (ny, nx), row stride m0_row_stride or nx) - the cube is then never written.
 * SPC_ERR_UNSUPPORTED (the caller falls back to spc_spatial_conv_sep_f32 + spc_moments_f32): more than 29 (third form: 33) taps per
 * axis, a negative tap or a zero centre tap, mask terms other than SPC_MASK_ARRAY / SPC_MASK_FINITE, odd nx or strides.
 * (ABI 4) */
int spc_spatial_conv_sep_mfma_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                                  const double* h_ky, int nky, const double* h_kx, int nkx,
                                  float* d_out, int64_t out_row_stride, int64_t out_plane_stride,
                                  double dv, double* d_m0, int64_t m0_row_stride,
                                  void* d_workspace, size_t workspace_bytes);

/* (ABI 6) The same operator with moments 1 / 2 of the smoothed cube as well, and - for both entry points, wherever nx and
 * the strides are multiples of 4 and the bases 16-byte aligned - a third form in which EVERY product runs on
 * v_mfma_f32_16x16x32_f16: the masked samples go in as fp16 hi + lo under one power-of-two scale per step of 16 rows
 * (the running maximum of the wave's channel), the taps as fp16 hi + lo, the x-pass result is split again for the y pass
 * (spc_spatial_split.hip; <= 1e-6 of the data range against float64).  Moments follow spc_moments_f32's conventions:
 *   d_cen  nz doubles in device memory = pix_cen[z] - c_ref;  m1 = S1 / S0 + m1_add,  m2 = S2 / S0 - (S1 / S0)^2,
 *   S_n = nansum over channels of c^n * smoothed value under the ORIGINAL mask (dask_spectral_cube.py:1083-1104 on the
 *   lazily smoothed cube of :962-993); rays without a contribution: m0 NaN, m1 / m2 NaN (0 / 0).
 * Any of d_out, d_m0, d_m1, d_m2 may be NULL (not all).  Workspace: spc_workspace_bytes(SPC_WS_SPATIAL_CONV_MFMA, nz, ny,
 * nx, 3, 0) when d_m1 or d_m2 is asked for.  SPC_ERR_UNSUPPORTED as above, and for moments 1 / 2 where the third form
 * does not apply. */
int spc_spatial_conv_sep_mfma_moments_f32(int device, void* stream, const spc_cube_f32* cube, const spc_mask* mask,
                                          const double* h_ky, int nky, const double* h_kx, int nkx,
                                          float* d_out, int64_t out_row_stride, int64_t out_plane_stride,
                                          const double* d_cen, double dv, double m1_add,
                                          double* d_m0, double* d_m1, double* d_m2, int64_t map_row_stride,
                                          void* d_workspace, size_t workspace_bytes);

/* ---- resampling -----------------------------------------------------------
 * spectral lerp: replaces interp_wrapper / scipy interp1d(kind='linear') of
 * DaskSpectralCubeMixin.spectral_interpolate (dask_spectral_cube.py:1342-1353).
 * For output channel j: lo = d_lo[j] (int32 input channel), and
 *   out = (in[lo+1]-in[lo]) * d_inv_dx[j] * d_t[j] + in[lo]      (float64 maths)
 * d_lo[j] < 0 marks out-of-range channels which receive `fill`.
 * NaN in either bracketing sample gives NaN (scipy semantics). */
int spc_spectral_lerp_f32(int device, void* stream, const spc_cube_f32* cube,
                          const spc_mask* mask, int64_t nz_out, const int32_t* d_lo,
                          const double* d_t, const double* d_inv_dx, float fill,
                          float* d_out, int64_t out_row_stride,
                          int64_t out_plane_stride);

/* Pixel map of a reprojection, on the device: for every pixel of the target grid (wcs_out) the
 * 0-based pixel coordinates in the source grid (wcs_in) - what reproject_interp obtains from
 * astropy.wcs (pixel_to_world on the target, world_to_pixel on the source; spectral_cube.py:2700-2732).
 * FITS paper II arithmetic in float64 for the zenithal projections TAN / SIN / ARC / STG / ZEA and the
 * (pseudo-)cylindrical CAR / SFL / CEA / MER / AIT, with astropy's SIP stage on either side (all_pix2world /
 * all_world2pix); pixels that cannot be projected (or lie beyond the edge of the sky of an all-sky projection, or
 * where the SIP inverse does not converge) get -1e30 (outside every footprint).  The host fills the
 * struct from the header (spectral_cube_amd/wcs.py). */
#define SPC_SIP_MAX_ORDER 9
#define SPC_SIP_TERMS 55           /* coefficients of u^p v^q, p + q <= 9: row p starts at p * 10 - p * (p - 1) / 2 */
typedef struct spc_celestial_wcs {
    int32_t proj;              /* 0 TAN, 1 SIN, 2 ARC, 3 STG, 4 ZEA, 5 CAR, 6 SFL, 7 CEA, 8 MER, 9 AIT */
    int32_t sip_order;         /* 0 = no SIP distortion; else max(A_ORDER, B_ORDER) <= 9 (ABI 4; was `reserved`) */
    double crpix[2];           /* FITS 1-based reference pixel (x, y) */
    double lin[4];             /* CDELT_i * PC_ij, 2 x 2 row-major: degrees per pixel */
    double lin_inv[4];         /* its inverse */
    double alpha_p, delta_p;   /* celestial coordinates of the native pole (radians) */
    double phi_p;              /* LONPOLE (radians) */
    double pv1;                /* CEA: PV2_1 (lambda), else unused (ABI 3) */
    double plane0[2];          /* (x0, y0) degrees: the projection of the user's fiducial point (PV1_0 != 0 with PV1_1 /
                                * PV1_2; wcslib prjoff), added before deprojection, subtracted after projection (ABI 4) */
    double sip_a[SPC_SIP_TERMS];   /* SIP forward polynomials (Shupe et al. 2005): u' = u + A(u, v), v' = v + B(u, v) with */
    double sip_b[SPC_SIP_TERMS];   /* (u, v) = pixel - CRPIX; as the TARGET they are evaluated, as the SOURCE they are
                                    * inverted by Newton's method - the limit of astropy's all_world2pix iteration (ABI 4) */
} spc_celestial_wcs;
/* frame_rot (HOST pointer, 15 doubles, may be NULL = same frame): [0..8] row-major rotation of the unit sphere that
 * takes the TARGET's celestial frame to the SOURCE's (ICRS / FK5(equinox) / FK4-NO-E(equinox) / Galactic:
 * spectral_cube_amd/wcs.py::frame_transform) - reproject_interp transforms the target's sky coordinates to the source's
 * frame before it asks the source WCS for pixels (the reference's own test goes RA/DEC -> GLON/GLAT,
 * tests/test_regrid.py:99-135); [9..11] the E-terms of aberration removed from the unit vector BEFORE the rotation (an
 * FK4 target; zeros = none), [12..14] the E-terms added AFTER it (an FK4 source; zeros = none).
 * (ABI 3: the argument; ABI 4: 15 doubles instead of 9.) */
int spc_wcs_pixel_map_f64(int device, void* stream, const spc_celestial_wcs* wcs_out,
                          const spc_celestial_wcs* wcs_in, const double* frame_rot,
                          int64_t ny_out, int64_t nx_out, double* d_xs, double* d_ys);

/* spatial resample: replaces the inner resampler of
 * reproject.reproject_interp(order='bilinear' | 'nearest-neighbor') called from
 * BaseSpectralCube.reproject (spectral_cube.py:2700-2732).  d_xs, d_ys:
 * (ny_out,nx_out) float64 source pixel coordinates (0-based).  Output pixels
 * whose source falls outside [-0.5, n-0.5] are NaN and get footprint 0.
 * order: 1 = bilinear (a NaN neighbour propagates even with weight 0, as in
 * scipy.ndimage.map_coordinates), 0 = nearest neighbour (floor(x + 0.5)).
 * d_footprint (uint8, (ny_out,nx_out), written as 0 / 1) may be NULL.  d_any_valid (one uint32 in
 * HBM, may be NULL) is set to 1 iff some output value is not NaN: the reference's
 * "All values in reprojected cube are nan" check (spectral_cube.py:2733-2739)
 * without another pass over the output. */
int spc_resample_bilinear_f32(int device, void* stream, const spc_cube_f32* cube,
                              const spc_mask* mask, float fill, int64_t ny_out,
                              int64_t nx_out, const double* d_xs, const double* d_ys,
                              float* d_out, int64_t out_row_stride,
                              int64_t out_plane_stride, uint8_t* d_footprint,
                              int order, uint32_t* d_any_valid,
                              void* d_workspace, size_t workspace_bytes);

/* spatial resample with the spectral interpolation folded in (ABI 8): ONE pass for what the reference does as
 * spectral_interpolate (dask_spectral_cube.py:1342-1353) followed by reproject (spectral_cube.py:2700-2732), and for
 * reproject onto a cube header whose spectral axis differs from the cube's (reproject_interp's single trilinear call for
 * a separable WCS, spectral_cube.py:2726-2732).  Output channel j (nz_out of them) is
 *   out[j] = (R[lo+1] - R[lo]) * d_inv_dx[j] * d_t[j] + R[lo],   lo = d_lo[j],
 * where R[k] is input channel k resampled exactly as spc_resample_bilinear_f32 does (mask, fill, order, footprint as there)
 * and the blend is spc_spectral_lerp_f32's arithmetic - both operators are linear interpolations with NaN propagation,
 * so they commute: a value is NaN iff one of its eight source samples is excluded / NaN or the pixel lies outside the
 * footprint, as in the two-pass form; finite values agree with it to float32 rounding (each input plane is read and
 * resampled ONCE, nz instead of nz_out gathers, and the intermediate cube is never written).  d_lo[j] < 0 marks channels
 * outside the input range (NaN planes).  Precondition: the non-negative entries of d_lo ascend and are contiguous in j
 * (an ascending output grid on ascending input channels; a descending plan is run reversed, with d_out at its LAST plane and
 * a negative out_plane_stride: the strides are signed); cube->nz >= 2.
 * Workspace: spc_workspace_bytes(SPC_WS_RESAMPLE_BILINEAR_LERP, nz, ny, nx, ny_out, nx_out). */
int spc_resample_bilinear_lerp_f32(int device, void* stream, const spc_cube_f32* cube,
                                   const spc_mask* mask, float fill, int64_t ny_out,
                                   int64_t nx_out, const double* d_xs, const double* d_ys,
                                   int64_t nz_out, const int32_t* d_lo, const double* d_t,
                                   const double* d_inv_dx, float* d_out, int64_t out_row_stride,
                                   int64_t out_plane_stride, uint8_t* d_footprint,
                                   int order, uint32_t* d_any_valid,
                                   void* d_workspace, size_t workspace_bytes);

/* spline resample: reproject_interp(order='biquadratic' | 'bicubic') for channels that map onto themselves
 * (spectral_cube.py:2667-2676 documents the orders; :2726-2732 is the call).  order 2 / 3 =
 * scipy.ndimage.map_coordinates(order, mode='constant', cval=nan) on the planes replicated by one border pixel: B-spline
 * prefilter with mirror boundaries along y and x, 3 x 3 / 4 x 4 gather, float64 throughout, NaN outside
 * [-0.5, n - 0.5].  The cube must hold finite samples only (scipy's recursive prefilter turns ONE non-finite sample into
 * an all-NaN result; the caller checks and raises the reference's "All values in reprojected cube are nan").
 * d_workspace: nz x (ny + 2) x (nx + 2) float64 coefficients (the caller resamples a slab of channels at a time). (ABI 4) */
int spc_resample_spline_f32(int device, void* stream, const spc_cube_f32* cube, int order, int64_t ny_out,
                            int64_t nx_out, const double* d_xs, const double* d_ys, float* d_out,
                            int64_t out_row_stride, int64_t out_plane_stride, uint8_t* d_footprint,
                            void* d_workspace, size_t workspace_bytes);

/* ---- multi-GPU stitch (RCCL over xGMI) -----------------------------------
 * One process per GPU; each rank owns a row strip of the 2-D map.  The id is
 * created on rank 0 (spc_comm_unique_id) and distributed by the host
 * launcher (torch.distributed store / file), then every rank calls
 * spc_comm_init.  spc_allgather_rows gathers equal-sized strips. */
#define SPC_COMM_ID_BYTES 128
int spc_comm_unique_id(uint8_t id[SPC_COMM_ID_BYTES]);
int spc_comm_init(int device, const uint8_t id[SPC_COMM_ID_BYTES], int nranks,
                  int rank, void** comm);
int spc_comm_destroy(void* comm);
int spc_allgather_rows(void* comm, void* stream, const void* d_send, void* d_recv,
                       size_t bytes_per_rank);
/* n all-gathers in ONE grouped launch (ncclGroupStart / ncclGroupEnd): e.g. the three moment maps of a row chunk,
 * each gathered into its own destination map. */
int spc_allgather_rows_batch(void* comm, void* stream, int n, const void* const* d_send, void* const* d_recv,
                             const size_t* bytes_per_rank);

#ifdef __cplusplus
}
#endif
#endif /* SPCUBE_HIP_H */
