"""ctypes binding of libspcube_hip.so (C ABI declared in include/spcube_hip.h).

The product path has NO CPU fallback: if the shared library cannot be loaded
every entry point raises :class:`HipLibraryError`.  Loading the library does
not need a GPU (symbols can be inspected on a CPU-only box); launching does.
"""
import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libspcube_hip.so"
LIB_PATH = os.environ.get("SPC_HIP_LIBRARY", os.path.join(_HERE, LIB_NAME))

SPC_OK = 0
SPC_ERR_INVALID = -1
SPC_ERR_HIP = -2
SPC_ERR_UNSUPPORTED = -3
SPC_ERR_NOMEM = -4
SPC_ERR_COMM = -5

MASK_NONE, MASK_ARRAY, MASK_FINITE = 0, 1, 2
MASK_GT, MASK_GE, MASK_LT, MASK_LE = 4, 8, 16, 32
COMM_ID_BYTES = 128
ABI_VERSION = 8
# spc_set_masked_spatial_form / spc_get_masked_spatial_form
SPATIAL_FORM_ENV, SPATIAL_FORM_SPLIT, SPATIAL_FORM_RING = -1, 0, 1
MAP_MUL, MAP_SECOND_MOMENT_SUM, MAP_DIV_ADD, MAP_DIV_SUB_SQ = 0, 1, 2, 3
# spc_ws_kind
(WS_MOMENTS, WS_SPECTRAL_CONV, WS_SPECTRAL_CONV_MOMENTS, WS_SPATIAL_CONV_SEP, WS_SPATIAL_CONV2D, WS_RESAMPLE_BILINEAR,
 WS_STATS_GLOBAL, WS_STATS_PLANES, WS_MAP_CONV2D, WS_CLIP_OUTSIDE, WS_PERCENTILE_GLOBAL, WS_SPATIAL_CONV_MFMA, WS_SIGMA_CLIP,
 WS_RESAMPLE_BILINEAR_LERP, WS_STATS_GLOBAL_F64, WS_SPECTRAL_CONV_F64, WS_SPATIAL_CONV_F64) = range(17)
# spc_ds_estimator (spc_downsample_f32 / _f64)
DS_NANMEAN, DS_NANSUM, DS_NANMAX, DS_NANMIN, DS_MEAN, DS_SUM, DS_MAX, DS_MIN = range(8)
# spc_rank_mode and the built window limits (spc_rank_filter_axis0_* / _plane_*)
RANK_MODES = {"reflect": 0, "constant": 1, "nearest": 2, "mirror": 3, "wrap": 4}
RANK_FILTER_MAX_KSIZE, RANK_FILTER_MAX_KSIZE_SPATIAL = 129, 15
# the longest padded spectrum of spc_stack_shift_* / spc_stack_sum_*
STACK_MAX_CHANNELS = 8192
# the most lines of spc_stack_cube_* and its spc_stack_cube_mode
STACK_CUBE_MAX_LINES = 64
STACK_CUBE_MODES = {"nanmean": 0, "mean": 1, "nansum": 2, "sum": 3}
# spc_mask_program (spc_mask_eval_f32 / _f64): limits, spc_mask_opcode, spc_mask_cmp, spc_mask_elem
MASK_PROG_MAX_SLOTS, MASK_PROG_MAX_OPERANDS, MASK_PROG_MAX_INSTR, MASK_PROG_MAX_STACK = 4, 8, 16, 8
MOP_CMP, MOP_FINITE, MOP_LOAD, MOP_NOT, MOP_AND, MOP_OR, MOP_XOR = range(7)
CMP_GT, CMP_GE, CMP_LT, CMP_LE, CMP_EQ, CMP_NE = range(6)
ELEM_F32, ELEM_F64, ELEM_U8 = range(3)
# spc_morph_op and the limits of the offset list (spc_mask_morph_u8)
MORPH_ERODE, MORPH_DILATE = 0, 1
MORPH_MAX_REACH, MORPH_MAX_OFFSETS = 3, 343
# spc_label_u8 / spc_label_objects_i32 / spc_label_select_i32: the most voxels (int32 linear indices), the flag's scratch
LABEL_MAX_VOXELS, LABEL_OBJECTS_WORKSPACE_BYTES = 2 ** 31 - 1, 256
# the groups of tables of spc_label_measure_f32 / _f64 (SPC_MEASURE_*)
MEASURE_SUMS, MEASURE_EXTREMA, MEASURE_FIRST, MEASURE_SECOND = 1, 2, 4, 8
# spc_arith_program (spc_arith_f32 / _f64): the step limit and spc_arith_opcode
ARITH_MAX_STEPS = 4
BASELINE_MAX_ORDER = 5          # SPC_BASELINE_MAX_ORDER
AOP_ADD, AOP_SUB, AOP_MUL, AOP_DIV, AOP_POW, AOP_SQUARE, AOP_SQRT, AOP_RECIP, AOP_ONE = range(9)
ARITH_OPCODES = {"add": AOP_ADD, "sub": AOP_SUB, "mul": AOP_MUL, "div": AOP_DIV, "pow": AOP_POW,
                 "square": AOP_SQUARE, "sqrt": AOP_SQRT, "recip": AOP_RECIP, "one": AOP_ONE}
ARITH_UNARY = ("square", "sqrt", "recip", "one")            # the exact power forms: no operand


class HipLibraryError(RuntimeError):
    """libspcube_hip.so is missing/unloadable, or a HIP call failed."""


class HipInvalidArgument(ValueError):
    pass


class HipUnsupported(NotImplementedError):
    pass


class SpcMask(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("thr_lo", C.c_float), ("thr_hi", C.c_float),
                ("d_array", C.c_void_p), ("row_stride", C.c_int64),
                ("plane_stride", C.c_int64)]


class SpcCube(C.Structure):
    _fields_ = [("d_data", C.c_void_p), ("nz", C.c_int64), ("ny", C.c_int64),
                ("nx", C.c_int64), ("row_stride", C.c_int64),
                ("plane_stride", C.c_int64)]


class SpcMomentOutputs(C.Structure):
    _fields_ = [("d_m0", C.c_void_p), ("d_m1", C.c_void_p), ("d_m2", C.c_void_p),
                ("d_mu", C.c_void_p), ("d_s0", C.c_void_p),
                ("d_argmax", C.c_void_p), ("d_argmin", C.c_void_p),
                ("d_vmax", C.c_void_p), ("d_vmin", C.c_void_p),
                ("d_nvalid", C.c_void_p), ("out_row_stride", C.c_int64)]


class SpcMomentsListDesc(C.Structure):
    """spc_moments_list_desc: the launch plan a list is made for"""
    _fields_ = [("zw", C.c_int32), ("nsplit", C.c_int32), ("zchunk", C.c_int64), ("nblocks", C.c_int64), ("nsub", C.c_int64)]


class SpcMomentsList(C.Structure):
    """spc_moments_list: the entry rows of the lane segments a mask includes (spc_moments_list_fill_f32 / spc_moments_list_f32)"""
    _fields_ = [("desc", SpcMomentsListDesc), ("d_samples", C.c_void_p), ("samples_bytes", C.c_size_t),
                ("d_meta", C.c_void_p), ("meta_bytes", C.c_size_t), ("d_off", C.c_void_p), ("d_len", C.c_void_p),
                ("nsublists", C.c_size_t), ("rows", C.c_uint64)]


class SpcMomentsVlist(C.Structure):
    """spc_moments_vlist: the 8-byte entries of the voxels a mask includes (spc_moments_vlist_fill_f32 / spc_moments_vlist_f32)"""
    _fields_ = [("desc", SpcMomentsListDesc), ("d_entries", C.c_void_p), ("entries_bytes", C.c_size_t),
                ("d_off", C.c_void_p), ("d_len", C.c_void_p), ("nsublists", C.c_size_t), ("rows", C.c_uint64)]


class SpcMask64(C.Structure):
    """spc_mask_f64: the mask of a float64 cube (thresholds compared in float64)"""
    _fields_ = [("flags", C.c_uint32), ("thr_lo", C.c_double), ("thr_hi", C.c_double),
                ("d_array", C.c_void_p), ("row_stride", C.c_int64), ("plane_stride", C.c_int64)]


class SpcMomentOutputs64(C.Structure):
    """spc_moment_outputs_f64 (no d_m2: moment 2 of a float64 cube is the second pass, spc_moment_order_f64)"""
    _fields_ = [("d_m0", C.c_void_p), ("d_m1", C.c_void_p), ("d_mu", C.c_void_p), ("d_s0", C.c_void_p),
                ("d_argmax", C.c_void_p), ("d_argmin", C.c_void_p), ("d_vmax", C.c_void_p), ("d_vmin", C.c_void_p),
                ("d_nvalid", C.c_void_p), ("out_row_stride", C.c_int64)]


class SpcCelestialWcs(C.Structure):
    _fields_ = [("proj", C.c_int32), ("sip_order", C.c_int32), ("crpix", C.c_double * 2), ("lin", C.c_double * 4),
                ("lin_inv", C.c_double * 4), ("alpha_p", C.c_double), ("delta_p", C.c_double), ("phi_p", C.c_double),
                ("pv1", C.c_double), ("plane0", C.c_double * 2), ("sip_a", C.c_double * 55), ("sip_b", C.c_double * 55)]


class SpcMosaicSource(C.Structure):
    """spc_mosaic_source_f32: one cube of spc_mosaic_f32 with its mask, fill value and pixel maps"""
    _fields_ = [("cube", SpcCube), ("mask", SpcMask), ("fill", C.c_float), ("d_xs", C.c_void_p), ("d_ys", C.c_void_p)]


class SpcMosaicSource64(C.Structure):
    """spc_mosaic_source_f64"""
    _fields_ = [("cube", SpcCube), ("mask", SpcMask64), ("fill", C.c_double), ("d_xs", C.c_void_p), ("d_ys", C.c_void_p)]


class SpcMaskSlot(C.Structure):
    _fields_ = [("d_data", C.c_void_p), ("row_stride", C.c_int64), ("plane_stride", C.c_int64)]


class SpcMaskOperand(C.Structure):
    _fields_ = [("d_data", C.c_void_p), ("elem", C.c_int32), ("reserved", C.c_int32),
                ("stride_z", C.c_int64), ("stride_y", C.c_int64), ("stride_x", C.c_int64)]


class SpcMaskInstr(C.Structure):
    _fields_ = [("opcode", C.c_int32), ("slot", C.c_int32), ("cmp", C.c_int32), ("operand", C.c_int32), ("imm", C.c_double)]


class SpcMaskProgram(C.Structure):
    """spc_mask_program: the postfix form of a mask tree (masks.compile_mask), run by spc_mask_eval_f32 / _f64"""
    _fields_ = [("n_slots", C.c_int32), ("n_operands", C.c_int32), ("n_instr", C.c_int32), ("reserved", C.c_int32),
                ("slots", SpcMaskSlot * MASK_PROG_MAX_SLOTS), ("operands", SpcMaskOperand * MASK_PROG_MAX_OPERANDS),
                ("instr", SpcMaskInstr * MASK_PROG_MAX_INSTR)]


class SpcArithStep(C.Structure):
    _fields_ = [("opcode", C.c_int32), ("refill", C.c_int32), ("is_scalar", C.c_int32), ("reserved", C.c_int32),
                ("scalar", C.c_double), ("d_data", C.c_void_p),
                ("stride_z", C.c_int64), ("stride_y", C.c_int64), ("stride_x", C.c_int64)]


class SpcArithProgram(C.Structure):
    """spc_arith_program: a chain of + - * / ** steps run in one pass by spc_arith_f32 / _f64"""
    _fields_ = [("n_steps", C.c_int32), ("reserved", C.c_int32), ("steps", SpcArithStep * ARITH_MAX_STEPS)]


class SpcStatsOutputs(C.Structure):
    _fields_ = [("d_count", C.c_void_p), ("d_min", C.c_void_p), ("d_max", C.c_void_p),
                ("d_sum", C.c_void_p), ("d_sumsq", C.c_void_p)]


class SpcLabelMeasureOutputs(C.Structure):
    """spc_label_measure_outputs: the tables of spc_label_measure_f32 / _f64, one pointer each; a group that is not wanted
    stays NULL"""
    _fields_ = [("d_count", C.c_void_p), ("d_sums", C.c_void_p), ("d_min", C.c_void_p), ("d_max", C.c_void_p),
                ("d_min_pos", C.c_void_p), ("d_max_pos", C.c_void_p), ("d_first", C.c_void_p), ("d_second", C.c_void_p)]


class SpcDeviceInfo(C.Structure):
    _fields_ = [("name", C.c_char * 128), ("arch", C.c_char * 64),
                ("compute_units", C.c_int), ("wavefront_size", C.c_int),
                ("total_mem", C.c_int64), ("free_mem", C.c_int64),
                ("clock_khz", C.c_int)]


_vp, _i, _i64, _sz, _d, _f = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_double, C.c_float
_P = C.POINTER

# name -> (restype, argtypes); mirrors include/spcube_hip.h one to one
SIGNATURES = {
    "spc_abi_version": (_i, []),
    "spc_last_error": (C.c_char_p, []),
    "spc_set_masked_spatial_form": (_i, [_i]),
    "spc_get_masked_spatial_form": (_i, []),
    "spc_device_count": (_i, [_P(_i)]),
    "spc_get_device_info": (_i, [_i, _P(SpcDeviceInfo)]),
    "spc_malloc": (_i, [_i, _sz, _P(_vp)]),
    "spc_free": (_i, [_i, _vp]),
    "spc_argextrema_axis_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i, _vp, _vp]),
    "spc_fill_masked_transpose_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _f, _vp]),
    "spc_percentile_global_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), C.c_double, _i, _f, _P(C.c_double), _vp, _sz]),
    "spc_percentile_groups_workspace_bytes": (_sz, [_i64]),
    "spc_percentile_groups_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i, _d, _vp, _f, _vp, _vp, _sz]),
    "spc_key_histogram_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), C.c_uint32, C.c_uint32, _i, _i, _f,
                                    _P(C.c_uint64), _P(C.c_uint32), _vp, _sz]),
    "spc_key_to_f32": (_f, [C.c_uint32]),
    "spc_clip_bounds_f32": (_i, [_i, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _d, _d, _vp, _vp]),
    "spc_wcs_pixel_map_f64": (_i, [_i, _vp, _P(SpcCelestialWcs), _P(SpcCelestialWcs), _P(C.c_double), _i64, _i64, _vp, _vp]),
    "spc_spatial_conv_sep_mfma_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _P(C.c_double), _i, _P(C.c_double), _i, _vp, _i64, _i64,
                                           _d, _vp, _i64, _vp, _sz]),
    "spc_spatial_conv_sep_mfma_moments_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _P(C.c_double), _i, _P(C.c_double), _i, _vp, _i64,
                                                   _i64, _vp, _d, _d, _vp, _vp, _vp, _i64, _vp, _sz]),
    "spc_map_check": (_i, [_i, _vp, _vp, C.c_int32, _vp, _i64, _vp]),
    "spc_resample_spline_f32": (_i, [_i, _vp, _P(SpcCube), _i, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _sz]),
    "spc_stats_planes_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _P(C.c_double), _vp, _sz]),
    "spc_pool_trim": (_i, [_i]),
    "spc_pool_stats": (_i, [_i, _P(C.c_int64), _P(C.c_int64)]),
    "spc_host_alloc": (_i, [_sz, _P(_vp)]),
    "spc_host_free": (_i, [_vp]),
    "spc_memcpy_h2d": (_i, [_i, _vp, _vp, _sz, _vp]),
    "spc_memcpy_d2h": (_i, [_i, _vp, _vp, _sz, _vp]),
    "spc_memcpy_d2d": (_i, [_i, _vp, _vp, _sz, _vp]),
    "spc_memcpy3d_h2d": (_i, [_i, _vp, _sz, _sz, _vp, _sz, _sz, _sz, _sz, _sz, _vp]),
    "spc_memcpy3d_d2d": (_i, [_i, _vp, _sz, _sz, _vp, _sz, _sz, _sz, _sz, _sz, _vp]),
    "spc_memset": (_i, [_i, _vp, _i, _sz, _vp]),
    "spc_stream_create": (_i, [_i, _P(_vp)]),
    "spc_stream_destroy": (_i, [_i, _vp]),
    "spc_stream_sync": (_i, [_i, _vp]),
    "spc_device_sync": (_i, [_i]),
    "spc_event_create": (_i, [_i, _P(_vp)]),
    "spc_event_destroy": (_i, [_i, _vp]),
    "spc_event_record": (_i, [_i, _vp, _vp]),
    "spc_event_sync": (_i, [_i, _vp]),
    "spc_stream_wait_event": (_i, [_i, _vp, _vp]),
    "spc_event_elapsed_ms": (_i, [_i, _vp, _vp, _P(_f)]),
    "spc_moments_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "spc_workspace_bytes": (_sz, [_i, _i64, _i64, _i64, _i64, _i64]),
    "spc_moments_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _vp, _d, _d,
                             _P(SpcMomentOutputs), _vp, _sz]),
    "spc_mask_bits_bytes": (_sz, [_i64, _i64, _i64]),
    "spc_mask_pack_bits": (_i, [_i, _vp, _i64, _i64, _i64, _P(SpcMask), _vp, _sz]),
    "spc_moments_bits_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _vp, _d, _d,
                                  _P(SpcMomentOutputs), _vp, _sz, _vp, _sz]),
    "spc_moments_list_plan_f32": (_i, [_P(SpcCube), _P(SpcMask), _P(SpcMomentOutputs), _vp, _sz, _P(SpcMomentsListDesc)]),
    "spc_moments_list_count_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _P(SpcMomentOutputs), _vp, _sz, _vp, _sz, _vp, _vp, _sz,
                                        _P(SpcMomentsListDesc)]),
    "spc_moments_list_fill_f32": (_i, [_i, _vp, _P(SpcCube), _vp, _sz, _P(SpcMomentsList)]),
    "spc_moments_list_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _vp, _d, _d,
                                  _P(SpcMomentOutputs), _vp, _sz, _vp, _sz, _P(SpcMomentsList)]),
    "spc_moments_vlist_count_f32": (_i, [_i, _vp, _P(SpcMomentsList), _vp, _sz]),
    "spc_moments_vlist_fill_f32": (_i, [_i, _vp, _P(SpcMomentsList), _P(SpcMomentsVlist)]),
    "spc_moments_vlist_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _vp, _d, _d,
                                   _P(SpcMomentOutputs), _vp, _sz, _vp, _sz, _P(SpcMomentsList), _P(SpcMomentsVlist)]),
    "spc_moment_order_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _vp, _i, _vp, _vp, _vp, _i64]),
    # (spc_cube_f64 has the layout of spc_cube_f32: a pointer and five int64)
    "spc_moments_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _vp, _d, _d, _P(SpcMomentOutputs64)]),
    "spc_moment_order_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _vp, _i, _vp, _vp, _vp, _i64]),
    "spc_stats_global_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _P(_d), _vp, _sz]),
    "spc_stats_axis_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _i, _P(SpcStatsOutputs)]),
    "spc_spectral_conv_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _P(_d), _i, _vp, _i64, _i64, _vp, _sz]),
    "spc_spatial_conv_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _P(_d), _i, _P(_d), _i, _i, _vp, _i64, _i64, _vp, _sz]),
    "spc_spectral_lerp_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _i64, _vp, _vp, _vp, _d, _vp, _i64, _i64]),
    "spc_resample_bilinear_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _d, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _i, _vp]),
    "spc_scale_f64": (_i, [_i, _vp, _vp, _i64, _d]),
    "spc_percentile_axis0_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _d, _vp, _d, _vp]),
    "spc_sigma_clip_axis0_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _d, _d, _i, _i, _i, _vp]),
    "spc_narrow_f64_to_f32": (_i, [_i, _vp, _P(SpcCube), _vp, _i64, _i64]),
    "spc_mask_include_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _i, _vp]),
    "spc_downsample_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i, _f, _i, _i64, _i, _i, _vp, _i64, _i64, _vp]),
    "spc_downsample_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _i, _d, _i, _i64, _i, _i, _vp, _i64, _i64, _vp]),
    "spc_subcube_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i, _P(_i64), _P(_i64), _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i, _f]),
    "spc_subcube_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _i, _P(_i64), _P(_i64), _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i, _d]),
    "spc_pv_extract_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i, _f, _i64, _i64, _vp, _vp, _i, _i, _vp, _i64, _vp, _i64]),
    "spc_pv_extract_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _i, _d, _i64, _i64, _vp, _vp, _i, _i, _vp, _i64, _vp, _i64]),
    "spc_baseline_segments": (_i64, [_i64, _i64, _i64, _i64]),
    "spc_baseline_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _i]),
    "spc_baseline_fit_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i, _vp, _i64, _vp, _vp, _vp, _vp, _sz]),
    "spc_baseline_fit_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _i, _vp, _i64, _vp, _vp, _vp, _vp, _sz]),
    "spc_baseline_apply_f32": (_i, [_i, _vp, _P(SpcCube), _i, _vp, _vp, _i, _vp, _i64, _i64]),
    "spc_baseline_apply_f64": (_i, [_i, _vp, _P(SpcCube), _i, _vp, _vp, _i, _vp, _i64, _i64]),
    "spc_mask_bbox_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i, _vp]),
    "spc_mask_bbox_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _i, _vp]),
    "spc_mask_eval_f32": (_i, [_i, _vp, _i64, _i64, _i64, _P(SpcMaskProgram), _vp, _i64, _i64]),
    "spc_mask_eval_f64": (_i, [_i, _vp, _i64, _i64, _i64, _P(SpcMaskProgram), _vp, _i64, _i64]),
    "spc_mask_morph_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "spc_mask_morph_u8": (_i, [_i, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i, _vp, _i, _i, _i, _vp, _vp, _sz,
                               _P(_i64)]),
    "spc_label_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "spc_label_u8": (_i, [_i, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _sz, _P(_i64)]),
    "spc_label_objects_i32": (_i, [_i, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _sz]),
    "spc_label_select_i32": (_i, [_i, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp]),
    "spc_label_measure_workspace_bytes": (_sz, [_i64, C.c_uint32]),
    "spc_label_measure_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _vp, _i64, _vp, C.c_uint32, _P(SpcLabelMeasureOutputs), _vp, _sz]),
    "spc_label_measure_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _vp, _i64, _vp, C.c_uint32, _P(SpcLabelMeasureOutputs), _vp, _sz]),
    "spc_arith_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i, _f, _P(SpcArithProgram), _vp, _i64, _i64]),
    "spc_arith_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _i, _d, _P(SpcArithProgram), _vp, _i64, _i64]),
    "spc_rank_filter_axis0_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i, _f, _i, _i, _i, _f, _vp, _i64, _i64]),
    "spc_rank_filter_axis0_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _i, _d, _i, _i, _i, _d, _vp, _i64, _i64]),
    "spc_rank_filter_plane_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i, _f, _i, _i, _i, _i, _f, _vp, _i64, _i64]),
    "spc_rank_filter_plane_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _i, _d, _i, _i, _i, _i, _d, _vp, _i64, _i64]),
    "spc_stack_workspace_bytes": (_sz, [_i64, _i64, _i, _i, _i]),
    "spc_stack_shift_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i, _f, _vp, _vp, _i64, _i, _i, _vp, _vp, _sz]),
    "spc_stack_shift_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _i, _d, _vp, _vp, _i64, _i, _i, _vp, _vp, _sz]),
    "spc_stack_sum_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i, _f, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _sz]),
    "spc_stack_sum_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _i, _d, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _sz]),
    "spc_stack_cube_workspace_bytes": (_sz, [_i, _i64]),
    "spc_stack_cube_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i, _f, _i, _vp, _vp, _vp, _vp, _i, _i64, _vp, _vp, _sz]),
    "spc_stack_cube_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _i, _d, _i, _vp, _vp, _vp, _vp, _i, _i64, _vp, _vp, _sz]),
    "spc_mosaic_workspace_bytes": (_sz, [_i]),
    "spc_mosaic_f32": (_i, [_i, _vp, _i, _P(SpcMosaicSource), _i64, _i64, _i64, _i, _vp, _vp, _vp, _sz]),
    "spc_mosaic_f64": (_i, [_i, _vp, _i, _P(SpcMosaicSource64), _i64, _i64, _i64, _i, _vp, _vp, _vp, _sz]),
    "spc_moments_spatial_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i, _vp, _d, _vp, _vp, _vp]),
    "spc_moment_order_spatial_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i, _vp, _i, _vp, _vp]),
    "spc_spectral_conv_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _P(_d), _i, _vp, _i64, _i64, _vp, _sz]),
    "spc_spectral_conv_moments_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _P(_d), _i, _vp, _P(_d), _d, _d,
                                           _P(SpcMomentOutputs), _vp, _sz]),
    "spc_spatial_conv_sep_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _P(_d), _i, _P(_d), _i,
                                      _vp, _i64, _i64, _vp, _sz]),
    "spc_spatial_conv2d_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _P(_d), _i, _i, _vp, _i64, _i64, _vp, _sz]),
    "spc_spectral_lerp_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i64, _vp, _vp, _vp, _f,
                                   _vp, _i64, _i64]),
    "spc_resample_bilinear_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _f, _i64, _i64, _vp, _vp,
                                       _vp, _i64, _i64, _vp, _i, _vp, _vp, _sz]),
    "spc_resample_bilinear_lerp_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _f, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp,
                                            _vp, _i64, _i64, _vp, _i, _vp, _vp, _sz]),
    "spc_percentile_axis0_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _d, _vp, _f, _vp]),
    "spc_percentile_axis2_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _d, _vp, _f, _vp]),
    "spc_mask_include_u8": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i, _vp]),
    "spc_fill_masked_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _f, _vp, _i64, _i64]),
    "spc_sigma_clip_axis0_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _d, _d, _i, _i, _i, _vp, _vp, _sz]),
    "spc_clip_outside_f32": (_i, [_i, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _P(C.c_uint64), _vp, _sz]),
    "spc_map_conv2d_f64": (_i, [_i, _vp, _vp, _i64, _i64, _P(_d), _i, _i, _vp, _vp, _sz]),
    "spc_map_arith_f64": (_i, [_i, _vp, _i, _vp, _vp, _vp, _d, _vp, _i64]),
    "spc_scale_f32": (_i, [_i, _vp, _vp, _i64, _d]),
    "spc_fits_to_f32": (_i, [_i, _vp, _vp, _i, _d, _d, _i, _i64, _i64, _vp]),
    "spc_fits_to_f64": (_i, [_i, _vp, _vp, _i, _d, _d, _i, _i64, _i64, _vp]),
    "spc_stats_global_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _P(_d), _vp, _sz]),
    "spc_stats_axis_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i, _P(SpcStatsOutputs)]),
    "spc_stats_m2_axis_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i, _vp, _vp, _vp]),
    "spc_stats_m2_axis_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _i, _vp, _vp, _vp]),
    "spc_stats_dev_axis_f32": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask), _i, _d, _vp, _vp]),
    "spc_stats_dev_axis_f64": (_i, [_i, _vp, _P(SpcCube), _P(SpcMask64), _i, _d, _vp, _vp]),
    "spc_comm_unique_id": (_i, [_P(C.c_uint8)]),
    "spc_comm_init": (_i, [_i, _P(C.c_uint8), _i, _i, _P(_vp)]),
    "spc_comm_destroy": (_i, [_vp]),
    "spc_allgather_rows": (_i, [_vp, _vp, _vp, _vp, _sz]),
    "spc_allgather_rows_batch": (_i, [_vp, _vp, _i, _P(_vp), _P(_vp), _P(_sz)]),
}

_lib = None
_lock = threading.Lock()
_load_error = None


def load():
    """Load the shared library once and declare every prototype."""
    global _lib, _load_error
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            _load_error = ("%s not found - build it with `python -c 'import __graft_entry__ as g; "
                           "g.build()'` or `make -C spectral_cube_amd/csrc`" % LIB_PATH)
            raise HipLibraryError(_load_error)
        try:
            lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        except OSError as exc:  # missing ROCm runtime etc.
            _load_error = "cannot load %s: %s" % (LIB_PATH, exc)
            raise HipLibraryError(_load_error)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError = ABI mismatch, keep it loud
            fn.restype = res
            fn.argtypes = args
        if lib.spc_abi_version() != ABI_VERSION:
            raise HipLibraryError("ABI version mismatch: %d" % lib.spc_abi_version())
        _lib = lib
        return _lib


def last_error():
    msg = load().spc_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc):
    """Translate a spc_status into the exception the reference would raise."""
    if rc == SPC_OK:
        return
    msg = last_error()
    if rc == SPC_ERR_INVALID:
        raise HipInvalidArgument(msg)
    if rc == SPC_ERR_UNSUPPORTED:
        raise HipUnsupported(msg)
    if rc == SPC_ERR_NOMEM:
        raise MemoryError(msg)
    raise HipLibraryError("status %d: %s" % (rc, msg))


def call(name, *args):
    lib = load()
    check(getattr(lib, name)(*args))


def device_count():
    n = C.c_int(0)
    call("spc_device_count", C.byref(n))
    return n.value


def require_gpu():
    if device_count() < 1:
        raise HipLibraryError("no HIP device visible: the spectral_cube_amd product path has no CPU fallback")
