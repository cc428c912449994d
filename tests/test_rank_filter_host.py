"""CPU: the host side of the median / rank filters (spectral_smooth_median, spectral_filter, spatial_smooth_median,
spatial_filter): argument checking, filter recognition, rank arithmetic, what the pending result keeps of its parent, the
entry points reached and the C ABI.  No kernel runs here."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

from conftest import REPO
from spectral_cube_amd import _lib, ops, SpectralCube
from spectral_cube_amd.beam import Beam
from spectral_cube_amd.cube import BeamUnitsError, VaryingResolutionSpectralCube, _rank_filter_options

HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CDELT1": -1e-3, "CDELT2": 1e-3, "CDELT3": 0.5,
       "CUNIT3": "km/s", "CRPIX1": 4, "CRPIX2": 3, "CRPIX3": 1, "CRVAL1": 10.0, "CRVAL2": 20.0, "CRVAL3": -16.0, "BUNIT": "K"}


def _cube(shape=(12, 9, 10), dtype=np.float32, **hdr):
    d = np.random.default_rng(3).normal(size=shape).astype(dtype)
    return SpectralCube.read(d, dict(HDR, **hdr))


def _stand_in(name):
    """a function object that only shares its name with scipy.ndimage's (the package never imports scipy)"""
    def fn(*a, **k):
        raise AssertionError("the filter function itself is never called")
    fn.__name__ = name
    return fn


# ---- the rank a filter selects ----------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, 9, 15, 25, 129])
def test_median_minimum_maximum_ranks(w):
    assert _rank_filter_options("median_filter", w, {})[0] == w // 2
    assert _rank_filter_options("minimum_filter", w, {})[0] == 0
    assert _rank_filter_options("maximum_filter", w, {})[0] == w - 1
    assert _rank_filter_options(_stand_in("median_filter"), w, {})[0] == w // 2


def test_rank_filter_rank_counts_from_either_end():
    assert _rank_filter_options("rank_filter", 9, {"rank": 2})[0] == 2
    assert _rank_filter_options("rank_filter", 9, {"rank": -1})[0] == 8
    assert _rank_filter_options("rank_filter", 9, {"rank": -9})[0] == 0
    assert _rank_filter_options("rank_filter", 9, {"rank": np.int64(3)})[0] == 3
    for bad in (9, -10):
        with pytest.raises(ValueError, match="rank"):
            _rank_filter_options("rank_filter", 9, {"rank": bad})
    with pytest.raises(TypeError):
        _rank_filter_options("rank_filter", 9, {})
    with pytest.raises(TypeError):
        _rank_filter_options("rank_filter", 9, {"rank": 2.5})


def test_percentile_filter_follows_scipys_rule():
    # negative values wrap by 100, 100 is the last sample, otherwise int(w * p / 100.0)
    cases = [(9, 50, 4), (9, 0, 0), (9, 100, 8), (9, 99.9, 8), (9, -50, 4), (9, -100, 0), (4, 50, 2), (5, 20, 1), (25, 33.3, 8),
             (7, 14.2, 0), (7, 14.3, 1), (3, 66.7, 2), (129, 75, 96)]
    for w, p, rank in cases:
        assert _rank_filter_options("percentile_filter", w, {"percentile": p})[0] == rank, (w, p)
    for bad in (100.5, -100.5):
        with pytest.raises(ValueError, match="percentile"):
            _rank_filter_options("percentile_filter", 9, {"percentile": bad})
    with pytest.raises(TypeError):
        _rank_filter_options("percentile_filter", 9, {})


def test_keywords():
    assert _rank_filter_options("median_filter", 3, {})[1:] == ("reflect", 0.0)
    assert _rank_filter_options("median_filter", 3, {"mode": "constant", "cval": 2.5})[1:] == ("constant", 2.5)
    for mode in ("reflect", "constant", "nearest", "mirror", "wrap"):
        assert _rank_filter_options("median_filter", 3, {"mode": mode})[1] == mode
    ignored = dict(use_memmap=False, verbose=3, num_cores=4, parallel=True, update_function=print, save_to_tmp_dir=True)
    assert _rank_filter_options("maximum_filter", 5, ignored) == (4, "reflect", 0.0)
    assert _rank_filter_options("median_filter", 3, {"origin": 0, "footprint": None})[0] == 1
    assert _rank_filter_options("median_filter", 9, {"origin": (0, 0)})[0] == 4
    with pytest.raises(NotImplementedError, match="origin"):
        _rank_filter_options("median_filter", 3, {"origin": 1})
    with pytest.raises(NotImplementedError, match="origin"):
        _rank_filter_options("median_filter", 9, {"origin": (0, -1)})
    with pytest.raises(NotImplementedError, match="footprint"):
        _rank_filter_options("median_filter", 3, {"footprint": np.ones(3, bool)})
    with pytest.raises(ValueError, match="mode"):
        _rank_filter_options("median_filter", 3, {"mode": "grid-wrap"})
    with pytest.raises(TypeError, match="bogus"):
        _rank_filter_options("median_filter", 3, {"bogus": 1})
    with pytest.raises(TypeError, match="rank"):
        _rank_filter_options("median_filter", 3, {"rank": 1})


@pytest.mark.parametrize("bad", ["gaussian_filter", "uniform_filter", "generic_filter", np.median, None, 3])
def test_anything_outside_the_rank_family_names_what_is_supported(bad):
    cube = _cube()
    f = _stand_in(bad) if isinstance(bad, str) else bad
    for call in (lambda: cube.spectral_filter(3, f), lambda: cube.spatial_filter(3, f)):
        with pytest.raises(NotImplementedError) as err:
            call()
        for name in ("median_filter", "minimum_filter", "maximum_filter", "percentile_filter", "rank_filter"):
            assert name in str(err.value)


# ---- ksize ------------------------------------------------------------------------------------------------------
def test_spectral_ksize():
    cube = _cube()
    for ok in (1, 2, 3, 5.0, np.int32(4), np.float32(7.0), 9):
        assert cube.spectral_smooth_median(ok).shape == cube.shape
    for bad in (2.5, "three", None, (3, 3), [3], True):
        with pytest.raises(TypeError, match="ksize should be an integer"):
            cube.spectral_smooth_median(bad)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="at least 1"):
            cube.spectral_smooth_median(bad)
    with pytest.raises(ValueError, match="129"):
        _cube((140, 2, 2)).spectral_smooth_median(131)
    assert _cube((140, 2, 2)).spectral_smooth_median(129).shape == (140, 2, 2)
    # a window may reach one axis length past an edge, not more: ksize // 2 <= nz
    assert cube.spectral_smooth_median(25).shape == cube.shape            # 12 channels, reach 12
    with pytest.raises(ValueError, match="ksize // 2 <= 12"):
        cube.spectral_smooth_median(26)


def test_spatial_ksize():
    cube = _cube()
    for ok in (1, 3, 4.0, (3, 5), [3, 3], np.array([5, 3]), (2.0, 7), 15, (15, 1)):
        assert cube.spatial_smooth_median(ok).shape == cube.shape
    for bad in (2.5, (3, 2.5), (3, 3, 3), (3,), "3", None, (True, 3)):
        with pytest.raises(TypeError, match="ksize should be an integer or a pair"):
            cube.spatial_smooth_median(bad)
    for bad in (0, (3, 0), (-1, 3)):
        with pytest.raises(ValueError, match="at least 1"):
            cube.spatial_smooth_median(bad)
    for bad in (17, (3, 16)):
        with pytest.raises(ValueError, match="15"):
            _cube((2, 40, 40)).spatial_smooth_median(bad)
    small = _cube((4, 3, 2))
    assert small.spatial_smooth_median((7, 5)).shape == (4, 3, 2)          # reach 3 rows, 2 columns
    with pytest.raises(ValueError, match="ksize // 2 <= 3"):
        small.spatial_smooth_median((8, 3))
    with pytest.raises(ValueError, match="ksize // 2 <= 2"):
        small.spatial_smooth_median((3, 6))


def test_only_the_spatial_methods_check_jy_per_beam():
    cube = _cube(BUNIT="Jy/beam")
    for call in (lambda **k: cube.spatial_smooth_median(3, **k), lambda **k: cube.spatial_filter(3, "maximum_filter", **k)):
        with pytest.raises(BeamUnitsError):
            call()
        assert call(raise_error_jybm=False).unit == cube.unit
    assert cube.spectral_smooth_median(3).shape == cube.shape
    assert cube.spectral_filter(3, "minimum_filter").shape == cube.shape


# ---- the pending result -----------------------------------------------------------------------------------------
def test_result_is_pending_and_keeps_mask_fill_wcs_unit_meta():
    d = np.random.default_rng(5).normal(size=(12, 9, 10)).astype(np.float32)
    keep = np.random.default_rng(6).random(d.shape) < 0.7
    cube = SpectralCube(d, header=HDR, meta={"origin": "test"}).with_mask(keep).with_fill_value(0.0)
    for out in (cube.spectral_smooth_median(3), cube.spectral_filter(5, "rank_filter", rank=-2, mode="wrap"),
                cube.spatial_smooth_median([3, 3]), cube.spatial_filter((3, 5), _stand_in("percentile_filter"), percentile=30)):
        assert type(out) is SpectralCube and out.shape == cube.shape
        assert out._dev is None and out._lazy is not None            # nothing ran
        assert out.mask is cube.mask and out.fill_value == 0.0
        assert out.wcs is cube.wcs and out.unit == cube.unit == "K" and out.meta == cube.meta
        assert out.header["CRVAL3"] == cube.header["CRVAL3"]
    # the out-of-core routes each declares: strips of whole spaxels along the spectral axis, slabs of whole planes per plane
    for out in (cube.spectral_smooth_median(3), cube.spectral_filter(5, "rank_filter", rank=-2, mode="wrap")):
        assert out._lazy.strips is True and out._lazy.slabs is False
    for out in (cube.spatial_smooth_median(3), cube.spatial_filter((3, 5), _stand_in("percentile_filter"), percentile=30)):
        assert out._lazy.slabs is True and out._lazy.strips is False


def test_varying_resolution_cube_keeps_its_beams():
    d = np.random.default_rng(8).normal(size=(5, 6, 7)).astype(np.float32)
    beams = [Beam(2e-3 + 1e-4 * k, 1.5e-3, 10.0) for k in range(5)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cube = VaryingResolutionSpectralCube(d, header=HDR, beams=beams)
        for out in (cube.spectral_smooth_median(3), cube.spatial_smooth_median(3)):
            assert isinstance(out, VaryingResolutionSpectralCube)
            assert out.unmasked_beams == beams


class _StandInArray:
    """what ops.py reads of a DeviceArray, without a device"""

    def __init__(self, shape, dtype, device=0):
        self.shape, self.dtype, self.device, self.ptr = tuple(int(n) for n in shape), np.dtype(dtype), device, 0x1000
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize


@pytest.fixture
def recorded_calls(monkeypatch):
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops, "DeviceArray", _StandInArray)
    return calls


def test_ops_reach_the_entry_point_of_the_cubes_dtype(recorded_calls):
    for dtype, suffix, struct in ((np.float32, "_f32", _lib.SpcMask), (np.float64, "_f64", _lib.SpcMask64)):
        del recorded_calls[:]
        cube = _StandInArray((6, 5, 4), dtype)
        out = ops.rank_filter_axis0(cube, 5, 2, mode="mirror", cval=1.5, fill=0.25, mask=ops.MaskSpec(_lib.MASK_GT, thr_lo=0.1),
                                    nan_excluded=True)
        out2 = ops.rank_filter_plane(cube, 3, 5, 14, mode="constant", cval=2.5)
        assert out.dtype == out2.dtype == np.dtype(dtype) and out.shape == out2.shape == (6, 5, 4)
        (n1, a1), (n2, a2) = recorded_calls
        assert n1 == "spc_rank_filter_axis0" + suffix and n2 == "spc_rank_filter_plane" + suffix
        assert type(a1[3]._obj) is struct
        # device, stream, cube, mask, nan_excluded, fill, ksize, rank, mode, cval, out, strides
        assert a1[4:10] == (1, 0.25, 5, 2, _lib.RANK_MODES["mirror"], 1.5) and len(a1) == len(_lib.SIGNATURES[n1][1])
        assert a2[4:11] == (0, a2[5], 3, 5, 14, _lib.RANK_MODES["constant"], 2.5) and np.isnan(a2[5])
        assert len(a2) == len(_lib.SIGNATURES[n2][1])
    with pytest.raises(ValueError, match="mode"):
        ops.rank_filter_axis0(_StandInArray((6, 5, 4), np.float32), 3, 1, mode="periodic")
    with pytest.raises(TypeError):
        ops.rank_filter_axis0(_StandInArray((6, 5, 4), np.int16), 3, 1)
    with pytest.raises(ValueError):
        ops.rank_filter_plane(_StandInArray((6, 5, 4), np.float32), 3, 3, 4, out=_StandInArray((6, 5, 4), np.float64))


def test_the_package_does_not_import_scipy():
    import subprocess
    import sys
    code = ("import sys; import spectral_cube_amd as s, numpy as np; "
            "c = s.SpectralCube(np.zeros((4, 3, 2), np.float32)); c.spectral_smooth_median(3); c.spatial_filter(3, 'maximum_filter'); "
            "assert not any(m == 'scipy' or m.startswith('scipy.') for m in sys.modules)")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=REPO)


# ---- the C ABI --------------------------------------------------------------------------------------------------
NEW = ("spc_rank_filter_axis0_f32", "spc_rank_filter_axis0_f64", "spc_rank_filter_plane_f32", "spc_rank_filter_plane_f64")


def test_entry_points_exported_and_declared():
    lib = _lib.load()
    assert lib.spc_abi_version() == 8 == _lib.ABI_VERSION
    text = open(os.path.join(REPO, "include", "spcube_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name + " is not declared in include/spcube_hip.h"
    for cited in ("2844-2898", "2749-2806", "920-960", "995-1029", "147-172"):
        assert cited in text
    assert re.search(r"#define\s+SPC_RANK_FILTER_MAX_KSIZE\s+%d\b" % _lib.RANK_FILTER_MAX_KSIZE, text)
    assert re.search(r"#define\s+SPC_RANK_FILTER_MAX_KSIZE_SPATIAL\s+%d\b" % _lib.RANK_FILTER_MAX_KSIZE_SPATIAL, text)
    modes = dict(re.findall(r"SPC_RANK_([A-Z]+)\s*=\s*(\d+)", text))
    assert {k.lower(): int(v) for k, v in modes.items()} == _lib.RANK_MODES


def test_invalid_arguments_are_reported_before_any_launch():
    lib = _lib.load()
    c = _lib.SpcCube()
    buf = (C.c_float * 64)()
    c.d_data = C.addressof(buf)
    c.nz, c.ny, c.nx, c.row_stride, c.plane_stride = 4, 4, 4, 4, 16
    out = (C.c_float * 64)()
    o = C.c_void_p(C.addressof(out))

    def axis0(ksize, rank, mode=0, dst=o):
        return lib.spc_rank_filter_axis0_f32(0, None, C.byref(c), None, 0, 0.0, ksize, rank, mode, 0.0, dst, 0, 0)

    def plane(ky, kx, rank, mode=0):
        return lib.spc_rank_filter_plane_f32(0, None, C.byref(c), None, 0, 0.0, ky, kx, rank, mode, 0.0, o, 0, 0)
    for call, word in ((lambda: axis0(0, 0), b"ksize"), (lambda: axis0(130, 0), b"129"), (lambda: axis0(11, 5), b"axis length"),
                       (lambda: axis0(3, 3), b"rank"), (lambda: axis0(3, -1), b"rank"), (lambda: axis0(3, 1, mode=5), b"mode"),
                       (lambda: axis0(3, 1, dst=None), b"NULL"),
                       (lambda: axis0(3, 1, dst=C.c_void_p(C.addressof(buf))), b"in place"),
                       (lambda: plane(0, 3, 0), b"ksize"), (lambda: plane(3, 16, 0), b"15"),
                       (lambda: plane(11, 3, 0), b"axis length"), (lambda: plane(3, 3, 9), b"rank")):
        assert call() == _lib.SPC_ERR_INVALID and word in lib.spc_last_error(), (word, lib.spc_last_error())
