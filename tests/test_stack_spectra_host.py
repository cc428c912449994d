"""stack_spectra's host side (spectral_cube_amd/analysis_utilities.py): the bookkeeping against the reference's results
(tests/golden/stack_spectra.npz), every error and warning, unit handling, and the C ABI of the new entry points.  No GPU."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

from conftest import golden
import spectral_cube_amd
from spectral_cube_amd import SpectralCube, BadVelocitiesWarning, UnitsError, _lib, ops, stack_spectra
from spectral_cube_amd.analysis_utilities import _finish, _fused_name, stack_plan
from spectral_cube_amd.wcs import parse_header

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX = 7


def fixture_cases():
    G = golden("stack_spectra.npz")
    keys = [str(k) for k in G["keys"]]
    stops = np.cumsum(G["npos"])
    pkeys = [str(k) for k in G["pkeys"]]
    for i, key in enumerate(keys):
        variant, case = key.split("|")
        hdr = parse_header(str(G[variant + "|header"]))
        d = G[variant + "|data"]
        cube = SpectralCube(d, header=hdr)
        if case == "bool0":
            cube = cube.with_mask(G[variant + "|keep"]).with_fill_value(0.0)
        sl = slice(stops[i] - G["npos"][i], stops[i])
        idx, shifts = G["idx"][sl], G["shifts"][sl]
        kw = {}
        if G["explicit_posns"][i]:
            kw["xy_posns"] = (idx // NX, idx % NX)
        if np.isfinite(G["v0"][i]):
            kw["v0"] = float(G["v0"][i])                    # km/s, like the velocities
        yield G, key, cube, G["vels"][i], idx, shifts, kw, [(j, p) for j, p in enumerate(pkeys) if p.startswith(key + "|")]


def test_bookkeeping_matches_the_reference():
    n = 0
    for G, key, cube, vel, idx, shifts, kw, pk in fixture_cases():
        for j, pkey in pk:
            pad_edges = pkey.endswith("pad1")
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", BadVelocitiesWarning)
                gi, gs, gpad = stack_plan(cube, vel, pad_edges=pad_edges, **kw)
            assert np.array_equal(gi, idx), pkey
            assert np.array_equal(np.isnan(gs), np.isnan(shifts)), pkey
            ok = np.isfinite(shifts)
            assert np.abs(gs[ok] - shifts[ok]).max() <= 1e-9, pkey       # (velocities of ~1e4 m/s over 500 m/s: 1e-12 relative)
            assert tuple(gpad) == tuple(G["pads"][j]), pkey
            nz = cube.shape[0]
            assert nz + gpad[0] + gpad[1] == G["naxis1"][j]
            assert cube.wcs.spectral_only().header["CRPIX1"] + gpad[0] == G["crpix1"][j]
            n += 1
    assert n == 30


def _cube(nz=8, cdelt=0.5):
    hdr = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CDELT1": -1e-3, "CDELT2": 1e-3, "CDELT3": cdelt,
           "CUNIT3": "km/s", "CRPIX1": 1, "CRPIX2": 1, "CRPIX3": 1, "CRVAL1": 10.0, "CRVAL2": 20.0, "CRVAL3": 3.0, "BUNIT": "K"}
    return SpectralCube(np.ones((nz, 3, 4), np.float32), header=hdr)


def test_errors_in_the_reference_order():
    cube = _cube()
    axis = cube.spectral_axis
    good = np.full((3, 4), axis[3])
    with pytest.raises(ValueError, match="no finite values"):
        stack_plan(cube, np.full((3, 4), np.nan))
    with pytest.raises(ValueError, match="no finite values"):      # (checked before the shape)
        stack_plan(cube, np.full((2, 2), np.nan))
    with pytest.raises(ValueError, match="does not match cube spatial"):
        stack_plan(cube, np.full((4, 3), axis[3]))
    for bad in (axis.min() - 0.1, axis.max() + 0.1):
        with pytest.raises(ValueError, match="v0 must be within the range"):
            stack_plan(cube, good, v0=bad)
    stack_plan(cube, good, v0=axis.max())                            # the ends themselves are inside


def test_non_linear_axis_is_refused(monkeypatch):
    cube = _cube()
    axis = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.6])
    monkeypatch.setattr(SpectralCube, "spectral_axis", property(lambda self: axis))
    with pytest.raises(ValueError, match="Cannot shift spectra on a non-linear axes"):
        stack_plan(cube, np.full((3, 4), 1.0))
    stack_plan(cube, np.full((3, 4), 1.0), vdiff_tol=0.25)          # 0.6 against 0.5 passes a tolerance of 25 %


def test_out_of_range_velocities_warn_and_are_masked_strictly():
    cube = _cube()
    axis = cube.spectral_axis
    vel = np.full((3, 4), axis[3])
    vel[0, 0] = axis.max()                  # equal to an end: no warning on its own ...
    with warnings.catch_warnings():
        warnings.simplefilter("error", BadVelocitiesWarning)
        idx, s, pad = stack_plan(cube, vel)
        assert np.isfinite(s).all() and idx.size == 12
    vel[1, 1] = axis.max() + 1.0
    vel[2, 2] = np.nan
    with pytest.warns(BadVelocitiesWarning, match="outside the allowed range"):
        idx, s, pad = stack_plan(cube, vel)
    assert idx.size == 11                    # the out-of-range velocity stays in the list, the NaN does not
    assert np.isnan(s[list(idx).index(5)])   # ... with a NaN shift
    assert np.isnan(s[0])                    # and once masking happens, the strict compare masks the end as well
    assert np.isfinite(np.delete(s, [0, list(idx).index(5)])).all()


def test_shifts_sign_padding_and_default_v0():
    for cdelt, sign in ((0.5, -1.0), (-0.5, 1.0)):
        cube = _cube(9, cdelt)
        axis = cube.spectral_axis
        vel = np.full((3, 4), axis.mean())
        vel[0, 1] = axis.mean() + 1.3 * 0.5
        vel[0, 2] = axis.mean() - 2.0 * 0.5
        idx, s, pad = stack_plan(cube, vel)
        assert np.allclose(s[1], sign * 1.3) and np.allclose(s[2], sign * -2.0) and np.allclose(np.delete(s, [1, 2]), 0.0)
        lo, hi = min(0, int(np.ceil(s.min()))), max(0, int(np.ceil(s.max())))
        assert pad == (-lo, hi) and pad in ((1, 2), (2, 2))
        assert stack_plan(cube, vel, pad_edges=False)[2] == (0, 0)
        assert stack_plan(cube, np.full((3, 4), axis[1]), v0=axis[1])[2] == (0, 0)      # only zero shifts: nothing to pad


def test_units_of_surface_and_v0():
    cube = _cube()
    axis = cube.spectral_axis

    class Q:
        def __init__(self, value, unit):
            self.value, self.unit = value, unit
            self.shape = np.shape(value)
    vel = np.full((3, 4), axis[2])
    vel[1, 1] = axis[5]
    base = stack_plan(cube, vel, v0=axis[4])
    in_ms = stack_plan(cube, Q(vel * 1000.0, "m/s"), v0=Q(axis[4] * 1000.0, "m / s"))
    assert np.array_equal(base[0], in_ms[0]) and np.allclose(base[1], in_ms[1], rtol=0, atol=1e-12) and base[2] == in_ms[2]
    with pytest.raises(UnitsError):
        stack_plan(cube, Q(vel, "Hz"))
    with pytest.raises(UnitsError):
        stack_plan(cube, vel, v0=Q(1.0, "GHz"))


def test_stack_functions_recognised_and_finished():
    assert [_fused_name(f) for f in (np.nanmean, np.mean, np.nansum, np.sum)] == ["nanmean", "mean", "nansum", "sum"]

    def nanmean(a, axis=0):
        return None
    assert _fused_name(nanmean) == "nanmean"
    assert _fused_name(np.nanmedian) is None and _fused_name(np.median) is None and _fused_name(lambda a, axis: a) is None
    rows = np.array([[1.0, np.nan, 2.0, np.nan], [3.0, 4.0, np.nan, np.nan], [5.0, 6.0, 7.0, np.nan]])
    total, count = np.nansum(rows, axis=0), np.isfinite(rows).sum(axis=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name in ("nanmean", "mean", "nansum", "sum"):
            assert np.array_equal(_finish(name, total, count, 3 - count, 3), getattr(np, name)(rows, axis=0), equal_nan=True), name


def test_no_cpu_fallback(monkeypatch):
    def no_gpu():
        raise _lib.HipLibraryError("no HIP device visible")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    cube = _cube()
    with pytest.raises(_lib.HipLibraryError):
        stack_spectra(cube, np.full((3, 4), cube.spectral_axis[3]), num_cores=4, chunk_size=10, progressbar=True)


# ---- the C ABI --------------------------------------------------------------------------------------------------
NEW = ("spc_stack_shift_f32", "spc_stack_shift_f64", "spc_stack_sum_f32", "spc_stack_sum_f64")


def test_entry_points_exported_and_declared():
    lib = _lib.load()
    assert lib.spc_abi_version() == 8 == _lib.ABI_VERSION
    text = open(os.path.join(REPO, "include", "spcube_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name + " is not declared in include/spcube_hip.h"
    assert hasattr(lib, "spc_stack_workspace_bytes") and "spc_stack_workspace_bytes" in _lib.SIGNATURES
    for cited in ("134-318", "14-78", "81-94"):
        assert cited in text
    assert re.search(r"#define\s+SPC_STACK_MAX_CHANNELS\s+%d\b" % _lib.STACK_MAX_CHANNELS, text)
    assert spectral_cube_amd.analysis_utilities.stack_spectra is stack_spectra


def test_workspace_query_and_argument_checks_before_any_launch():
    lib = _lib.load()
    assert lib.spc_stack_workspace_bytes(24, 41, 3, 4, 0) >= 2 * 31 * 8
    assert lib.spc_stack_workspace_bytes(24, 41, 3, 4, 1) > lib.spc_stack_workspace_bytes(24, 41, 3, 4, 0)
    assert lib.spc_stack_workspace_bytes(4096, 15, 2048, 2048, 1) > 0 and lib.spc_stack_workspace_bytes(4096, 15, 2048, 2049, 1) == 0
    c = _lib.SpcCube()
    buf = (C.c_float * 64)()
    c.d_data = C.addressof(buf)
    c.nz, c.ny, c.nx, c.row_stride, c.plane_stride = 4, 4, 4, 4, 16
    idx, sh, out = (C.c_int32 * 4)(), (C.c_double * 4)(), (C.c_double * 64)()
    pi, ps, po = (C.c_void_p(C.addressof(a)) for a in (idx, sh, out))

    def shift(npos=4, pad=(0, 0), d_idx=pi, d_out=po):
        return lib.spc_stack_shift_f32(0, None, C.byref(c), None, 0, 0.0, d_idx, ps, npos, pad[0], pad[1], d_out, None, 0)
    for call, status, word in ((lambda: shift(d_out=None), _lib.SPC_ERR_INVALID, b"NULL"), (lambda: shift(d_idx=None), _lib.SPC_ERR_INVALID, b"NULL"),
                               (lambda: shift(npos=0), _lib.SPC_ERR_INVALID, b"positions"), (lambda: shift(pad=(-1, 0)), _lib.SPC_ERR_INVALID, b"pads"),
                               (lambda: shift(pad=(8000, 189)), _lib.SPC_ERR_UNSUPPORTED, b"8192"),
                               (lambda: lib.spc_stack_sum_f32(0, None, C.byref(c), None, 0, 0.0, pi, ps, 4, 0, 0, None, None, None, None, 0),
                                _lib.SPC_ERR_INVALID, b"NULL")):
        assert call() == status and word in lib.spc_last_error(), (word, lib.spc_last_error())


class _StandInArray:
    """what ops.py reads of a DeviceArray, without a device"""

    def __init__(self, shape, dtype, device=0):
        self.shape, self.dtype, self.device, self.ptr = tuple(int(n) for n in shape), np.dtype(dtype), device, 0x1000
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize

    @classmethod
    def from_numpy(cls, arr, device=0, stream=None, dtype=None):
        a = np.asarray(arr, dtype=dtype)
        out = cls(a.shape, a.dtype, device)
        out.host = a
        return out


def test_ops_reach_the_entry_point_of_the_cubes_dtype(monkeypatch):
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops, "DeviceArray", _StandInArray)
    for dtype, suffix, struct in ((np.float32, "_f32", _lib.SpcMask), (np.float64, "_f64", _lib.SpcMask64)):
        del calls[:]
        cube = _StandInArray((6, 5, 4), dtype)
        out = ops.stack_shift(cube, [0, 7, 19], [0.5, -1.25, np.nan], pad=(2, 1), fill=0.25, nan_excluded=True)
        assert out.shape == (9, 3) and out.dtype == np.float64
        (name, a), = calls
        assert name == "spc_stack_shift" + suffix and type(a[3]._obj) is struct and len(a) == len(_lib.SIGNATURES[name][1])
        assert a[4:6] == (1, 0.25) and a[8:11] == (3, 2, 1)
    for bad in (lambda: ops.stack_shift(cube, [20], [0.0]), lambda: ops.stack_shift(cube, [-1], [0.0]),
                lambda: ops.stack_shift(cube, [1, 2], [0.0]), lambda: ops.stack_shift(cube, [], []),
                lambda: ops.stack_shift(cube, [1], [0.0], pad=(-1, 0))):
        with pytest.raises((ValueError, IndexError)):
            bad()
    with pytest.raises(TypeError):
        ops.stack_sum(_StandInArray((6, 5, 4), np.int16), [0], [0.0])
