"""CPU: the host side of stack_cube (analysis_utilities.py:321-432) against tests/golden/stack_cube.npz, the reference's
results through its Dask class (tools/gen_golden_stack_cube.py), and the float64 numpy restatement of its steps 1 - 5 that
the GPU tests check the kernels against.

The reference's mask on a decreasing grid.  Its spectral_interpolate takes ``~isnan`` of the result as the new mask before
it flips the result back to a decreasing output grid (dask_spectral_cube.py:1364-1367): the mask is then the mirror image,
along the spectral axis, of the one that fits the data, and the cutout stack_cube averages has the fill value wherever the
data OR its mirror image is NaN.  Every ``inc`` case of the fixture (increasing frequency = decreasing velocity) is affected.
``restate(..., mirror=True)`` has that line as the reference has it and must reproduce every recorded array, NaN pattern
exactly; ``mirror=False`` is the mask that fits the data - what this project builds - and the two differ only in that line.
"""
import warnings

import numpy as np
import pytest

from conftest import golden
from spectral_cube_amd import SpectralCube, HipUnsupported, _lib, stack_cube
from spectral_cube_amd.analysis_utilities import stack_cube_plan
from spectral_cube_amd.wcs import parse_header

C_KMS = 299792.458
FUSED = ("nanmean", "mean", "nansum", "sum")


# ---- the restatement: steps 1 - 5 in float64 numpy, never the library ----------------------------------------------
def slab_plan(freq, lines, vmin, vmax):
    """[(line, ilo, ihi, velocity axis of the whole cube)] of the lines whose slab has more than one channel"""
    out = []
    for f0 in lines:
        v = C_KMS * (f0 - freq) / f0
        a, b = int(np.argmin(np.abs(v - vmin))), int(np.argmin(np.abs(v - vmax)))
        if abs(a - b) + 1 > 1:
            out.append((f0, min(a, b), max(a, b), v))
    return out


def interp(x, y, grid, mirror):
    """DaskSpectralCubeMixin.spectral_interpolate (dask_spectral_cube.py:1291-1373): (data, include)"""
    rin, rout = np.mean(np.diff(x)) < 0, np.mean(np.diff(grid)) < 0
    if rin:
        x, y = x[::-1], y[::-1]
    if rout:
        grid = grid[::-1]
    idx = np.clip(np.searchsorted(x, grid), 1, len(x) - 1)
    lo = idx - 1
    with np.errstate(invalid="ignore"):
        slope = (y[idx] - y[lo]) / (x[idx] - x[lo])[:, None, None]
        new = slope * (grid - x[lo])[:, None, None] + y[lo]
    new[(grid < x[0]) | (grid > x[-1])] = np.nan
    include = ~np.isnan(new)                                  # :1364, before the flip of :1366-1367
    if rout:
        new = new[::-1]
        if not mirror:
            include = include[::-1]
    return new, include


def restate(d, inc, fill, freq, lines, vmin, vmax, mirror=False):
    """(cutouts, plan): the filled first slab and every other slab interpolated onto its velocity axis, in float64"""
    plan = slab_plan(freq, lines, vmin, vmax)
    d64 = np.asarray(d, dtype=np.float64)
    f0, ilo, ihi, v = plan[0]
    grid = v[ilo:ihi + 1]
    cuts = [np.where(inc, d64, fill)[ilo:ihi + 1]]
    for f0, ilo, ihi, v in plan[1:]:
        new, include = interp(v[ilo:ihi + 1], np.where(inc, d64, np.nan)[ilo:ihi + 1], grid, mirror)
        cuts.append(np.where(include, new, fill))
    return cuts, plan


def average(name, cuts):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return getattr(np, name)(cuts, axis=0)


def freq_axis(hdr, nz):
    return hdr["CRVAL3"] + hdr["CDELT3"] * (np.arange(nz) + 1.0 - hdr["CRPIX3"])


def fixture():
    """[(key, cube, data, include, fill, freq, lines)] of tests/golden/stack_cube.npz, and the file"""
    G = golden("stack_cube.npz")
    out = []
    for variant in (str(v) for v in G["variants"]):
        d, keep = G[variant + "|data"], G[variant + "|keep"]
        hdr = parse_header(str(G[variant + "|header"]))
        for case in (str(c) for c in G["cases"]):
            key = variant + "|" + case
            cube, inc, fill = SpectralCube.read(d, hdr), np.isfinite(d), np.nan
            if case == "bool0":
                cube, inc, fill = cube.with_mask(keep).with_fill_value(0.0), inc & keep, 0.0
            out.append((key, cube, d, inc, fill, freq_axis(hdr, d.shape[0]), G[key + "|lines"]))
    return G, out


def scale_of(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.abs(a[np.isfinite(a)]).max())


# ---- the plan ------------------------------------------------------------------------------------------------------
def test_plan_reproduces_the_reference_bounds_grid_and_wcs():
    G, cases = fixture()
    assert len(cases) == 6 and float(G["margin"]) >= 1e-6
    vmin, vmax = float(G["vmin"]), float(G["vmax"])
    for key, cube, d, inc, fill, freq, lines in cases:
        P = stack_cube_plan(cube, lines, vmin, vmax)
        assert np.array_equal(np.array(P.windows), G[key + "|bounds"]), key
        assert np.array_equal(np.array(P.lines, dtype=np.float64), G[key + "|included"]), key
        assert len(P.lines) == (4 if key.endswith("l5") else 3) and P.cube_index == [0] * len(P.lines)
        np.testing.assert_allclose(P.grid, G[key + "|grid"], rtol=1e-12, atol=0.0)
        h = P.wcs.header
        np.testing.assert_allclose([h["CRPIX3"], h["CRVAL3"], h["CDELT3"]], G[key + "|wcs3"], rtol=1e-12, atol=0.0)
        assert h["CTYPE3"] == str(G[key + "|ctype3"]) == "VRAD"
        assert h["CUNIT3"] == "km/s" and str(G[key + "|cunit3"]).replace(" ", "") in ("kms-1", "km/s")
        assert not any(k in h for k in ("RESTFRQ", "RESTFREQ", "RESTWAV")) and h["NAXIS3"] == P.grid.size
        assert h["CTYPE1"] == cube.header["CTYPE1"] and h["CRVAL2"] == cube.header["CRVAL2"]
        np.testing.assert_allclose(P.wcs.spectral_pix2world(np.arange(P.grid.size)), P.grid, rtol=1e-12, atol=0.0)
        # the tables: the reference slab copied, everything else inside its own window or -1
        n0 = P.grid.size
        assert P.lo.shape == P.t.shape == P.inv_dx.shape == (len(P.lines), n0) and P.lo.dtype == np.int32
        assert list(P.exact) == [1] + [0] * (len(P.lines) - 1)
        assert np.array_equal(P.lo[0], P.windows[0][0] + np.arange(n0))
        for s in range(1, len(P.lines)):
            ilo, ihi = P.windows[s]
            inside = P.lo[s] >= 0
            assert (P.lo[s][~inside] == -1).all() and (P.lo[s][inside] >= ilo).all() and (P.lo[s][inside] + 1 <= ihi).all()
        if key.endswith("l5"):
            assert P.windows[2][0] == 0 and (P.lo[2] == -1).any(), "the window that runs off the band edge"


def emulate(d, inc, fill, P):
    """the arithmetic the kernel is specified to do with the tables (include/spcube_hip.h), in numpy"""
    d64 = np.asarray(d, dtype=np.float64)
    filled, nanned = np.where(inc, d64, fill), np.where(inc, d64, np.nan)
    cuts = []
    for s in range(P.lo.shape[0]):
        lo = P.lo[s]
        if P.exact[s]:
            cuts.append(filled[lo])
            continue
        a, b = nanned[np.clip(lo, 0, None)], nanned[np.clip(lo, 0, None) + 1]
        with np.errstate(invalid="ignore"):
            c = (b - a) * (P.inv_dx[s] * P.t[s])[:, None, None] + a
        c[lo < 0] = np.nan
        cuts.append(np.where(np.isnan(c), fill, c))
    return cuts


def test_tables_give_the_restatement():
    G, cases = fixture()
    for key, cube, d, inc, fill, freq, lines in cases:
        P = stack_cube_plan(cube, lines, float(G["vmin"]), float(G["vmax"]))
        exp, _ = restate(d, inc, fill, freq, lines, float(G["vmin"]), float(G["vmax"]))
        got = emulate(d, inc, fill, P)
        for s, (a, b) in enumerate(zip(got, exp)):
            assert np.array_equal(np.isnan(a), np.isnan(b)), (key, s)
            ok = np.isfinite(b)
            assert np.abs(a[ok] - b[ok]).max() <= 1e-11 * scale_of(d), (key, s)


# ---- the restatement against the reference ---------------------------------------------------------------------------
def test_restatement_reproduces_the_reference():
    G, cases = fixture()
    dist = float(G["restatement_distance"])
    assert 0.0 < dist < 8 * 2.0 ** -24
    funcs = [str(f) for f in G["funcs"]]
    assert funcs == ["nanmean", "mean", "nansum", "nanmedian"]
    differ = 0
    for key, cube, d, inc, fill, freq, lines in cases:
        vmin, vmax = float(G["vmin"]), float(G["vmax"])
        mirrored, plan = restate(d, inc, fill, freq, lines, vmin, vmax, mirror=True)
        fitting, _ = restate(d, inc, fill, freq, lines, vmin, vmax, mirror=False)
        decreasing_grid = plan[0][3][1] < plan[0][3][0]
        assert decreasing_grid == key.startswith("inc")
        if not decreasing_grid:                               # the one line the two differ in does not run
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(mirrored, fitting))
        scale = scale_of(d)
        for k, fname in enumerate(funcs):
            ref = G[key + "|stacks"][k]
            mine = average(fname, mirrored)
            assert np.array_equal(np.isnan(mine), np.isnan(ref)), (key, fname)
            ok = np.isfinite(ref)
            assert np.abs(mine[ok] - ref[ok]).max() <= dist * scale * (len(mirrored) if "sum" in fname else 1), (key, fname)
            differ += int((~np.isclose(mine, average(fname, fitting), rtol=1e-9, atol=0.0, equal_nan=True)).sum())
        if key + "|cutouts" in G.files:
            for a, b in zip(G[key + "|cutouts"], mirrored):
                assert np.array_equal(np.isnan(a), np.isnan(b)) and np.abs(a - b)[np.isfinite(a)].max() <= dist * scale
    assert differ == int(G["mirror_differs"]) > 0


# ---- argument checks -------------------------------------------------------------------------------------------------
HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "FREQ", "CUNIT3": "Hz", "CDELT1": -1e-3, "CDELT2": 1e-3,
       "CDELT3": 0.5e6, "CRPIX1": 2, "CRPIX2": 2, "CRPIX3": 1, "CRVAL1": 10.0, "CRVAL2": 20.0, "CRVAL3": 100e9, "BUNIT": "K"}


class Q:
    def __init__(self, value, unit):
        self.value, self.unit = value, unit


def test_argument_checks():
    d = np.zeros((40, 3, 4), np.float32)
    cube = SpectralCube.read(d, HDR)
    f = freq_axis(HDR, 40)
    for bad in (dict(HDR, CTYPE3="VRAD", CUNIT3="km/s", CDELT3=1.0, CRVAL3=0.0, RESTFRQ=100e9), dict(HDR, CTYPE3="WAVE", CUNIT3="m"),
                dict(HDR, CTYPE3="VOPT", CUNIT3="m/s")):
        with pytest.raises(NotImplementedError, match=bad["CTYPE3"]):
            stack_cube(SpectralCube.read(d, bad), [f[10]], -5.0, 5.0)
    with pytest.raises(ValueError):
        stack_cube(cube, [f[0] - 1e9, f[-1] + 1e9], -5.0, 5.0)                # every line outside the band
    with pytest.raises(ValueError, match="spatial shape"):
        stack_cube([cube, SpectralCube.read(np.zeros((40, 3, 5), np.float32), HDR)], [f[10]], -5.0, 5.0)
    lines = list(f[10] + 0.1e6 * np.arange(_lib.STACK_CUBE_MAX_LINES + 1))
    with pytest.raises(HipUnsupported, match=str(_lib.STACK_CUBE_MAX_LINES)):
        stack_cube(cube, lines, -5.0, 5.0)
    with pytest.raises(HipUnsupported):
        stack_cube(cube, lines, -5.0, 5.0, average=np.sum)
    # quantities: rest values in any frequency unit, bounds in any speed unit, either order
    P = stack_cube_plan(cube, [f[10], f[25]], -5.0, 5.0)
    Pq = stack_cube_plan(cube, [Q(f[10] / 1e9, "GHz"), Q(f[25] / 1e6, "MHz")], Q(5000.0, "m/s"), Q(-5.0, "km/s"))
    assert Pq.windows == P.windows and np.array_equal(Pq.lo, P.lo) and np.allclose(Pq.grid, P.grid, rtol=1e-12)
    with pytest.raises(ValueError):
        stack_cube_plan(cube, [f[10]], Q(1.0, "GHz"), 5.0)
    # with_spectral_unit still refuses the conversion (the frequency-to-velocity step lives in stack_cube)
    with pytest.raises(NotImplementedError):
        cube.with_spectral_unit("km/s", velocity_convention="radio", rest_value=f[10])


def test_exports_and_abi():
    import os
    import re
    from conftest import REPO
    lib = _lib.load()
    text = open(os.path.join(REPO, "include", "spcube_hip.h")).read()
    for name in ("spc_stack_cube_f32", "spc_stack_cube_f64"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name + " is not declared in include/spcube_hip.h"
    assert _lib.STACK_CUBE_MAX_LINES == int(re.search(r"#define SPC_STACK_CUBE_MAX_LINES (\d+)", text).group(1)) == 64
    assert lib.spc_abi_version() == 8
    assert lib.spc_stack_cube_workspace_bytes(8, 64) >= 8 * 64 * 20
