"""CPU: the Pending record a cube -> cube operator leaves in ``_lazy`` - every field the consumers read (out-of-core strips
and slabs, the fused smooth -> moment paths, the interpolation reproject folds in, write() / stream_into()), stated per
producer.  No kernel runs here.  The records of ``reproject`` need a device before they exist (the pixel map, the
one-plane probe of the footprint): they are left to the GPU tests (tests/test_gpu_round3.py, test_gpu_round4.py)."""
import warnings

import numpy as np
import pytest

from spectral_cube_amd import _lib, Gaussian1DKernel, Gaussian2DKernel, SpectralCube, VaryingResolutionSpectralCube
from spectral_cube_amd.beam import Beam
from spectral_cube_amd.cube import _ArithPending
from spectral_cube_amd.kernels import kernel_array
from spectral_cube_amd.pending import Pending
from spectral_cube_amd.streaming import HugeCubeError

HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CDELT1": -1e-3, "CDELT2": 1e-3, "CDELT3": 0.5,
       "CUNIT3": "km/s", "CRPIX1": 4, "CRPIX2": 3, "CRPIX3": 1, "CRVAL1": 10.0, "CRVAL2": 20.0, "CRVAL3": -16.0, "BUNIT": "K"}
BEAM, TARGET = Beam(2e-3, 1.5e-3, 10.0), Beam(4e-3, 4e-3, 0.0)
K1, K2 = Gaussian1DKernel(1.0), Gaussian2DKernel(0.7)
GRID = -16.0 + 0.75 * np.arange(7)          # km/s, inside the cube's axis


def _cube(**hdr):
    d = np.random.default_rng(3).normal(size=(12, 9, 10)).astype(np.float32)
    keep = np.random.default_rng(4).random(d.shape) < 0.8
    return SpectralCube(d, header=dict(HDR, **hdr)).with_mask(keep)


FIELDS = ("op", "strips", "slabs", "halo", "keeps_mask", "fusable", "arithmetic")
DEFAULTS = dict(strips=False, slabs=False, halo=0, keeps_mask=False, fusable=False, arithmetic=None)

# operator -> (call, the declared fields that differ from the defaults, has a kernel, has a lerp plan)
TABLE = {
    "spectral_smooth": (lambda c: c.spectral_smooth(K1), dict(strips=True, keeps_mask=True, fusable=True), 1, False),
    "spatial_smooth": (lambda c: c.spatial_smooth(K2, arithmetic="f32"),
                       dict(strips=True, slabs=True, halo=kernel_array(K2, 2).shape[0] // 2, keeps_mask=True, arithmetic="f32"), 2, False),
    "spectral_filter": (lambda c: c.spectral_smooth_median(3), dict(strips=True, keeps_mask=True), 0, False),
    "spatial_filter": (lambda c: c.spatial_smooth_median(3), dict(slabs=True, keeps_mask=True), 0, False),
    "spectral_interpolate": (lambda c: c.spectral_interpolate(GRID), dict(strips=True), 0, True),
    # (the two below are pending only for a parent above the budget; of a resident parent they run at once)
    "sigma_clip_spectrally": (lambda c: c.sigma_clip_spectrally(3.0), dict(strips=True, keeps_mask=True), 0, False),
    "convolve_to": (lambda c: c.with_beam(BEAM).convolve_to(TARGET), dict(slabs=True, keeps_mask=True), 0, False),
}
OUT_OF_CORE_ONLY = ("sigma_clip_spectrally", "convolve_to")
# the budget: 1G - the parent is resident; 2k - the 4320-byte cube is out of core
CASES = [(name, budget) for name in sorted(TABLE) for budget in ("1G", "2k") if budget == "2k" or name not in OUT_OF_CORE_ONLY]


@pytest.mark.parametrize("name,budget", CASES)
def test_the_record_of_every_producer(name, budget, monkeypatch):
    monkeypatch.setenv("SPC_HBM_BUDGET", budget)
    call, declared, kernel_ndim, has_lerp = TABLE[name]
    cube = _cube()
    out = call(cube)
    rec = out._lazy
    assert type(rec) is Pending and out._dev is None                  # nothing ran
    want = dict(DEFAULTS, op=name, **declared)
    assert {f: getattr(rec, f) for f in FIELDS} == want
    assert rec.parent._data_id is cube._data_id and (name == "convolve_to" or rec.parent is cube)
    assert callable(rec.fn) and rec.run is None
    if kernel_ndim:
        assert np.array_equal(rec.kernel, kernel_array(K1 if kernel_ndim == 1 else K2, kernel_ndim))
    else:
        assert rec.kernel is None
    if has_lerp:
        (lo, t, inv_dx), fill = rec.lerp
        assert len(lo) == len(t) == len(inv_dx) == len(GRID) and np.isnan(fill)
        assert out.shape == (len(GRID), 9, 10) and out.mask is not cube.mask
    else:
        assert rec.lerp is None and out.shape == cube.shape and out.mask is cube.mask
    if budget == "2k":
        # never resident: materialising asks the parent for its samples, which names the budget
        monkeypatch.setattr(_lib, "require_gpu", lambda: None)
        with pytest.raises(HugeCubeError, match="SPC_HBM_BUDGET"):
            out._device_data()


def test_spatial_smooth_without_an_arithmetic_declares_none(monkeypatch):
    monkeypatch.setenv("SPC_HBM_BUDGET", "1G")
    assert _cube().spatial_smooth(K2)._lazy.arithmetic is None


def test_per_channel_beams_convolve_in_slabs_out_of_core(monkeypatch):
    monkeypatch.setenv("SPC_HBM_BUDGET", "2k")
    d = np.random.default_rng(8).normal(size=(12, 9, 10)).astype(np.float32)
    beams = [Beam(2e-3 + 1e-5 * (k // 3), 1.5e-3, 10.0) for k in range(12)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cube = VaryingResolutionSpectralCube(d, header=HDR, beams=beams)
        out = cube.convolve_to(TARGET)
    rec = out._lazy
    assert type(out) is SpectralCube and type(rec) is Pending and rec.op == "convolve_to" and rec.parent is cube
    assert (rec.slabs, rec.strips, rec.halo, rec.keeps_mask, rec.fusable) == (True, False, 0, True, False)
    assert out._strip_plan(True)[0] is cube
    monkeypatch.setattr(_lib, "require_gpu", lambda: None)
    with pytest.raises(HugeCubeError, match="SPC_HBM_BUDGET"):
        out._device_data()


def test_out_of_core_plan_takes_the_declared_route(monkeypatch):
    """_strip_plan hands the streamed parent and a fn(dev, mspec, stream); a record without a route, or whose parent is
    resident, gives None"""
    cube = _cube()
    monkeypatch.setenv("SPC_HBM_BUDGET", "1G")
    assert cube.spectral_smooth(K1)._strip_plan(True) is None
    monkeypatch.setenv("SPC_HBM_BUDGET", "2k")
    sm = cube.spectral_smooth(K1)
    src, fn, nz_out = sm._strip_plan(True)
    assert src is cube and callable(fn) and fn is not sm._lazy.fn and nz_out == 12       # filled under the parent's mask
    assert sm._strip_plan(False)[1] is sm._lazy.fn
    interp = cube.spectral_interpolate(GRID)
    assert interp._strip_plan(True)[1:] == (interp._lazy.fn, len(GRID))                  # its data are their own fill
    assert cube.spatial_smooth(K2)._strip_halo() == kernel_array(K2, 2).shape[0] // 2 and sm._strip_halo() == 0
    assert sm._fusable()[0] is cube and cube.spatial_smooth(K2)._fusable() is None and interp._fusable() is None


def test_plain_deferred_results_have_no_operator_and_no_route(monkeypatch):
    monkeypatch.setenv("SPC_HBM_BUDGET", "1G")
    cube = _cube(BUNIT="")
    total = cube + 1.0
    for out in (total, cube[2:8, 1:, :5], cube.downsample_axis(2, 0)):
        rec = out._lazy
        assert type(rec) is Pending and out._dev is None
        assert rec.op is None and rec.parent is None and rec.fn is None and callable(rec.run)
        assert (rec.strips, rec.slabs, rec.halo, rec.keeps_mask, rec.fusable) == (False, False, 0, False, False)
        assert rec.kernel is None and rec.lerp is None and rec.arithmetic is None
        assert out._strip_plan(True) is None and out._fusable() is None and out._strip_halo() == 0
    assert type(total._arith) is _ArithPending and total._lazy.run is total._arith


def test_bare_callable_is_wrapped_and_runs_once():
    calls, sentinel = [], object()
    cube = SpectralCube(None, header=HDR, _shape=(12, 9, 10), _lazy=lambda: calls.append(1) or sentinel)
    assert type(cube._lazy) is Pending and cube._lazy.op is None and cube._lazy.parent is None
    assert cube._device_data() is sentinel and cube._device_data() is sentinel
    assert calls == [1] and cube._lazy is None
    rec = Pending(run=lambda: sentinel)
    assert SpectralCube(None, header=HDR, _shape=(12, 9, 10), _lazy=rec)._lazy is rec          # a record is taken as it is


def test_derived_views_carry_the_same_record(monkeypatch):
    monkeypatch.setenv("SPC_HBM_BUDGET", "1G")
    sm = _cube().spectral_smooth(K1)
    rec = sm._lazy
    for out in (sm.with_mask(np.ones(sm.shape, bool)), sm.with_fill_value(0.0), sm.with_spectral_unit("m/s"), sm.with_beam(BEAM)):
        assert out._lazy is rec and out._dev is None


def test_pending_rejects_what_is_not_a_field():
    with pytest.raises(TypeError):
        Pending(run=lambda: None, strip_fn=lambda dev, mspec, stream: dev)       # a misspelt route is an error, not "not streamable"
    with pytest.raises(AttributeError):
        Pending(run=lambda: None).slab_fn = None
    with pytest.raises(TypeError):
        Pending()                                                                # neither run() nor fn + parent
    with pytest.raises(TypeError):
        Pending(run=lambda: None, strips=True)                                   # a route without fn and parent
