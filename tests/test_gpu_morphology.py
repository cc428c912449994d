"""GPU: binary mask morphology (csrc/spc_mask_morph.hip through ops.mask_morph and spectral_cube_amd.morphology) against
scipy.ndimage.  Booleans have no tolerance: every result is np.array_equal to scipy's."""
import functools

import numpy as np
import pytest
import scipy.ndimage as ndi

import dirty_memory
import morphology as R
import views
from spectral_cube_amd import _lib, morphology, ops, SpectralCube
from spectral_cube_amd import masks as M
from spectral_cube_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CDELT1": -1e-3, "CDELT2": 1e-3, "CDELT3": 0.5,
       "CUNIT3": "km/s", "CRPIX1": 4, "CRPIX2": 3, "CRPIX3": 1, "CRVAL1": 10.0, "CRVAL2": 20.0, "CRVAL3": -16.0, "BUNIT": "K"}
CASES = R.cases()


def up(a):
    return None if a is None else DeviceArray.from_numpy(np.asarray(a, dtype=bool).astype(np.uint8))


def run(x, structure, op, iterations=1, mask=None, border_value=0, **kw):
    out = ops.mask_morph(up(x), R.offsets(structure), op, iterations=iterations, mask=up(mask), border_value=border_value, **kw)
    if isinstance(out, tuple):
        return out[0].get().view(bool), out[1]
    got = out.get()
    assert got.max() <= 1                                # the bytes are 0 / 1, whatever the input bytes were
    return got.view(bool)


def check(x, structure, op, iterations=1, mask=None, border_value=0, what=""):
    exp = R.scipy_morph(x, structure, op, iterations, mask, border_value)
    got = run(x, structure, op, iterations, mask, border_value)
    assert np.array_equal(got, exp), "%s: %d voxels differ, first %s" % (what, (got != exp).sum(), np.argwhere(got != exp)[:4].tolist())


# ---- the host case table ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted({c.split("-")[0] for c, _ in CASES}))
def test_case_table(gpu, name):
    n = 0
    for cid, kw in CASES:
        if cid.split("-")[0] == name:
            check(what=cid, **kw)
            n += 1
    assert n >= 64


# ---- x extents around the 32-voxel words ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [1, 31, 32, 33, 36, 63, 64, 65, 70, 100, 130])
def test_row_lengths_around_a_word(gpu, nx):
    shape = (3, 4, nx)
    x = R.field(shape, nx, 0.3)
    x[:, :, -1] |= R.field((3, 4), nx + 1, 0.5)                       # voxels at the end of a row, next to the padding bits
    mask = R.field(shape, nx + 2, 0.7)
    reach3 = np.ones((1, 1, 7), bool)                                  # 3 voxels across a word seam either way
    lop = np.array([1, 0, 0, 1, 1, 0, 1], bool).reshape(1, 1, 7)
    for s in (R.generate_binary_structure(3, 1), reach3, lop, np.ones((2, 3, 6), bool)):
        for op in (R.ERODE, R.DILATE):
            xx = ~x if op == R.ERODE else x
            for border in (0, 1):                                      # 1: a row's tail must read as the border, not as zero
                for it, m in ((1, None), (2, None), (1, mask), (0, mask)):
                    if it < 1 and not s[tuple(n // 2 for n in s.shape)]:
                        continue
                    check(xx, s, op, it, m, border, what="nx=%d %s op=%d it=%d border=%d" % (nx, s.shape, op, it, border))


@pytest.mark.parametrize("shape", [(1, 5, 40), (5, 1, 40), (1, 1, 70), (1, 6, 1)])
def test_structure_taller_than_the_axis(gpu, shape):
    x, mask = R.field(shape, 7, 0.4), R.field(shape, 8, 0.7)
    for s in (np.ones((7, 7, 1), bool), np.ones((5, 5, 5), bool), R.generate_binary_structure(3, 3), R._pattern((7, 6, 3), 3, True)):
        for op in (R.ERODE, R.DILATE):
            for border in (0, 1):
                for it, m in ((1, None), (2, mask), (0, mask)):
                    check(x, s, op, it, m, border, what="%s %s op=%d it=%d border=%d" % (shape, s.shape, op, it, border))


@pytest.mark.parametrize("shape", [(70000, 2, 3), (2, 3, 70000), (2, 70000, 3)])
def test_one_long_axis(gpu, shape):
    x = R.field(shape, 1, 0.05)
    s = R.generate_binary_structure(3, 1)
    check(x, s, R.DILATE, 2, what="dilate %s" % (shape,))
    check(~x, s, R.ERODE, 2, border_value=1, what="erode %s" % (shape,))


# ---- propagation ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corridor(shape):
    """(mask, input): the serpentine corridor with its one seed; a second seed on a one-voxel island of the mask that the
    corridor does not reach (it must stay exactly itself); a voxel of the input outside the mask (kept, and it does not spread)"""
    m, seed = R.serpentine(shape)
    x = np.zeros(shape, bool)
    x[seed] = True
    m[1, 3, 51] = True
    x[1, 3, 51] = True
    assert not m[3, 3, 100]
    x[3, 3, 100] = True
    for a in (m, x):
        a.setflags(write=False)
    return m, x


@pytest.mark.parametrize("shape", [(6, 40, 200), (20, 40, 600)])          # one and three tiles of the kernel along z and x
@pytest.mark.parametrize("connectivity", [1, 3])
def test_propagation_along_a_serpentine_corridor(gpu, shape, connectivity):
    m, x = corridor(shape)
    s = ndi.generate_binary_structure(3, connectivity)
    exp = ndi.binary_propagation(x, structure=s, mask=m)
    got, sweeps = run(x, s, R.DILATE, -1, m, return_iterations=True)
    assert np.array_equal(got, exp), "%d voxels differ" % (got != exp).sum()
    assert exp.sum() > 500 and exp[1, 3, 51] and exp[3, 3, 100] and not exp[3, 3, 99] and not exp[1, 3, 50]
    assert sweeps >= 2                                   # the last sweep is the one that changed nothing
    # the module's function, the same result as a mask object
    res = morphology.binary_propagation(x, structure=s, mask=m)
    assert isinstance(res, M.DeviceBooleanMask) and res.shape == shape
    assert np.array_equal(res.include(), exp)


def test_erosion_to_its_fixed_point_takes_the_dual_route(gpu):
    m, x = corridor((6, 40, 200))
    s = ndi.generate_binary_structure(3, 1)
    # the complement of the propagation: eroding ~x under the same mask until nothing changes, border 1
    exp = ndi.binary_erosion(~x, structure=s, iterations=-1, mask=m, border_value=1)
    assert np.array_equal(exp, ~ndi.binary_propagation(x, structure=s, mask=m))
    assert np.array_equal(run(~x, s, R.ERODE, -1, m, 1), exp)
    field = R.field((12, 30, 100), 2, 0.97)
    for border in (0, 1):
        check(field, s, R.ERODE, 0, None, border, what="unmasked erosion to the fixed point, border %d" % border)
        check(~field, np.ones((1, 1, 3), bool), R.DILATE, 0, None, border, what="unmasked dilation to the fixed point")


def test_repeating_a_structure_without_its_centre(gpu):
    x, mask = R.field((9, 12, 70), 5, 0.3), R.field((9, 12, 70), 6, 0.6)
    for s in (np.array([True, False]).reshape(2, 1, 1), R._one_sided((4, 3, 2), 5), R._one_sided((7, 1, 7), 9)):
        for op in (R.ERODE, R.DILATE):
            for m in (None, mask):
                for border in (0, 1):
                    check(x, s, op, -1, m, border, what="one-sided %s op=%d border=%d" % (s.shape, op, border))
    # a structure that cycles (two voxels that swap for ever) ends with an error, not with a hang
    pair = np.zeros((1, 1, 4), bool)
    pair[0, 0, 1] = True
    with pytest.raises(NotImplementedError, match="no fixed point"):
        run(pair, np.array([True, False, True]).reshape(1, 1, 3), R.DILATE, 0)


# ---- views ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rows", "planes_of_rows", "xwin_aligned", "xwin_off1", "xwin_oddstride", "xwin_tail"])
def test_strided_and_offset_views(gpu, name):
    lay = views.layout(name)
    x, mask = R.field(lay.shape, 3, 0.25), R.field(lay.shape, 4, 0.7)
    s = np.ones((3, 3, 7), bool)
    # what lies around a view is 1: an over-read grows into the result of a dilation
    xv, xparent = views.upload(lay, x.astype(np.uint8), 1)
    mv, mparent = views.upload(lay, mask.astype(np.uint8), 1)
    offs = R.offsets(s)
    for op, it, m_dev, m_host, border in ((R.DILATE, 1, None, None, 0), (R.DILATE, 2, mv, mask, 0), (R.ERODE, 1, mv, mask, 1),
                                           (R.DILATE, -1, mv, mask, 0), (R.DILATE, 1, up(mask), mask, 0)):
        got = ops.mask_morph(xv, offs, op, iterations=it, mask=m_dev, border_value=border).get().view(bool)
        assert np.array_equal(got, R.scipy_morph(x, s, op, it, m_host, border)), (name, op, it, border)
        assert np.array_equal(got, run(x, s, op, it, m_host, border))               # = the copied-out arrays
    got = ops.mask_morph(up(x), offs, R.DILATE, mask=mv).get().view(bool)            # a view as the mask alone
    assert np.array_equal(got, R.scipy_morph(x, s, R.DILATE, 1, mask))
    if name in ("rows", "planes_of_rows"):                                          # as DeviceArray.rows() / planes() build them
        parent = DeviceArray.from_numpy(views.place(lay, x.astype(np.uint8), 1).reshape(lay.parent_shape))
        v = parent.rows(views.Y0, views.Y0 + lay.shape[1])
        if name == "planes_of_rows":
            v = v.planes(views.Z0, views.Z0 + lay.shape[0])
        assert (v.ptr, v.row_stride, v.plane_stride) == (xv.ptr - xparent.ptr + parent.ptr, lay.row_stride, lay.plane_stride)
        assert np.array_equal(ops.mask_morph(v, offs, R.DILATE).get().view(bool), R.scipy_morph(x, s, R.DILATE))


def test_aliased_output_is_refused(gpu):
    x = up(R.field((6, 5, 40), 1, 0.3))
    m = up(R.field((6, 5, 40), 2, 0.7))
    offs = R.offsets(R.generate_binary_structure(3, 1))
    before = x.get().copy()
    with pytest.raises(_lib.HipInvalidArgument, match="overlaps d_in"):
        ops.mask_morph(x, offs, R.DILATE, out=x)
    with pytest.raises(_lib.HipInvalidArgument, match="overlaps d_mask"):
        ops.mask_morph(x, offs, R.DILATE, mask=m, out=m)
    big = DeviceArray((7, 5, 40), np.uint8)
    with pytest.raises(_lib.HipInvalidArgument, match="overlaps d_in"):
        ops.mask_morph(big.planes(0, 6), offs, R.DILATE, out=big.planes(1, 7))
    assert np.array_equal(x.get(), before)


# ---- what memory held before the call -------------------------------------------------------------------------------------------
def test_dirty_workspace_and_output(gpu):
    shape = (9, 20, 70)                                                  # 6 voxels and 26 padding bits in a row's last word
    x, mask = R.field(shape, 3, 0.2), R.field(shape, 4, 0.7)
    s = R.generate_binary_structure(3, 2)
    jobs = {"dilate": (x, s, R.DILATE, 2, None, 0), "dilate_b1": (x, s, R.DILATE, 1, None, 1), "erode_mask": (~x, s, R.ERODE, 2, mask, 1),
            "propagate": (x & mask, s, R.DILATE, -1, mask, 0), "erode_fix": (~x, s, R.ERODE, -1, mask, 0),
            "one_sided": (x, R._one_sided((4, 3, 2), 5), R.DILATE, 0, mask, 1)}

    def all_jobs():
        return {k: run(*a) for k, a in jobs.items()}

    def against_scipy(first):
        for k, a in jobs.items():
            assert np.array_equal(first[k], R.scipy_morph(*a)), k
    dirty_memory.same_under_every_pattern(all_jobs, check=against_scipy, patterns=(0xFF, 0x00, "random"))


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def line_cube(dtype):
    shape = (24, 20, 70)
    rng = np.random.default_rng(12)
    z = np.arange(shape[0])[:, None, None]
    amp = 6.0 * np.exp(-0.5 * (((np.arange(shape[1])[:, None] - 9) / 4.0) ** 2 + ((np.arange(shape[2])[None, :] - 35) / 12.0) ** 2))
    d = (rng.normal(size=shape) + amp[None] * np.exp(-0.5 * ((z - 11) / 2.5) ** 2)).astype(dtype)
    d[:, :2] = d[:, -2:] = np.nan
    d[:, :, :3] = d[:, :, -3:] = np.nan
    return d


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_signal_mask_end_to_end(gpu, dtype, monkeypatch):
    d = line_cube(dtype)
    hi, lo = 4.0, 2.0
    cube = SpectralCube.read(d, HDR)
    came_down = []
    original = DeviceArray.get
    monkeypatch.setattr(DeviceArray, "get", lambda self, stream=None: came_down.append(self.nbytes) or original(self, stream))
    core = morphology.binary_opening(cube > hi, structure=np.ones((2, 1, 1), bool))
    sig = morphology.binary_propagation(core, mask=cube > lo)
    masked = cube.with_mask(sig, inherit_mask=False)
    assert came_down == []                               # nothing of the chain came to the host: the change words travel inside the call
    monkeypatch.setattr(DeviceArray, "get", original)
    assert isinstance(sig, M.DeviceBooleanMask) and sig.shape == cube.shape and sig._wcs is not None
    with np.errstate(invalid="ignore"):
        ecore = ndi.binary_opening(d > hi, structure=np.ones((2, 1, 1), bool))
        esig = ndi.binary_propagation(ecore, mask=d > lo)
    assert 200 < esig.sum() < esig.size // 4 and ecore.sum() < esig.sum()
    assert np.array_equal(masked.get_mask_array(), esig)
    assert np.array_equal(core.include(), ecore)
    m0 = np.asarray(masked.moment0())
    e0 = np.asarray(cube.with_mask(esig, inherit_mask=False).moment0())
    assert m0.dtype == e0.dtype and m0.tobytes() == e0.tobytes()
    assert np.isfinite(m0).sum() > 20


def test_cube_conveniences(gpu):
    d = line_cube(np.float32)
    bare = SpectralCube(d, header=HDR)                                   # (read() attaches an isfinite mask; this has none)
    assert bare.mask is None and bare.with_mask_dilated().get_mask_array().all()           # all True, and it stays so
    assert bare.with_mask_eroded(iterations=2).get_mask_array().sum() == 20 * 16 * 66      # two voxels off every face
    cube = SpectralCube.read(d, HDR)
    assert np.array_equal(cube.with_mask_dilated().get_mask_array(), ndi.binary_dilation(np.isfinite(d)))
    with np.errstate(invalid="ignore"):
        inc = d > 2.0
    bright = cube.with_mask(cube > 2.0)
    s = np.ones((3, 3), bool)                                            # 2-D: per plane
    assert np.array_equal(bright.with_mask_dilated(s, iterations=2).get_mask_array(),
                          ndi.binary_dilation(inc, structure=s[None], iterations=2))
    assert np.array_equal(bright.with_mask_eroded().get_mask_array(), ndi.binary_erosion(inc))
    # every kind of input and mask, one result
    exp = ndi.binary_dilation(inc, mask=np.isfinite(d))
    fin = M.LazyMask(np.isfinite, cube=cube)
    for inp, kw in ((bright, dict(mask=fin)), (cube > 2.0, dict(mask=np.isfinite(d))), (inc, dict(mask=fin, cube=cube)),
                    (M.DeviceBooleanMask(up(inc)), dict(mask=cube.with_mask(fin))),
                    (M.FunctionMask(lambda a: a > 2.0), dict(mask=M.DeviceBooleanMask(up(np.isfinite(d))), cube=cube))):
        assert np.array_equal(morphology.binary_dilation(inp, **kw).include(), exp)
    rms = np.full(d.shape[1:], 2.0, np.float32)                          # a map threshold: the mask is compiled and evaluated
    rms[5] = 3.0                                                         # on the device, morphology takes its array
    with np.errstate(invalid="ignore"):
        assert np.array_equal(morphology.binary_dilation(cube > rms).include(), ndi.binary_dilation(d > rms))
    assert np.array_equal(morphology.binary_closing(inc, iterations=2, border_value=1).include(),
                          ndi.binary_closing(inc, iterations=2, border_value=1))
