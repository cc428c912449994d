"""GPU: connected-component labelling (csrc/spc_label.hip through ops.label / label_objects / label_select and
spectral_cube_amd.labelling) against scipy.ndimage.label, np.bincount and scipy.ndimage.find_objects.  Integers and
booleans have no tolerance: every result is np.array_equal to scipy's, the numbering of the components included."""
import functools

import numpy as np
import pytest
import scipy.ndimage as ndi

import dirty_memory
import labelling as R
import views
from spectral_cube_amd import _lib, labelling, morphology, ops, SpectralCube
from spectral_cube_amd import masks as M
from spectral_cube_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CDELT1": -1e-3, "CDELT2": 1e-3, "CDELT3": 0.5,
       "CUNIT3": "km/s", "CRPIX1": 4, "CRPIX2": 3, "CRPIX3": 1, "CRVAL1": 10.0, "CRVAL2": 20.0, "CRVAL3": -16.0, "BUNIT": "K"}
CONN = {c: ndi.generate_binary_structure(3, c) for c in (1, 2, 3)}


def up(a):
    return DeviceArray.from_numpy(np.asarray(a, dtype=bool).astype(np.uint8))


def check(x, structure=None, what="", objects=True):
    """label(x) through the public function against scipy: labels, n, and (objects) sizes and find_objects"""
    exp, n = R.scipy_label(x, structure)
    lab, got_n = labelling.label(x, structure=structure)
    got = lab.get()
    assert got.dtype == np.int32 and got.shape == exp.shape
    assert got_n == lab.n == n, "%s: %d labels, scipy has %d" % (what, got_n, n)
    assert np.array_equal(got, exp), "%s: %d voxels differ, first %s" % (what, (got != exp).sum(), np.argwhere(got != exp)[:4].tolist())
    if objects:
        sizes, objs = R.scipy_objects(exp, n)
        s = lab.sizes()
        assert s.dtype == np.int64 and np.array_equal(s, sizes), what
        assert lab.find_objects() == objs, what
        assert s is lab.sizes()                                          # one label_objects call, kept
    return lab, exp, n


# ---- the case table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in R.structures()])
def test_case_table(gpu, name):
    n = 0
    for cid, x, s in R.cases():
        if cid.split("-")[0] == name:
            check(x, s, what=cid)
            n += 1
    assert n == len(R.SHAPES) * len(R.DENSITIES)


def test_a_plane_structure_labels_every_plane_on_its_own(gpu):
    x = R.field((5, 17, 33), 4, 0.45)
    s2 = ndi.generate_binary_structure(2, 1)
    lab, n = labelling.label(x, structure=s2)
    got = lab.get()
    base = 0
    for k in range(x.shape[0]):                                           # scipy, plane by plane, numbered on
        e, m = ndi.label(x[k], structure=s2)
        assert np.array_equal(got[k], np.where(e > 0, e + base, 0))
        base += m
    assert n == base
    assert np.array_equal(got, R.scipy_label(x, s2)[0])                   # = the middle plane of a 3x3x3 structure


# ---- row lengths around a wave's 64 voxels ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [1, 31, 32, 33, 63, 64, 65, 100, 130, 255, 256, 257])
def test_row_lengths(gpu, nx):
    shape = (3, 4, nx)
    for seed, p in enumerate((0.3, 0.7)):
        x = R.field(shape, nx + seed, p)
        x[:, :, -1] = True                                                # a row's tail must not join the next row's head
        x[:, ::2, 0] = True
        for s in (CONN[1], CONN[3], R._only((0, 0, 1)), R._only((0, 1, 1), (0, 0, 1)), R._only((1, 1, -1))):
            check(x, s, what="nx=%d p=%g" % (nx, p))
    ones = np.ones(shape, bool)
    lab, exp, n = check(ones, R._only((0, 0, 1)), what="rows nx=%d" % nx)  # every row one component of its own
    assert n == 12 and lab.sizes()[1:].tolist() == [nx] * 12


# ---- one component that every part of the array has to agree on ---------------------------------------------------------------
@pytest.mark.parametrize("shape", [(6, 40, 200), (20, 40, 600)])
@pytest.mark.parametrize("connectivity", [1, 3])
def test_serpentine(gpu, shape, connectivity):
    m, seed = R.serpentine(shape)
    m[1, 3, 51] = True                                                    # an island next to the corridor
    lab, exp, n = check(m, CONN[connectivity], what="serpentine %s" % (shape,))
    assert n == 2 and lab.sizes()[1] > 500 and lab.sizes()[2] == 1


def test_nested_shells(gpu):
    x = R.shells(40)
    for c in (1, 3):
        lab, exp, n = check(x, CONN[c], what="shells conn%d" % c)
        assert n == 40
        assert [o[0].start for o in lab.find_objects()] == list(range(0, 80, 2))       # outermost first: raster order


# ---- degenerate fields ---------------------------------------------------------------------------------------------------------
def test_all_false_and_all_true(gpu):
    for shape in ((5, 6, 7), (1, 1, 1), (3, 17, 130)):
        lab, exp, n = check(np.zeros(shape, bool), what="all False")
        assert n == 0 and not lab.get().any() and lab.sizes().tolist() == [int(np.prod(shape))] and lab.find_objects() == []
        for s in (CONN[1], CONN[3]):
            lab, exp, n = check(np.ones(shape, bool), s, what="all True")
            assert n == 1 and lab.sizes().tolist() == [0, int(np.prod(shape))]
        lab, exp, n = check(np.ones(shape, bool), np.zeros((3, 3, 3), bool), what="all True, no pair")
        assert n == int(np.prod(shape))


@functools.lru_cache(maxsize=None)
def board():
    x = R.checkerboard((64, 256, 256))
    x.setflags(write=False)
    return x


def test_checkerboard_two_million_labels(gpu):
    x = board()
    lab, n = labelling.label(x, structure=CONN[1])
    assert n == 2097152 == x.sum()
    exp = np.zeros(x.shape, np.int32)
    exp[x] = np.arange(1, n + 1, dtype=np.int32)                          # every True voxel its own label, in raster order
    assert np.array_equal(lab.get(), exp)
    assert np.array_equal(lab.sizes(), np.r_[x.size - n, np.ones(n, np.int64)])
    bbox = lab.bounding_boxes()
    zyx = np.argwhere(x).astype(np.int32)
    assert np.array_equal(bbox[1:, 0::2], zyx) and np.array_equal(bbox[1:, 1::2], zyx + 1)
    one, n3 = labelling.label(x, structure=CONN[3])
    assert n3 == 1 and np.array_equal(one.get(), x.astype(np.int32))


@pytest.mark.parametrize("p,connectivity", [(0.5, 3), (0.31, 1)])
def test_mid_size_field(gpu, p, connectivity):
    x = R.field((64, 256, 256), 17, p)
    lab, exp, n = check(x, CONN[connectivity], what="p=%g conn%d" % (p, connectivity))
    sizes = lab.sizes()
    assert n > 1 and sizes[1:].min() == 1
    if connectivity == 3:
        assert sizes[1:].max() > x.sum() // 2                             # the percolating giant and a few single voxels
    else:
        assert n > 100000 and 1000 < sizes[1:].max() < x.sum() // 10      # near the threshold: every size up to thousands


@pytest.mark.parametrize("shape", [(70000, 2, 3), (2, 70000, 3), (2, 3, 70000)])
def test_one_long_axis(gpu, shape):
    x = R.field(shape, 1, 0.4)
    for c in (1, 3):
        check(x, CONN[c], what="%s conn%d" % (shape, c))


# ---- past the first round of every kernel ------------------------------------------------------------------------------------------
# Grids are capped at 65536 blocks of 256 voxels (lb_objects: 2048 blocks of 4096), so only beyond 2^24 = 16.8M voxels do the
# grid-stride loops of init / merge / relabel come round again and do flatten / number walk a chunk of two rounds with the
# running count carried on; lb_objects carries its open run into a wave's next round beyond 2^23 = 8.4M.
@pytest.mark.parametrize("shape", [(130, 256, 256), (260, 256, 256)])
def test_beyond_the_grid_caps(gpu, shape):
    nz = shape[0]
    x = R.field(shape, 23, 0.004)                                         # single voxels and pairs everywhere: roots in every chunk
    x[:, 0, 0] = x[-1, :, 0] = x[-1, -1, :] = True                        # one component from the first voxel to the last
    x[nz // 2 - 3:nz // 2 + 3, 40:200, 30:230] = True                     # two blocks: between them they lie across plane 128 of
    x[nz - 8:nz - 1, 100:180, 5:250] = True                               # either shape (voxel 2^23) and plane 256 of the larger (2^24)
    x[3:9, 60:90, 100:140] = R.field((6, 30, 40), 24, 0.55)               # a ragged cluster in the first round
    assert (x.size > 2 ** 24) == (nz == 260) and x.size > 2 ** 23
    for c in (1, 3):
        lab, exp, n = check(x, CONN[c], what="%s conn%d" % (shape, c))
        assert n > 10000 and exp[0, 0, 0] == 1 == exp[-1, -1, -1]
    keep = np.random.default_rng(5).random(n + 1) < 0.5                   # n + 1 > 32768: the table is read from memory
    assert np.array_equal(lab.select(keep).include(), keep[exp])


# ---- views, other bytes, aliasing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rows", "planes_of_rows", "xwin_aligned", "xwin_off1", "xwin_oddstride", "xwin_tail"])
def test_strided_and_offset_views(gpu, name):
    lay = views.layout(name)
    x = R.field(lay.shape, 3, 0.25)
    x[:, :, 0] |= R.field(lay.shape[:2], 4, 0.5)                          # voxels on the faces next to the 1s around the view:
    x[:, :, -1] |= R.field(lay.shape[:2], 5, 0.5)                         # an over-read joins their components
    xv, parent = views.upload(lay, x.astype(np.uint8), 1)
    for c in (1, 3):
        exp, n = R.scipy_label(x, CONN[c])
        got, m = ops.label(xv, CONN[c])
        assert m == n and np.array_equal(got.get(), exp), (name, c)
    assert np.array_equal(parent.get(), views.place(lay, x.astype(np.uint8), 1))       # the input is only read


def test_any_non_zero_byte_is_true(gpu):
    x = R.field((9, 8, 70), 2, 0.4)
    exp, n = R.scipy_label(x, CONN[2])
    for byte in (2, 127, 255):
        raw = np.where(x, byte, 0).astype(np.uint8)
        raw[x & R.field(x.shape, 3, 0.3)] = 1                              # mixed with 1s
        got, m = ops.label(DeviceArray.from_numpy(raw), CONN[2])
        assert m == n and np.array_equal(got.get(), exp), byte


def test_aliased_output_is_refused(gpu):
    x = R.field((6, 5, 40), 1, 0.3)
    host = np.zeros((4 * 6 + 6, 5, 40), np.uint8)
    host[:6] = x
    big = DeviceArray.from_numpy(host)
    inp = big.planes(0, 6)
    out = DeviceArray(x.shape, np.int32, 0, ptr=big.ptr, owner=big)       # the labels over the input's own bytes
    before = big.get().copy()
    with pytest.raises(_lib.HipInvalidArgument, match="overlaps d_in"):
        ops.label(inp, CONN[1], out=out)
    assert np.array_equal(big.get(), before)
    lab, n = ops.label(inp, CONN[1])
    with pytest.raises(_lib.HipInvalidArgument, match="overlaps d_labels"):
        ops.label_select(lab, n, np.ones(n + 1, bool), out=DeviceArray(x.shape, np.uint8, 0, ptr=lab.ptr + 7, owner=lab))
    assert np.array_equal(lab.get(), R.scipy_label(x)[0])


# ---- what memory held before the call -----------------------------------------------------------------------------------------
def test_dirty_workspace_outputs_and_tables(gpu):
    x = R.field((9, 20, 70), 3, 0.35)
    keep_rng = np.random.default_rng(8)
    jobs = {"conn1": CONN[1], "conn3": CONN[3], "none": np.zeros((3, 3, 3), bool), "random": R.random_structure(2)}
    keeps = {k: keep_rng.random(R.scipy_label(x, s)[1] + 1) < 0.5 for k, s in jobs.items()}

    def all_jobs():
        out = {}
        for k, s in jobs.items():
            lab, n = ops.label(up(x), s)
            sizes, bbox = ops.label_objects(lab, n)
            sel = ops.label_select(lab, n, keeps[k])
            out[k + "_labels"], out[k + "_n"], out[k + "_sizes"] = lab.get(), np.int64(n), sizes.get()
            out[k + "_bbox"], out[k + "_select"] = bbox.get()[1:], sel.get()
        return out

    def against_scipy(first):
        for k, s in jobs.items():
            exp, n = R.scipy_label(x, s)
            sizes, objs = R.scipy_objects(exp, n)
            assert first[k + "_n"] == n and np.array_equal(first[k + "_labels"], exp) and np.array_equal(first[k + "_sizes"], sizes), k
            assert first[k + "_bbox"].tolist() == [[v for sl in o for v in (sl.start, sl.stop)] for o in objs], k
            assert np.array_equal(first[k + "_select"].view(bool), keeps[k][exp]), k
    dirty_memory.same_under_every_pattern(all_jobs, check=against_scipy, patterns=(0xFF, 0x00, "random"))


# ---- label_objects and label_select on their own ----------------------------------------------------------------------------------
def test_label_objects_refuses_a_label_outside_the_tables(gpu):
    shape = (5, 6, 70)
    lab = np.random.default_rng(4).integers(0, 10, size=shape).astype(np.int32)
    n = 9
    guard = 64                                                            # table entries of 0x5A bytes on either side
    for bad in (10, -1, 2 ** 31 - 1, -2 ** 31, 12345):
        l2 = lab.copy()
        l2[2, 3, 40] = bad
        l2[4, 5, 69] = bad
        sbuf = DeviceArray.from_numpy(np.full(n + 1 + 2 * guard, 0x5A5A5A5A5A5A5A5A, np.int64))
        bbuf = DeviceArray.from_numpy(np.full((n + 1 + 2 * guard) * 6, 0x5A5A5A5A, np.int32))
        sizes = DeviceArray((n + 1,), np.int64, 0, ptr=sbuf.ptr + 8 * guard, owner=sbuf)
        bbox = DeviceArray((n + 1, 6), np.int32, 0, ptr=bbuf.ptr + 24 * guard, owner=bbuf)
        with pytest.raises(_lib.HipInvalidArgument, match="outside 0"):
            ops.label_objects(DeviceArray.from_numpy(l2), n, out={"sizes": sizes, "bbox": bbox})
        s, b = sbuf.get(), bbuf.get()
        assert (s[:guard] == 0x5A5A5A5A5A5A5A5A).all() and (s[-guard:] == 0x5A5A5A5A5A5A5A5A).all(), bad
        assert (b[:6 * guard] == 0x5A5A5A5A).all() and (b[-6 * guard:] == 0x5A5A5A5A).all(), bad
        ok = (l2 >= 0) & (l2 <= n)                                        # the voxels in range were counted, the others skipped
        assert np.array_equal(s[guard:-guard], np.bincount(l2[ok], minlength=n + 1))
    sizes, bbox = ops.label_objects(DeviceArray.from_numpy(lab), n)      # in range: no error, and labels need not be components
    assert np.array_equal(sizes.get(), np.bincount(lab.ravel(), minlength=n + 1))
    assert [tuple(slice(int(r[2 * a]), int(r[2 * a + 1])) for a in range(3)) for r in bbox.get()[1:]] == ndi.find_objects(lab, max_label=n)
    # a label without a voxel: size 0 and None, as in scipy
    lm = labelling.LabelMap(DeviceArray.from_numpy(np.where(lab == 4, 0, lab)), n)
    assert lm.sizes()[4] == 0 and lm.find_objects() == ndi.find_objects(np.where(lab == 4, 0, lab), max_label=n) and lm.find_objects()[3] is None


@pytest.mark.parametrize("case", ["small", "table beyond LDS"])
def test_select(gpu, case):
    if case == "small":
        x, s = R.field((9, 8, 70), 6, 0.3), CONN[1]
    else:
        x, s = board()[:8], CONN[1]                                       # 262144 labels: the table is read from memory
    lab, n = labelling.label(x, structure=s)
    exp = R.scipy_label(x, s)[0]
    assert (n + 1 > 32768) == (case != "small")
    keep = np.random.default_rng(2).random(n + 1) < 0.5
    keep[0] = False
    got = lab.select(keep)
    assert isinstance(got, M.DeviceBooleanMask) and got.shape == x.shape
    raw = got.device_array().get()
    assert raw.dtype == np.uint8 and raw.max() <= 1 and np.array_equal(raw.view(bool), keep[exp])
    assert not lab.select([]).include().any()
    assert np.array_equal(lab.select(np.r_[False, np.ones(n, bool)]).include(), x)
    assert np.array_equal(lab.select(np.ones(n + 1, bool)).include(), np.ones(x.shape, bool))          # entry 0: the background
    numbers = [1, n, max(1, n // 2)]
    assert np.array_equal(lab.select(numbers).include(), np.isin(exp, numbers))
    two = ops.label_select(lab.device_array(), n, (keep * 7).astype(np.uint8)).get()                    # any non-zero entry keeps
    assert np.array_equal(two, raw)
    with pytest.raises(ValueError):
        lab.select([n + 1])
    with pytest.raises(ValueError):
        lab.select(np.ones(n, bool))
    with pytest.raises(TypeError, match="uint8"):                          # table or numbers? only a bool array is a table
        lab.select(np.ones(n + 1, np.uint8))


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pruned_signal_mask_end_to_end(gpu, dtype, monkeypatch):
    d = R.line_cube(dtype)
    hi, lo, min_size = 4.0, 2.0, 3
    s3 = CONN[3]                                                          # grown over corners; labelled over faces, which splits
    cube = SpectralCube.read(d, HDR)
    with np.errstate(invalid="ignore"):
        ecore = ndi.binary_opening(d > hi, structure=np.ones((2, 1, 1), bool))
        esig = ndi.binary_propagation(ecore, structure=s3, mask=d > lo)
    epruned, ekeep = R.scipy_remove_small(esig, min_size, None, 2)
    assert ekeep[1:].any() and not ekeep[1:].all()                        # scipy alone removes a component and keeps one
    assert 0 < epruned.sum() < esig.sum()
    assert R.scipy_remove_small(esig, min_size, None, 1)[1].sum() > ekeep.sum()          # min_channels removes some of its own
    n = len(ekeep) - 1

    came_down = []
    original = DeviceArray.get
    monkeypatch.setattr(DeviceArray, "get", lambda self, stream=None: came_down.append(self.nbytes) or original(self, stream))
    core = morphology.binary_opening(cube > hi, structure=np.ones((2, 1, 1), bool))
    sig = morphology.binary_propagation(core, structure=s3, mask=cube > lo)
    pruned = labelling.remove_small_objects(sig, min_size=min_size, min_channels=2)
    masked = cube.with_mask(pruned, inherit_mask=False)
    again = cube.with_mask(sig, inherit_mask=False).with_mask_pruned(min_size=min_size, min_channels=2)
    # two runs, each brought down its two tables and nothing else: 8 and 24 bytes per label, never a cube-sized array
    # (the smallest of those is the uint8 mask, one byte per voxel)
    assert sorted(came_down) == sorted(2 * [8 * (n + 1), 24 * (n + 1)]) and max(came_down) < d.size
    monkeypatch.setattr(DeviceArray, "get", original)

    assert isinstance(pruned, M.DeviceBooleanMask) and pruned.shape == cube.shape and pruned._wcs is not None
    assert np.array_equal(pruned.include(), epruned)
    assert np.array_equal(masked.get_mask_array(), epruned) and np.array_equal(again.get_mask_array(), epruned)
    m0 = np.asarray(masked.moment0())
    e0 = np.asarray(cube.with_mask(epruned, inherit_mask=False).moment0())
    assert m0.dtype == e0.dtype and m0.tobytes() == e0.tobytes()
    assert np.asarray(again.moment0()).tobytes() == e0.tobytes()
    assert np.isfinite(m0).sum() > 20
    # the README's last step: the largest component alone
    lab, nl = labelling.label(sig)
    assert nl == n
    largest = lab.select([lab.sizes()[1:].argmax() + 1])
    elab = R.scipy_label(esig)[0]
    assert np.array_equal(largest.include(), elab == np.bincount(elab.ravel())[1:].argmax() + 1)


def test_every_kind_of_input(gpu):
    d = R.line_cube(np.float32)
    cube = SpectralCube.read(d, HDR)
    with np.errstate(invalid="ignore"):
        inc = d > 2.0
    exp, n = R.scipy_label(inc, CONN[2])
    bright = cube.with_mask(cube > 2.0)
    for inp, kw in ((bright, {}), (cube > 2.0, {}), (inc, {}), (M.DeviceBooleanMask(up(inc)), {}),
                    (M.FunctionMask(lambda a: a > 2.0), dict(cube=cube))):
        lab, m = labelling.label(inp, structure=CONN[2], **kw)
        assert m == n and np.array_equal(lab.get(), exp)
    assert labelling.label(bright)[0].wcs is not None and lab.shape == d.shape
    assert np.array_equal(bright.with_mask_pruned(min_size=5, structure=CONN[2]).get_mask_array(),
                          R.scipy_remove_small(inc, 5, CONN[2])[0])
