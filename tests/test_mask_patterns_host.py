"""CPU companion of test_gpu_mask_patterns.py: the matrix there can see what it is for.  A numpy restatement of a masked
count / sum / min / max / median over rays and of a 3-tap stencil along x reads the uint8 include array the way a kernel
does; from it come the neighbouring wrong readings (WRONG).  The right restatement passes every (pattern, bytes, poison) cell
of the three checks that the GPU matrix applies - canonical bytes against a reference, every byte variant bit for bit against
the canonical run, the poisoned cube bit for bit against the zeroed one - and every wrong reading fails at least one cell.
The pattern properties of mask_patterns.properties hold for every shape the matrix uses.  numpy only; no GPU."""
import numpy as np
import pytest

import mask_patterns as P
import views as V

WRONG = ("bit 0 decides", "signed byte > 0", "byte == 1", "byte as weight and count", "popcount of the dword is the count",
         "byte lanes reversed", "excluded sample times zero", "an empty 16-byte group skips the next one", "excluded samples enter min / max")
TAPS = np.array([0.25, 0.5, 0.25])
SHAPE = V.BASE


def _decode(mb, wrong):
    """the include set a kernel makes of the bytes *mb*"""
    if wrong == "bit 0 decides":
        return (mb & 1) != 0
    if wrong == "signed byte > 0":
        return mb.view(np.int8) > 0
    if wrong == "byte == 1":
        return mb == 1
    inc = mb != 0
    if wrong == "byte lanes reversed":
        nz, ny, nx = mb.shape
        return inc.reshape(nz, ny, nx // 4, 4)[..., ::-1].reshape(mb.shape)
    if wrong == "an empty 16-byte group skips the next one":
        flat = inc.reshape(-1).copy()
        n = flat.size // 16 * 16
        g = flat[:n].reshape(-1, 16)
        skip = np.zeros(g.shape[0], bool)
        skip[1:] = ~g[:-1].any(axis=1)
        g[skip] = False
        return flat.reshape(mb.shape)
    return inc


def restate(d, mb, wrong=None):
    """{count, sum, min, max, median over axis 0; stencil}: the masked operators as a kernel computes them from the cube *d* and
    the include bytes *mb*; *wrong*: one of WRONG"""
    inc = _decode(mb, wrong)
    valid = inc & ~np.isnan(d)
    with np.errstate(all="ignore"):
        sel = np.where(valid, d, 0).astype(np.float64)
        if wrong == "excluded sample times zero":          # NaN * 0 and inf * 0 are NaN
            sel = np.where(inc, sel, d.astype(np.float64) * 0.0)
        weight = valid.astype(np.float64)
        if wrong == "byte as weight and count":
            weight = np.where(valid, mb, 0).astype(np.float64)
        count = weight.sum(axis=0)
        if wrong == "popcount of the dword is the count":
            count = np.where(valid, np.unpackbits(mb[..., None], axis=-1).sum(axis=-1), 0).sum(axis=0).astype(np.float64)
        some = valid.any(axis=0)
        total = np.where(some, (sel * weight if wrong == "byte as weight and count" else sel).sum(axis=0), np.nan)
        lo_src = hi_src = valid
        if wrong == "excluded samples enter min / max":
            lo_src = hi_src = ~np.isnan(d)
        vmin = np.where(some, np.min(np.where(lo_src, d, np.inf), axis=0), np.nan)
        vmax = np.where(some, np.max(np.where(hi_src, d, -np.inf), axis=0), np.nan)
        f = np.where(valid, d, np.nan).astype(np.float64)
        median = np.full(d.shape[1:], np.nan)
        median[some] = np.nanmedian(f[:, some], axis=0)
        num, den = np.zeros(d.shape), np.zeros(d.shape)
        for k, w in zip((-1, 0, 1), TAPS):                 # normalised masked stencil along x, zero outside the row
            s, v = np.zeros(d.shape), np.zeros(d.shape)
            src = slice(max(0, k), d.shape[2] + min(0, k))
            dst = slice(max(0, -k), d.shape[2] + min(0, -k))
            s[..., dst], v[..., dst] = sel[..., src], valid[..., src]
            num += w * s
            den += w * v
        stencil = np.where(den > 0, num / den, np.nan)
    return {"count": count, "sum": total, "min": vmin, "max": vmax, "median": median, "stencil": stencil}


def reference(d, inc):
    """the same outputs straight from the include set, no bytes involved"""
    f = np.where(inc, d, np.nan).astype(np.float64)
    some = ~np.isnan(f).all(axis=0)
    with np.errstate(all="ignore"):
        out = {"count": (~np.isnan(f)).sum(axis=0).astype(np.float64), "sum": np.where(some, np.nansum(f, axis=0), np.nan)}
        out["min"], out["max"], out["median"] = (np.full(some.shape, np.nan) for _ in range(3))
        out["min"][some], out["max"][some] = np.nanmin(f[:, some], axis=0), np.nanmax(f[:, some], axis=0)
        out["median"][some] = np.nanmedian(f[:, some], axis=0)
        pad = np.pad(f, ((0, 0), (0, 0), (1, 1)), constant_values=np.nan)
        win = np.stack([pad[..., k:k + f.shape[2]] for k in range(3)])
        w = TAPS[:, None, None, None] * ~np.isnan(win)
        den = w.sum(axis=0)
        out["stencil"] = np.where(den > 0, (w * np.nan_to_num(win)).sum(axis=0) / den, np.nan)
    return out


def _bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def _close(got, exp):
    for k, e in exp.items():
        g = got[k]
        if not np.array_equal(np.isnan(g), np.isnan(e)) or not np.array_equal(np.isinf(g), np.isinf(e)):
            return False
        fin = np.isfinite(e)
        if not np.allclose(g[fin], e[fin], rtol=1e-12, atol=1e-12):
            return False
    return True


def failing_cells(wrong):
    """the (pattern, bytes, check) cells of the GPU matrix's three checks that the reading *wrong* misses"""
    data = V.data(np.float32, SHAPE)[0]
    failed = []
    for pattern in P.PATTERNS:
        inc = P.include(pattern, SHAPE)
        canon = restate(data, P.to_bytes(inc, "canonical"), wrong)
        if not _close(canon, reference(data, inc)):                                      # (a)
            failed.append((pattern, "canonical", "reference"))
        bad, zero = P.poison(data, inc)
        for kind in P.BYTES:
            mb = P.to_bytes(inc, kind)
            if kind != "canonical" and not _bits(restate(data, mb, wrong), canon):          # (b)
                failed.append((pattern, kind, "bytes"))
            if pattern != "all one" and kind in ("canonical", "mixed") and not _bits(restate(bad, mb, wrong), restate(zero, mb, wrong)):
                failed.append((pattern, kind, "poison"))                                 # (c)
    return failed


def test_the_right_restatement_passes_every_cell():
    assert failing_cells(None) == []


@pytest.mark.parametrize("wrong", WRONG)
def test_a_wrong_reading_of_the_mask_fails_some_cell(wrong):
    failed = failing_cells(wrong)
    print("%s: %d cells fail, first %s" % (wrong, len(failed), failed[:4]))
    assert failed, "a kernel that reads the mask this way would pass the matrix"


def test_each_wrong_reading_needs_what_the_matrix_adds():
    """on the canonical bytes of the 70 % random mask of views.data, clean samples under the excluded voxels, the readings that
    differ only in the byte value are invisible: that is the gap"""
    data, m = V.data(np.float32, SHAPE)
    ref = reference(data, m.astype(bool))
    for wrong in WRONG[:5]:
        assert _close(restate(data, m, wrong), ref), wrong


@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pattern_properties(shape):
    for name in P.PATTERNS:
        p = P.properties(name, shape)
        inc = P.include(name, shape)
        assert inc.shape == tuple(shape) and inc.dtype == bool and not inc.flags.writeable
        assert p["included"] + p["excluded"] == inc.size
        for unit in p["claims"]:
            assert p["empty"][unit] > 0, (name, unit, "claims an empty one")
            assert p["occupied"][unit] > 0, (name, unit, "claims one that is not empty")
        assert (p["poisoned"] > 0) == (p["excluded"] > 0), name
        assert P.poison_set(inc)[inc].sum() == 0
    assert P.properties("all zero", shape)["included"] == 0 and P.properties("all one", shape)["excluded"] == 0
    one = P.include("one voxel", shape)
    assert one.sum() == 1 and one[-1, -1, -1]
    lanes = P.properties("lanes", shape)
    assert lanes["lanes"] == {0, 1, 2, 3} and lanes["empty"]["dword"] == 0
    assert (P.include("lanes", shape).reshape(-1, 4).sum(axis=1) == 1).all()
    seg = P.include("segments", shape)
    z, x = np.arange(shape[0])[:, None, None], np.arange(shape[2])[None, None, :]
    assert not seg[np.broadcast_to((x // 32 + z) % 2 == 1, shape)].any() and 0.25 < seg[np.broadcast_to((x // 32 + z) % 2 == 0, shape)].mean() < 0.35
    slabs = P.properties("slabs", shape)
    assert slabs["last_plane_only"] > 0, "slabs: rays whose only samples lie in the last plane"
    assert 0.02 < P.include("sparse", shape).mean() < 0.06


def test_bytes_and_poison():
    inc = P.include("sparse", SHAPE)
    for kind, values in (("canonical", {1}), ("two", {2}), ("sign", {0x80}), ("ones", {0xFF}), ("mixed", set(P.MIXED_VALUES))):
        mb = P.to_bytes(inc, kind)
        assert mb.dtype == np.uint8 and np.array_equal(mb != 0, inc) and set(np.unique(mb[inc]).tolist()) == values, kind
    for dtype in (np.float32, np.float64):
        d = V.data(dtype, SHAPE)[0]
        bad, zero = P.poison(d, inc)
        pick = P.poison_set(inc)
        assert bad.dtype == dtype and np.array_equal(bad[~pick], d[~pick], equal_nan=True) and not zero[pick].any()
        u = np.uint32 if dtype == np.float32 else np.uint64
        assert set(np.unique(bad[pick].view(u)).tolist()) == set(P.poison_values(dtype).view(u).tolist())
        assert 0.2 < pick.sum() / (~inc).sum() < 0.3 and not pick[inc].any()
