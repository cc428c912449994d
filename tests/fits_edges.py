"""What test_fits_decode_host.py and test_gpu_fits.py share: the fixture tests/golden/fits_decode_edges.npz (written by
oracle/gen_golden.py::case_fits_decode_edges from files astropy wrote and read), the bit-for-bit comparison, generated
payloads that carry the fixture's edge vectors, and a numpy model of the decode that can be run with one defect at a time."""
import json
from fractions import Fraction

import numpy as np

from conftest import golden

_RAW = {8: "u1", 16: "i2", 32: "i4", 64: "i8", -32: "f4", -64: "f8"}
BYTES = {b: np.dtype(t).itemsize for b, t in _RAW.items()}
WIDE = (-64, 32, 64)                       # the sample types spc_fits_to_f64 takes
SENTINEL = -777.25                         # what output buffers hold before a decode


class Fixture:
    """the files of fits_decode_edges.npz: .names, .meta[name] (bitpix, bscale, bzero, blank, astropy_deviates, data_offset),
    .file(name) bytes, .payload(name) bytes, .expected(name, dtype), .vector(bitpix)"""

    shape = (3, 5, 7)

    def __init__(self):
        self.g = golden("fits_decode_edges.npz")
        self.meta = json.loads(str(self.g["meta"]))
        self.names = sorted(self.meta)
        self.start = int(self.g["start"])

    def file(self, name):
        return self.g[name + "_file"].tobytes()

    def payload(self, name):
        m = self.meta[name]
        off = m["data_offset"]
        return self.file(name)[off:off + 105 * BYTES[m["bitpix"]]]

    def expected(self, name, dtype=np.float32):
        return self.g[name + ("_f32" if np.dtype(dtype) == np.float32 else "_f64")]

    def vector(self, bitpix):
        return self.g["vector_%s%d" % ("b" if bitpix > 0 else "f", abs(bitpix))]

    def args(self, name):
        """(bitpix, bscale, bzero, blank or None) as the decoders take them"""
        m = self.meta[name]
        return m["bitpix"], float(m["bscale"]), float(m["bzero"]), m["blank"]


_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = Fixture()
    return _fixture


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def exact_nan(bitpix, bscale, bzero):
    """NaNs that only were moved (an unscaled float image) keep their bits; NaNs out of arithmetic or BLANK are just NaNs"""
    return bitpix < 0 and bscale == 1.0 and bzero == 0.0


def mismatch(got, exp, nan_bits):
    """boolean array: where *got* is not *exp* bit for bit (signs of zero, denormals, infinities; NaN payloads if nan_bits)"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    bad = bits(got) != bits(exp)
    if not nan_bits:
        bad &= ~(np.isnan(got) & np.isnan(exp))
    return bad


def assert_same(got, exp, nan_bits, what):
    bad = mismatch(got, exp, nan_bits)
    if bad.any():
        at = np.flatnonzero(bad.ravel())
        raise AssertionError("%s: %d of %d samples differ, first at %s: got %s (%s), expected %s (%s)" % (
            what, at.size, bad.size, at[:6].tolist(), got.ravel()[at[:6]], [hex(int(b)) for b in bits(got).ravel()[at[:6]]],
            exp.ravel()[at[:6]], [hex(int(b)) for b in bits(exp).ravel()[at[:6]]]))


def to_payload(raw):
    """big-endian bytes of native samples, moved as integers (no float passes through a register)"""
    raw = np.ascontiguousarray(raw)
    if raw.dtype.itemsize == 1:
        return raw.tobytes()
    return raw.view("u%d" % raw.dtype.itemsize).byteswap().tobytes()


def generated(bitpix, n, seed=0):
    """n native raw samples: random ones over the type's whole range (floats: standard normal) with the fixture's edge vector
    laid over them every len + 5 samples from sample 1 on (every phase of a 4-sample group), cut off at the end"""
    rng = np.random.default_rng([abs(bitpix), n, seed])
    dt = np.dtype(_RAW[bitpix])
    if bitpix > 0:
        info = np.iinfo(dt)
        raw = rng.integers(info.min, info.max, size=n, dtype=dt, endpoint=True)
    else:
        raw = rng.standard_normal(n).astype(dt)
    vec = fixture().vector(bitpix)
    for p in range(1 if n > 1 else 0, n, vec.size + 5):
        m = min(vec.size, n - p)
        raw[p:p + m] = vec[:m]                     # (same type: the bits are copied, NaN payloads included)
    return raw


# ---- a numpy model of the decode, and what it gives with one defect ------------------------------------------------
DEFECTS = (
    "no swap", "swap at the wrong width", "int16 without sign extension", "uint8 read as signed", "8/16 scaled in float64",
    "32/64 scaled in float32", "-64 scaled in float32", "multiply-add fused into one rounding", "BLANK compared after scaling",
    "BLANK compared unsigned", "BLANK applied to float images", "int64 narrowed in one rounding",
    "last n % 4 samples skipped", "NaN payload canonicalised",
    "identity add applied (x + 0 for BZERO 0: -0 becomes +0)",          # what spc_fits.hip did until this table was written
)


def _fused(v, s, z, work):
    """v * s + z with ONE rounding to *work*, exactly (finite values; the others as numpy gives them)"""
    with np.errstate(all="ignore"):
        out = (v * s + z).astype(work)
    for i in np.flatnonzero(np.isfinite(v)):
        out[i] = work(Fraction(float(v[i])) * Fraction(float(s)) + Fraction(float(z))) if work is np.float64 else \
            np.float32(np.float64(v[i]) * np.float64(s) + np.float64(z))        # (24 x 24 bits and the add fit float64's 53 here)
    return out


def model(payload, n, bitpix, bscale=1.0, bzero=0.0, blank=None, out_dtype=np.float32, defect=None):
    """the decode spc_fits.hip documents, byte by byte, written apart from oracle_np.fits_decode; *defect*: one of DEFECTS"""
    assert defect is None or defect in DEFECTS
    out_dtype = np.dtype(out_dtype).type
    bps = BYTES[bitpix]
    b = np.frombuffer(payload, dtype=np.uint8, count=n * bps).reshape(n, bps)
    if defect == "no swap":
        le = b
    elif defect == "swap at the wrong width" and bps == 2 and n >= 2:        # 16-bit samples swapped as 32-bit words
        le = b.copy()
        pairs = b[:n // 2 * 2].reshape(-1, 4)[:, ::-1]
        le[:n // 2 * 2] = pairs.reshape(-1, 2)
    elif defect == "swap at the wrong width" and bps >= 4:                   # swapped as two halves
        h = bps // 2
        le = np.concatenate([b[:, :h][:, ::-1], b[:, h:][:, ::-1]], axis=1)
    else:
        le = b[:, ::-1]
    u = np.ascontiguousarray(le).view("<u%d" % bps).reshape(n)
    sentinel = out_dtype(SENTINEL)
    with np.errstate(all="ignore"):
        if bitpix < 0:
            v = u.view("<f%d" % bps).astype("f%d" % bps)
            work = v.dtype.type
            if defect == "-64 scaled in float32" and bitpix == -64 and (bscale != 1.0 or bzero != 0.0):
                v, work = v.astype(np.float32), np.float32
            r, has_blank = u.view("<i%d" % bps).astype(np.int64), defect == "BLANK applied to float images" and blank is not None
        else:
            if bitpix == 8:
                r = u.view(np.int8).astype(np.int64) if defect == "uint8 read as signed" else u.astype(np.int64)
            elif bitpix == 16 and defect == "int16 without sign extension":
                r = u.astype(np.int64)
            else:
                r = u.view("<i%d" % bps).astype(np.int64)
            has_blank = blank is not None
            work = np.float32 if bitpix in (8, 16) else np.float64
            if defect == "8/16 scaled in float64" and bitpix in (8, 16):
                work = np.float64
            if defect == "32/64 scaled in float32" and bitpix in (32, 64) and (bscale != 1.0 or bzero != 0.0):
                work = np.float32
            if bitpix == 64 and bscale == 1.0 and bzero == 2.0 ** 63:
                v, work, bzero = (r.view(np.uint64) ^ np.uint64(1 << 63)).astype(out_dtype), out_dtype, 0.0      # the uint64, one rounding
            elif bitpix == 64 and defect == "int64 narrowed in one rounding":
                v = r.astype(out_dtype).astype(work)
            else:
                v = r.astype(work)
        if defect == "multiply-add fused into one rounding" and bscale != 1.0 and bzero != 0.0:
            v = _fused(v, work(bscale), work(bzero), work)
        else:
            if bscale != 1.0:
                v = v * work(bscale)
            if bzero != 0.0 or (defect is not None and defect.startswith("identity add") and bscale != 1.0):
                v = v + work(bzero)
        if has_blank:
            if defect == "BLANK compared after scaling":
                hit = v == blank
            elif defect == "BLANK compared unsigned":
                hit = (u.astype(object) == blank) if bitpix > 0 else (r == blank)
                hit = np.asarray(hit, dtype=bool)
            else:
                hit = r == blank
            v = v.copy()
            v[hit] = np.nan
        out = v.astype(out_dtype)
    if defect == "NaN payload canonicalised":
        out[np.isnan(out)] = out_dtype(np.nan)
    if defect == "last n % 4 samples skipped" and n % 4:
        out[n - n % 4:] = sentinel
    return out
