"""GPU: FITS decode and encode (csrc/spc_fits.hip, io_fits.py, the FITS source / sink of streaming.py) pinned sample by
sample at every BITPIX, scaling, BLANK, chunk seam, row strip, ragged end and alignment.

Through the C ABI: spc_fits_to_f32 / spc_fits_to_f64 against the fixture tests/golden/fits_decode_edges.npz (what astropy
read from files it wrote; test_fits_decode_host.py shows which decode defects it can tell) and against
oracle_np.fits_decode on generated payloads, bit for bit - NaNs that went through arithmetic or BLANK only have to be NaNs,
NaNs of an unscaled float image keep their payload.  Through the reader: load_cube over chunk sizes, buffer counts, reader
threads, row strips and a reused Staging; SpectralCube.read resident and out of core.  Through the writers: the payload
bytes of save_cube and of the streamed writer.

Every comparison is exact: no tolerance anywhere.  Measured on an MI355X: the 232 cases of this file take 6.2 s together, the
slowest (save_cube of a (9, 16, 24) cube in 16-byte chunks) 0.45 s, the two 134 MB decodes 0.27 s each.
"""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import fits_edges as F
import oracle_np as O
from spectral_cube_amd import SpectralCube, _lib, io_fits, streaming
from spectral_cube_amd.device import DeviceArray, Stream, synchronize

pytestmark = pytest.mark.gpu

GUARD = 16
NS = (0, 1, 2, 3, 4, 5, 7, 8, 15, 17, 255, 257, 1023, 1025, 4095, 4097, 8195)
BIG_N = 8192 * 4096 + 4099                 # past the grid cap of 8192 blocks x 4096 samples, ragged end
HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CDELT1": -1e-3, "CDELT2": 1e-3, "CDELT3": 0.5, "CUNIT3": "km/s",
       "CRPIX1": 1.0, "CRPIX2": 4.0, "CRPIX3": 1.0, "CRVAL1": 10.0, "CRVAL2": 20.0, "CRVAL3": -16.0, "BUNIT": "K"}


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def decode(payload, n, bitpix, bscale=1.0, bzero=0.0, blank=None, out_dtype=np.float32, raw_off=0, out_off=0, expect=None):
    """spc_fits_to_f32 / _f64 on *payload* placed raw_off samples into its buffer, writing out_off samples (+ the guard)
    into a buffer that holds a sentinel: the n decoded samples; nothing else in the buffer may have changed.
    expect: the call is left to the caller (a refusal test): (entry, args, output buffer, the sentinel's bits) come back."""
    out_dtype = np.dtype(out_dtype)
    bps = F.BYTES.get(bitpix, 4)
    host_raw = np.zeros(max(max(n, 0) * bps, len(payload)) + 4 * bps + 16, dtype=np.uint8)
    host_raw[raw_off * bps:raw_off * bps + len(payload)] = np.frombuffer(payload, dtype=np.uint8)
    d_raw = DeviceArray.from_numpy(host_raw)
    total = GUARD + 4 + max(n, 0) + GUARD
    d_out = DeviceArray.from_numpy(np.full(total, F.SENTINEL, dtype=out_dtype))
    assert d_raw.ptr % 16 == 0 and d_out.ptr % 16 == 0            # the offsets below decide the alignment
    first = GUARD + out_off
    entry = "spc_fits_to_f64" if out_dtype == np.float64 else "spc_fits_to_f32"
    args = (0, None, C.c_void_p(d_raw.ptr + raw_off * bps), bitpix, float(bscale), float(bzero), 0 if blank is None else 1,
            0 if blank is None else int(blank), n, C.c_void_p(d_out.ptr + first * out_dtype.itemsize))
    sentinel = F.bits(np.full(1, F.SENTINEL, dtype=out_dtype))[0]
    if expect is not None:
        return entry, args, d_out, sentinel
    _lib.call(entry, *args)
    synchronize(0)
    res = d_out.get()
    assert (F.bits(res[:first]) == sentinel).all() and (F.bits(res[first + n:]) == sentinel).all(), "wrote outside its n samples"
    return np.array(res[first:first + n])


def check(payload, n, bitpix, bscale, bzero, blank, out_dtype, exp, what, **kw):
    got = decode(payload, n, bitpix, bscale, bzero, blank, out_dtype, **kw)
    F.assert_same(got, np.asarray(exp).reshape(-1), F.exact_nan(bitpix, bscale, bzero), what)


def outs(bitpix):
    return (np.float32, np.float64) if bitpix in F.WIDE else (np.float32,)


@pytest.mark.parametrize("name", F.fixture().names)
def test_c_abi_on_every_fixture_file(gpu, name):
    fx = F.fixture()
    bitpix, bscale, bzero, blank = fx.args(name)
    card = fx.meta[name]["blank_card"]                  # (a float image's BLANK card is handed over too: it must be ignored)
    for out in outs(bitpix):
        for off in (0, 1):
            check(fx.payload(name), 105, bitpix, bscale, bzero, card, out, fx.expected(name, out), "%s -> %s, offset %d" % (name, out.__name__, off),
                  raw_off=off, out_off=off)


# what the generated payloads are decoded with: unscaled, and a scaling with a BLANK that the edge vector holds
def _settings(bitpix):
    if bitpix < 0:
        return [(1.0, 0.0, None), (0.3, 1.7, None), (0.1, 0.0, None)]
    blank = {8: 255, 16: -32768, 32: -2 ** 31, 64: -2 ** 63}[bitpix]
    unsigned = (1.0, 2.0 ** (bitpix - 1), blank) if bitpix > 8 else (1.0, -128.0, 0)
    return [(1.0, 0.0, None), (0.0125, 3.5, blank), (-1.0, 0.0, 0), unsigned]


@pytest.mark.parametrize("bitpix", [8, 16, 32, 64, -32, -64])
def test_c_abi_on_generated_payloads_of_every_length(gpu, bitpix):
    """n from 0 over the 4-sample groups and the 256 x 4 x 4 samples of a block to several blocks, each with a ragged end"""
    for n in NS:
        raw = F.generated(bitpix, n)
        payload = F.to_payload(raw)
        for bscale, bzero, blank in _settings(bitpix):
            for out in outs(bitpix):
                exp = O.fits_decode(payload, bitpix, (n,), bscale, bzero, blank, out_dtype=out)
                model = F.model(payload, n, bitpix, bscale, bzero, blank, out_dtype=out)
                F.assert_same(model, exp, F.exact_nan(bitpix, bscale, bzero), "the oracle against the model, n = %d" % n)
                check(payload, n, bitpix, bscale, bzero, blank, out, exp, "BITPIX %d n = %d (%r, %r, BLANK %r) -> %s" % (
                    bitpix, n, bscale, bzero, blank, out.__name__))


@pytest.mark.parametrize("bitpix", [8, 16, 32, 64, -32, -64])
def test_c_abi_at_every_alignment(gpu, bitpix):
    """raw and out start 0..3 samples into 16-byte aligned buffers: every pair for BITPIX -32 (whose 16-byte path has to step
    aside for anything but (0, 0)), both diagonals for the other types"""
    pairs = [(a, b) for a in range(4) for b in range(4)] if bitpix == -32 else sorted({(a, a) for a in range(4)} | {(a, 3 - a) for a in range(4)})
    for n in (3, 5, 17, 257, 1025, 4097):
        raw = F.generated(bitpix, n, seed=1)
        payload = F.to_payload(raw)
        for bscale, bzero, blank in _settings(bitpix)[:2]:
            for out in outs(bitpix):
                exp = O.fits_decode(payload, bitpix, (n,), bscale, bzero, blank, out_dtype=out)
                for a, b in pairs:
                    check(payload, n, bitpix, bscale, bzero, blank, out, exp, "BITPIX %d n = %d raw + %d out + %d -> %s" % (
                        bitpix, n, a, b, out.__name__), raw_off=a, out_off=b)


@pytest.mark.parametrize("bitpix", [-32, 16])
def test_c_abi_past_the_grid_cap(gpu, bitpix):
    """8192 * 4096 + 4099 samples: every thread sweeps the grid more than once and the end is ragged (134 MB of output)"""
    n = BIG_N
    rng = np.random.default_rng(5)
    if bitpix == -32:                       # random BITS: every class of float32, payloads included, must come back as it went
        raw = rng.integers(0, 2 ** 32, size=n, dtype=np.uint32).view(np.float32)
        bscale, bzero, blank = 1.0, 0.0, None
    else:
        raw = rng.integers(-2 ** 15, 2 ** 15, size=n, dtype=np.int16)
        bscale, bzero, blank = 0.0125, 3.5, -32768
    vec = F.fixture().vector(bitpix)
    raw[1:1 + vec.size] = vec
    raw[n - vec.size:] = vec
    payload = F.to_payload(raw)
    exp = O.fits_decode(payload, bitpix, (n,), bscale, bzero, blank)
    if bitpix == -32:
        assert np.array_equal(F.bits(exp), F.bits(raw))
    check(payload, n, bitpix, bscale, bzero, blank, np.float32, exp, "BITPIX %d, %d samples" % (bitpix, n))


@pytest.mark.parametrize("entry_dtype, bitpix, n, null", [
    (np.float32, 0, 8, None), (np.float32, 24, 8, None), (np.float32, -16, 8, None), (np.float32, -8, 8, None),
    (np.float64, 8, 8, None), (np.float64, 16, 8, None), (np.float64, -32, 8, None), (np.float64, 7, 8, None),
    (np.float32, -32, -1, None), (np.float64, -64, -1, None),
    (np.float32, -32, 8, "raw"), (np.float32, -32, 8, "out"), (np.float64, 64, 8, "raw"), (np.float64, 64, 8, "out"),
])
def test_c_abi_refusals_leave_the_output_untouched(gpu, entry_dtype, bitpix, n, null):
    payload = bytes(range(1, 65))
    entry, args, d_out, sentinel = decode(payload, n, bitpix, out_dtype=entry_dtype, expect=_lib.HipInvalidArgument)
    args = list(args)
    if null == "raw":
        args[2] = None
    if null == "out":
        args[9] = None
    with pytest.raises(_lib.HipInvalidArgument):
        _lib.call(entry, *args)
    synchronize(0)
    assert (F.bits(d_out.get()) == sentinel).all()


# ---- the reader ----------------------------------------------------------------------------------------------------------
SHAPES = ((3, 5, 7), (4, 3, 5), (2, 1, 1), (1, 1, 3), (9, 16, 24))
CHUNKS = (1, 48, 100, 4096, None)          # None: the default
# one scaling and BLANK per sample type for the files io_fits.write_fits makes (the fixture holds every combination)
WRITTEN = {8: (0.0125, 3.5, 255), 16: (0.1, 0.0, -32768), 32: (1e-4, -2.0, -2 ** 31), 64: (1.0, 2.0 ** 63, -2 ** 63), -32: (1.0, 0.0, None),
           -64: (0.3, 1.7, None)}


def written_file(tmp_path, bitpix, shape, seed=0):
    """a file of generated samples by io_fits.write_fits, and (payload, bscale, bzero, blank)"""
    n = int(np.prod(shape))
    raw = F.generated(bitpix, n, seed).reshape(shape)
    bscale, bzero, blank = WRITTEN[bitpix]
    path = str(tmp_path / ("w%d_%s_%d.fits" % (bitpix, "x".join(map(str, shape)), seed)))
    io_fits.write_fits(path, raw, header=HDR, bitpix=bitpix, bscale=None if bscale == 1.0 else bscale,
                       bzero=None if bzero == 0.0 else bzero, blank=blank)
    img = io_fits.find_image(path)
    with open(path, "rb") as f:
        f.seek(img.data_offset)
        payload = f.read(img.nbytes)
    assert payload == F.to_payload(raw) and (img.bscale, img.bzero, img.blank) == (bscale, bzero, blank)
    return path, payload, (bscale, bzero, blank)


def _pairwise():
    """30 of the 6 x 5 x 3 x 5 x 2 = 900 (BITPIX, chunk_bytes, nbuffers, shape, readers) settings that hold every PAIR of values"""
    rows = [(b, c, (b + c) % 3, (b + 2 * c) % 5, ((b + c) // 3) % 2) for b in range(6) for c in range(5)]
    sizes = (6, 5, 3, 5, 2)
    for i in range(5):
        for j in range(i + 1, 5):
            assert len({(r[i], r[j]) for r in rows}) == sizes[i] * sizes[j], (i, j)
    return [((8, 16, 32, 64, -32, -64)[b], CHUNKS[c], (1, 2, 3)[k], SHAPES[s], (1, 3)[r]) for b, c, k, s, r in rows]


@pytest.mark.parametrize("bitpix, chunk_bytes, nbuffers, shape, readers", _pairwise())
def test_load_cube_over_chunks_buffers_and_readers(gpu, tmp_path, bitpix, chunk_bytes, nbuffers, shape, readers):
    path, payload, (bscale, bzero, blank) = written_file(tmp_path, bitpix, shape)
    kw = dict(nbuffers=nbuffers, readers=readers)
    if chunk_bytes is not None:
        kw["chunk_bytes"] = chunk_bytes
    for out in outs(bitpix):
        dev, hdr = io_fits.load_cube(path, dtype=out, **kw)
        assert dev.shape == shape and dev.dtype == out and hdr["NAXIS"] == 3 and hdr["BUNIT"] == "K"
        exp = O.fits_decode(payload, bitpix, shape, bscale, bzero, blank, out_dtype=out)
        F.assert_same(dev.get(), exp, F.exact_nan(bitpix, bscale, bzero), "load_cube(%s, dtype=%s)" % (kw, out.__name__))


@pytest.mark.parametrize("name", F.fixture().names)
def test_load_cube_on_every_fixture_file(gpu, tmp_path, name):
    fx = F.fixture()
    bitpix, bscale, bzero, blank = fx.args(name)
    path = tmp_path / (name + ".fits")
    path.write_bytes(fx.file(name))
    img = io_fits.find_image(str(path))
    assert (img.bitpix, img.bscale, img.bzero, img.data_offset) == (bitpix, bscale, bzero, fx.meta[name]["data_offset"])
    assert img.blank == fx.meta[name]["blank_card"]
    for out in outs(bitpix):
        for kw in ({}, dict(chunk_bytes=48, nbuffers=2, readers=2)):
            dev, _ = io_fits.load_cube(str(path), dtype=out, **kw)
            F.assert_same(dev.get(), fx.expected(name, out), F.exact_nan(bitpix, bscale, bzero), "%s load_cube(%s) -> %s" % (name, kw, out.__name__))


@pytest.mark.parametrize("bitpix", [8, 16, 32, 64, -32, -64])
def test_load_cube_refuses_float64_of_narrow_types_and_bad_rows(gpu, tmp_path, bitpix):
    path, _, _ = written_file(tmp_path, bitpix, (4, 3, 5))
    if bitpix in F.WIDE:
        assert io_fits.load_cube(path, dtype=np.float64)[0].dtype == np.float64
    else:
        with pytest.raises(ValueError, match="float64"):
            io_fits.load_cube(path, dtype=np.float64)
    for rows in ((0, 0), (2, 1), (-1, 2), (0, 4)):
        with pytest.raises(ValueError, match="rows"):
            io_fits.load_cube(path, rows=rows)


@pytest.mark.parametrize("bitpix", [8, 16, 32, 64, -32, -64])
def test_load_cube_row_strips(gpu, tmp_path, bitpix):
    """rows=(y0, y1): single rows, strips whose ny * nx is odd (the decoded chunks then start 4 bytes off a 16-byte line),
    one and many chunks, values and the shifted CRPIX2"""
    for shape, strips, chunks in (((3, 5, 7), ((0, 1), (1, 4), (2, 5), (4, 5), (0, 5)), (1, 100, None)),
                                  ((9, 16, 24), ((3, 4), (5, 16), (0, 7)), (100, 4096))):
        path, payload, (bscale, bzero, blank) = written_file(tmp_path, bitpix, shape, seed=2)
        for out in outs(bitpix):
            whole = O.fits_decode(payload, bitpix, shape, bscale, bzero, blank, out_dtype=out)
            for y0, y1 in strips:
                for chunk_bytes in chunks:
                    kw = {} if chunk_bytes is None else dict(chunk_bytes=chunk_bytes)
                    dev, hdr = io_fits.load_cube(path, rows=(y0, y1), nbuffers=2, readers=2, dtype=out, **kw)
                    assert dev.shape == (shape[0], y1 - y0, shape[2])
                    F.assert_same(dev.get(), whole[:, y0:y1], F.exact_nan(bitpix, bscale, bzero), "BITPIX %d rows (%d, %d) of %s, chunk_bytes %s -> %s" % (
                        bitpix, y0, y1, shape, chunk_bytes, out.__name__))
                    assert hdr["NAXIS2"] == y1 - y0 and hdr["CRPIX2"] == HDR["CRPIX2"] - y0 and hdr["CRPIX1"] == HDR["CRPIX1"]


def test_one_staging_across_files_of_every_type(gpu, tmp_path):
    """the pinned buffers and their device twins of one Staging serve file after file, from the largest payload down: what
    an earlier file left behind in them must not reach a later cube"""
    st = io_fits.Staging(0, chunk_bytes=4096, nbuffers=3)
    try:
        order = [(64, (9, 16, 24)), (-64, (9, 16, 24)), (32, (9, 16, 24)), (-32, (9, 16, 24)), (16, (9, 16, 24)), (8, (9, 16, 24)),
                 (64, (3, 5, 7)), (-64, (4, 3, 5)), (32, (3, 5, 7)), (-32, (4, 3, 5)), (16, (3, 5, 7)), (8, (4, 3, 5)), (-32, (1, 1, 3)), (16, (2, 1, 1)),
                 (8, (1, 1, 3))]
        for k, (bitpix, shape) in enumerate(order):
            path, payload, (bscale, bzero, blank) = written_file(tmp_path, bitpix, shape, seed=10 + k)
            for rows in (None, (0, 1), (shape[1] // 2, shape[1])):
                for out in outs(bitpix):
                    dev, _ = io_fits.load_cube(path, staging=st, rows=rows, readers=2, dtype=out)
                    exp = O.fits_decode(payload, bitpix, shape, bscale, bzero, blank, out_dtype=out)
                    exp = exp if rows is None else exp[:, rows[0]:rows[1]]
                    F.assert_same(dev.get(), exp, F.exact_nan(bitpix, bscale, bzero), "file %d (BITPIX %d %s rows %s) through the shared Staging" % (
                        k, bitpix, shape, rows))
        with pytest.raises(ValueError, match="does not fit"):
            io_fits.load_cube(written_file(tmp_path, -64, (2, 32, 24))[0], staging=st, rows=(0, 32), dtype=np.float64)
    finally:
        st.close()


BLANKED = [n for n in F.fixture().names if F.fixture().meta[n]["blank"] is not None]


@pytest.mark.parametrize("name", BLANKED)
def test_cube_read_of_blanked_integer_files_resident_and_out_of_core(gpu, tmp_path, monkeypatch, name):
    """SpectralCube.read(path) of every integer file with a BLANK: resident (load_cube) and out of core (FitsSource strips):
    both hold the expectation, and the isfinite mask the reader attaches excludes exactly the blanked samples"""
    fx = F.fixture()
    bitpix, bscale, bzero, blank = fx.args(name)
    path = tmp_path / (name + ".fits")
    off = fx.meta[name]["data_offset"]
    cards = fx.file(name)[:off].decode("ascii")
    cards = [cards[i:i + 80] for i in range(0, off, 80)]
    cards = cards[:[c.startswith("END ") for c in cards].index(True)]        # astropy's cards, then a spectral-cube WCS
    text = "".join(cards + [io_fits._card(k, v) for k, v in HDR.items()] + ["END".ljust(80)])
    path.write_bytes((text + " " * (-len(text) % 2880)).encode("ascii") + fx.file(name)[off:])
    exp = fx.expected(name)
    raw = np.frombuffer(fx.payload(name), dtype=np.dtype(F._RAW[bitpix]).newbyteorder(">")).reshape(fx.shape)
    blanked = raw == blank
    assert blanked.any() and not blanked.all() and np.array_equal(np.isnan(exp), blanked)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")              # (BITPIX 32 / 64 read as float32: a PrecisionWarning)
        cube = SpectralCube.read(str(path))
        assert cube._stream_source() is None
        F.assert_same(cube._device_data().get(), exp, False, name + " resident")
        assert np.array_equal(cube.get_mask_array(), ~blanked)
        if bitpix in F.WIDE:
            F.assert_same(cube._device_data64().get(), fx.expected(name, np.float64), False, name + " resident, float64")
        monkeypatch.setenv("SPC_HBM_BUDGET", "200")            # below the cube's 420 bytes, above one plane with its mask
        big = SpectralCube.read(str(path))
        assert isinstance(big._stream_source(), streaming.FitsSource) and big._dev is None
        planes = np.stack([np.asarray(big[z]) for z in range(fx.shape[0])]).astype(np.float32)
        assert big._dev is None, "never made resident"
        F.assert_same(planes, exp, False, name + " out of core")
        assert np.array_equal(np.isfinite(planes), ~blanked)


# ---- the writers -----------------------------------------------------------------------------------------------------------
def edge_cube(shape, seed=0):
    """float32 (nz, ny, nx) that carries the BITPIX -32 edge vector (every class of value, NaN payloads, -0, denormals)"""
    return F.generated(-32, int(np.prod(shape)), seed).reshape(shape)


def check_written(path, d):
    data = open(path, "rb").read()
    img = io_fits.find_image(path)
    assert img.bitpix == -32 and io_fits.cube_shape(img) == d.shape and (img.bscale, img.bzero, img.blank) == (1.0, 0.0, None)
    assert img.data_offset % 2880 == 0 and len(data) % 2880 == 0 and len(data) == img.data_offset + d.nbytes + (-d.nbytes) % 2880
    body = data[img.data_offset:img.data_offset + d.nbytes]
    want = d.astype(">f4").tobytes()
    assert want == F.to_payload(d)                          # (numpy's own swap moves the bits too)
    if body != want:
        a, b = np.frombuffer(body, dtype=">u4"), np.frombuffer(want, dtype=">u4")
        at = np.flatnonzero(a != b)
        raise AssertionError("%d of %d samples differ in the file, first at %s: %s, expected %s" % (
            at.size, a.size, at[:6].tolist(), [hex(int(x)) for x in a[at[:6]]], [hex(int(x)) for x in b[at[:6]]]))
    assert not any(data[img.data_offset + d.nbytes:]), "padding is not zero"
    back, _ = io_fits.load_cube(path, chunk_bytes=48, nbuffers=2)
    assert np.array_equal(back.get().view(np.uint32), d.view(np.uint32))


@pytest.mark.parametrize("shape", [(3, 5, 7), (1, 1, 3), (2, 1, 1), (5, 9, 7), (9, 16, 24)])
def test_save_cube_payload_bytes(gpu, tmp_path, shape):
    """payloads that are no multiple of 16 bytes, chunks of 16 bytes to the whole file, 1 to 4 buffers in rotation"""
    d = edge_cube(shape)
    dev = DeviceArray.from_numpy(d)
    for chunk_bytes in (16, 48, 112, 4096):
        for nbuffers in (1, 2, 4):
            path = str(tmp_path / ("s_%d_%d.fits" % (chunk_bytes, nbuffers)))
            io_fits.save_cube(path, dev, header=HDR, chunk_bytes=chunk_bytes, nbuffers=nbuffers)
            check_written(path, d)
    with pytest.raises(OSError):
        io_fits.save_cube(path, dev, header=HDR)
    io_fits.save_cube(path, dev, header=HDR, overwrite=True)
    check_written(path, d)


@pytest.mark.parametrize("shape", [(5, 9, 7), (3, 19, 5), (4, 17, 24)])
def test_streamed_write_payload_bytes(gpu, tmp_path, monkeypatch, shape):
    """cube.write of an out-of-core cube (strips in, the plain copy, strips out through StripWriter and FitsSink): raw voxels
    (filled=False) arrive byte for byte; the filled form differs exactly where the reader's isfinite mask excludes"""
    d = edge_cube(shape, seed=3)
    nz, ny, nx = shape
    monkeypatch.setenv("SPC_HBM_BUDGET", str(4 * nz * 8 * nx))              # strips of 8 rows: ny is no multiple of 8
    assert 4 * d.size > streaming.hbm_budget(0)
    cube = SpectralCube.read(d.copy(), HDR)
    assert cube._stream_source() is not None
    path = str(tmp_path / "raw.fits")
    cube.write(path, filled=False)
    assert cube._dev is None
    check_written(path, d)
    assert [f for f in os.listdir(tmp_path) if "spc-part" in f] == []
    # from a FITS source onto a second file, and the filled form
    src = SpectralCube.read(path)
    assert isinstance(src._stream_source(), streaming.FitsSource)
    path2 = str(tmp_path / "again.fits")
    src.write(path2, filled=False)
    check_written(path2, d)
    path3 = str(tmp_path / "filled.fits")
    src.write(path3)
    img = io_fits.find_image(path3)
    got = np.frombuffer(open(path3, "rb").read()[img.data_offset:img.data_offset + d.nbytes], dtype=">u4").reshape(shape)
    fin = np.isfinite(d)
    assert np.array_equal(got[fin], d.view(np.uint32)[fin]) and np.isnan(got.astype(np.uint32).view(np.float32)[~fin]).all()


@pytest.mark.parametrize("chunk_bytes, nbuffers", [(16, 1), (48, 2), (112, 4), (4096, 2)])
def test_strip_writer_with_small_chunks(gpu, tmp_path, chunk_bytes, nbuffers):
    """StripWriter.put cuts a strip into chunks of planes: with odd rows * nx the chunks after the first start 4 bytes off
    a 16-byte line on the device (strip.ptr + z0 * seg) - the source of the byte-swap kernel"""
    shape = (7, 11, 5)
    d = edge_cube(shape, seed=4)
    nz, ny, nx = shape
    path = str(tmp_path / "w.fits")
    sink = streaming.FitsSink(path, HDR, shape)
    w = streaming.StripWriter(sink, 0, nbuffers=nbuffers, chunk_bytes=chunk_bytes, writers=2)
    produced = Stream(0)
    try:
        for y0, y1 in ((0, 3), (3, 4), (4, 11)):
            strip = DeviceArray.from_numpy(np.ascontiguousarray(d[:, y0:y1]))
            w.put(y0, y1, strip, produced)
    except BaseException:
        w.close(ok=False)
        raise
    w.close()
    check_written(path, d)
