"""CPU companion of test_gpu_fits.py.  The fixture tests/golden/fits_decode_edges.npz (files astropy wrote, what astropy read
from them, the expected float32 / float64 cubes) against oracle_np.fits_decode in both output types, bit for bit; a defect
table in the manner of test_mask_edges_host.py - a numpy model of the decode (fits_edges.model) is run with one defect at a
time and at least one fixture file must then fail, so the fixture can show each of them; and the header cards the reader has
to take (integer, E and D exponent BSCALE / BZERO, negative BLANK, BLANK on a float image, END opening the second block)
through io_fits.scan_hdus / FitsImage.  No GPU."""
import numpy as np
import pytest

import fits_edges as F
import oracle_np as O
from spectral_cube_amd import io_fits


def _outs(bitpix):
    return (np.float32, np.float64) if bitpix in F.WIDE else (np.float32,)


def test_the_fixture_holds_the_cases_of_the_issue():
    fx = F.fixture()
    by = {}
    for name in fx.names:
        m = fx.meta[name]
        by.setdefault(m["bitpix"], []).append((m["bscale"], m["bzero"], m["blank"], m["blank_card"]))
    assert sorted(by) == [-64, -32, 8, 16, 32, 64]
    common = [(1.0, 0.0), (0.0125, 3.5), (1e-4, -2.0), (0.1, 0.0), (1.0, 7.25), (-1.0, 0.0)]
    for bitpix, cases in by.items():
        scalings = {c[:2] for c in cases}
        extra = {8: (1.0, -128.0), 16: (1.0, 2.0 ** 15), 32: (1.0, 2.0 ** 31), 64: (1.0, 2.0 ** 63), -32: (0.3, 1.7), -64: (0.3, 1.7)}[bitpix]
        assert scalings == set(common) | {extra}, bitpix
        if bitpix > 0:
            present = int(fx.vector(bitpix)[-1 if bitpix == 8 else 0])
            for sc in ((1.0, 0.0), (0.0125, 3.5)):
                assert (sc + (present, present)) in cases and (sc + (0, 0)) in cases and (sc + (None, None)) in cases
            assert bitpix == 8 or (extra + (present, present)) in cases          # BLANK on a pseudo-unsigned image
        else:
            assert any(c[2] is None and c[3] is not None for c in cases)        # a BLANK card that is ignored
    assert sum(fx.meta[n]["astropy_deviates"] for n in fx.names) == 4 * 2 + 3   # BLANK = 0 (x 2 scalings), BLANK on unsigned
    # the edge vectors start at sample 2 (across 4-sample groups) and hold what the issue lists
    for bitpix in by:
        vec = fx.vector(bitpix)
        name = [n for n in fx.names if fx.meta[n]["bitpix"] == bitpix and n.endswith("_none")][0]
        raw = np.frombuffer(fx.payload(name), dtype=np.dtype(F._RAW[bitpix]).newbyteorder(">"))
        assert raw.size == 105 and fx.start == 2 and vec.size > 4
        assert np.array_equal(F.bits(raw[2:2 + vec.size].astype(vec.dtype)) if bitpix < -8 else raw[2:2 + vec.size], F.bits(vec) if bitpix < -8 else vec)
    assert {0, 1, 127, 128, 254, 255} == set(fx.vector(8).tolist())
    assert {-32768, -32767, -256, -255, -1, 0, 1, 255, 256, 0x0102, 32767} == set(fx.vector(16).tolist())
    assert {-2 ** 31, -2 ** 31 + 1, -1, 0, 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 3, 0x01020304, 2 ** 31 - 1} == set(fx.vector(32).tolist())
    tie = 2 ** 62 + 2 ** 38 + 1
    assert {-2 ** 63, -2 ** 63 + 1, -1, 0, 1, 2 ** 53, 2 ** 53 + 1, tie, -tie, 2 ** 39 + 1, 0x0102030405060708, 2 ** 63 - 1} == set(fx.vector(64).tolist())
    assert {0x0, 0x80000000, 0x1, 0x007fffff, 0x00800000, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0x7fc00001,
            0x7f800001, 0xffc12345, 0x01020304} == set(F.bits(fx.vector(-32)).tolist())
    v64 = fx.vector(-64)
    for x in (1e39, -1e39, 1e-46, 1e-40, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -52, np.finfo(np.float64).smallest_subnormal,
              np.finfo(np.float64).max, -np.finfo(np.float64).max, np.finfo(np.float64).tiny, np.inf, -np.inf):
        assert (v64 == x).any(), x
    assert np.isnan(v64).sum() == 4 and len(set(F.bits(v64[np.isnan(v64)]).tolist())) == 4 and np.signbit(v64[v64 == 0]).sum() == 1


@pytest.mark.parametrize("name", F.fixture().names)
def test_oracle_and_model_equal_the_fixture(name):
    fx = F.fixture()
    bitpix, bscale, bzero, blank = fx.args(name)
    for out in _outs(bitpix):
        exp = fx.expected(name, out)
        assert exp.dtype == out and exp.shape == fx.shape
        nan_bits = F.exact_nan(bitpix, bscale, bzero)
        got = O.fits_decode(fx.payload(name), bitpix, fx.shape, bscale, bzero, blank, out_dtype=out)
        F.assert_same(got, exp, nan_bits, "%s: oracle_np.fits_decode -> %s" % (name, out.__name__))
        got = F.model(fx.payload(name), 105, bitpix, bscale, bzero, blank, out_dtype=out).reshape(fx.shape)
        F.assert_same(got, exp, nan_bits, "%s: fits_edges.model -> %s" % (name, out.__name__))
        # astropy's own array, where it keeps the standard, is the expectation made float
        if not fx.meta[name]["astropy_deviates"] and not (bitpix in (32, 64) and out is np.float32):
            with np.errstate(all="ignore"):
                F.assert_same(fx.g[name + "_astropy"].astype(out), exp, nan_bits, name + ": astropy's array")
    if bitpix not in F.WIDE:
        with pytest.raises(ValueError):
            O.fits_decode(fx.payload(name), bitpix, fx.shape, bscale, bzero, blank, out_dtype=np.float64)


def test_astropy_quirks_are_the_three_named_ones():
    """astropy_quirks=True changes fits_decode on the files marked astropy_deviates and on no other; there it gives what
    astropy gave: no NaN for BLANK = 0 or on a pseudo-unsigned image"""
    fx = F.fixture()
    for name in fx.names:
        bitpix, bscale, bzero, blank = fx.args(name)
        for out in _outs(bitpix):
            std = O.fits_decode(fx.payload(name), bitpix, fx.shape, bscale, bzero, blank, out_dtype=out)
            quirk = O.fits_decode(fx.payload(name), bitpix, fx.shape, bscale, bzero, blank, out_dtype=out, astropy_quirks=True)
            differs = F.mismatch(quirk, std, F.exact_nan(bitpix, bscale, bzero)).any()
            assert differs == fx.meta[name]["astropy_deviates"], name
            if differs:
                assert not np.isnan(quirk).any() and np.isnan(std).sum() == (np.frombuffer(
                    fx.payload(name), dtype=np.dtype(F._RAW[bitpix]).newbyteorder(">")) == blank).sum() > 0
                a = fx.g[name + "_astropy"]
                ref = a.astype(np.float64).astype(out) if (bitpix == 32 or (bitpix == 64 and a.dtype != np.uint64)) else a.astype(out)
                F.assert_same(quirk, ref, False, name + ": astropy_quirks against astropy's array")


def test_the_values_the_product_pins_where_astropy_differs():
    """BITPIX 64 reaches float32 through float64 (two roundings; astype(float32) of the integers is one), except the uint64
    of BSCALE 1, BZERO 2**63, which is rounded once; BLANK = 0 and BLANK on unsigned images blank"""
    fx = F.fixture()
    tie = 2 ** 62 + 2 ** 38 + 1
    v = fx.vector(64)
    e = fx.expected("b64_none")
    at = fx.start + int(np.flatnonzero(v == tie)[0])
    assert e.ravel()[at] == np.float32(2.0 ** 62) and np.int64(tie).astype(np.float32) == np.float32(2.0 ** 62 + 2.0 ** 39)
    assert e.ravel()[at + 1] == -np.float32(2.0 ** 62)
    at = fx.start + int(np.flatnonzero(v == 2 ** 39 + 1)[0])
    assert fx.expected("b64_unsigned").ravel()[at] == np.float32(2.0 ** 63 + 2.0 ** 40)      # (float64 first would give 2**63)
    assert fx.expected("b64_unsigned", np.float64).ravel()[at] == 2.0 ** 63 + 2.0 ** 39
    for name in ("b8_none_blank0", "b16_s0125_blank0", "b16_unsigned_blank", "b32_unsigned_blank", "b64_unsigned_blank"):
        assert np.isnan(fx.expected(name)).any() and not np.isnan(fx.g[name + "_astropy"].astype(np.float64)).any(), name
    # (-1, 0): -1 * 0 is -0 and stays -0 (no BZERO is added)
    e = fx.expected("b16_neg").ravel()
    z = fx.start + int(np.flatnonzero(fx.vector(16) == 0)[0])
    assert e[z] == 0 and np.signbit(e[z])


def test_every_defect_is_caught_by_some_fixture_file():
    fx = F.fixture()
    table = {}
    for defect in F.DEFECTS:
        caught = []
        for name in fx.names:
            bitpix, bscale, bzero, blank = fx.args(name)
            if defect == "BLANK applied to float images":
                blank = fx.meta[name]["blank_card"]
            for out in _outs(bitpix):
                got = F.model(fx.payload(name), 105, bitpix, bscale, bzero, blank, out_dtype=out, defect=defect).reshape(fx.shape)
                if F.mismatch(got, fx.expected(name, out), F.exact_nan(bitpix, bscale, bzero)).any():
                    caught.append(name + ("" if out is np.float32 else ":f64"))
        table[defect] = caught
        print("%-58s caught by %2d cases, e.g. %s" % (defect, len(caught), ", ".join(caught[:3])))
    missed = [d for d, c in table.items() if not c]
    assert not missed, "the fixture cannot show: %s" % missed
    # a defect of one sample type is shown by files of that type, scaled ones only by scaled files
    assert all(c.startswith("b16_") for c in table["int16 without sign extension"])
    assert all(c.startswith("b8_") for c in table["uint8 read as signed"])
    assert all(c.startswith("b64_") for c in table["int64 narrowed in one rounding"])
    assert all(c.startswith(("f32_", "f64_")) and c.split(":")[0].endswith("_blankcard") for c in table["BLANK applied to float images"])
    assert all(c.split(":")[0].endswith("_none") or "blankcard" in c for c in table["NaN payload canonicalised"])
    assert {"b16_s01", "b16_s0125"} <= set(table["8/16 scaled in float64"])
    assert {"b32_s01", "b64_s0125"} <= set(table["32/64 scaled in float32"])
    fused = set(table["multiply-add fused into one rounding"])
    assert any(c.endswith("_s0125") for c in fused) and any(c.endswith("_s1em4") for c in fused)


# ---- header cards ----------------------------------------------------------------------------------------------------
def _file(tmp_path, name, cards, payload):
    text = "".join(c.ljust(80) for c in cards + ["END"])
    assert all(len(c) <= 80 for c in cards)
    text += " " * ((-len(text)) % 2880)
    p = tmp_path / name
    p.write_bytes(text.encode("ascii") + payload + b"\0" * ((-len(payload)) % 2880))
    return str(p)


def _base(bitpix, shape=(2, 3, 4)):
    return ["SIMPLE  =                    T / conforms to FITS standard", "BITPIX  = %20d / array data type" % bitpix,
            "NAXIS   =                    3", "NAXIS1  = %20d" % shape[2], "NAXIS2  = %20d" % shape[1], "NAXIS3  = %20d" % shape[0]]


@pytest.mark.parametrize("cards, bscale, bzero, blank", [
    (["BSCALE  =                    1", "BZERO   =                32768"], 1.0, 32768.0, None),
    (["BSCALE  =                    1 / default scaling factor", "BZERO   =  9223372036854775808 / offset data range to that of unsigned long"],
     1.0, 2.0 ** 63, None),
    (["BSCALE  =             1.25E-02", "BZERO   =              3.5E+00 / offset"], 0.0125, 3.5, None),
    (["BSCALE  =             1.25D-02", "BZERO   =             -2.0D+00"], 0.0125, -2.0, None),
    (["BSCALE  =               1.0D-4 / a comment with = and 'quotes'", "BZERO   =                  -2."], 1e-4, -2.0, None),
    (["BLANK   =               -32768 / value of undefined pixels"], 1.0, 0.0, -32768),
    (["BZERO   =                  7.25", "BLANK   =                    0"], 1.0, 7.25, 0),
])
def test_header_cards_of_an_integer_image(tmp_path, cards, bscale, bzero, blank):
    raw = F.generated(16, 24)
    path = _file(tmp_path, "a.fits", _base(16) + cards, F.to_payload(raw))
    (img,) = io_fits.scan_hdus(path)
    assert (img.bitpix, img.bscale, img.bzero, img.blank) == (16, bscale, bzero, blank)
    assert isinstance(img.bscale, float) and isinstance(img.bzero, float) and (blank is None or isinstance(img.blank, int))
    assert img.data_offset == 2880 and img.nbytes == 48 and io_fits.cube_shape(img) == (2, 3, 4)
    assert io_fits.find_image(path).data_offset == 2880


def test_blank_card_on_a_float_image_is_parsed_and_left_to_the_decoder(tmp_path):
    path = _file(tmp_path, "f.fits", _base(-32) + ["BLANK   =             16909060"], F.to_payload(F.generated(-32, 24)))
    (img,) = io_fits.scan_hdus(path)
    assert img.bitpix == -32 and img.blank == 16909060 and (img.bscale, img.bzero) == (1.0, 0.0)
    # (load_cube and FitsSource pass has_blank only where BITPIX > 0, and spc_fits_to_f32 ignores it otherwise: test_gpu_fits.py)


def test_header_of_exactly_36_cards_puts_end_into_the_second_block(tmp_path):
    raw = F.generated(16, 24)
    cards = _base(16) + ["BSCALE  =               1.0E-01", "BZERO   =                    0", "BLANK   =               -32768"]
    cards += ["KEY%05d= %20d" % (i, i) for i in range(36 - len(cards))]
    assert len(cards) == 36
    path = _file(tmp_path, "b.fits", cards, F.to_payload(raw))
    (img,) = io_fits.scan_hdus(path)
    assert img.data_offset == 2 * 2880 and (img.bscale, img.bzero, img.blank) == (0.1, 0.0, -32768) and img.header["KEY00026"] == 26
    with open(path, "rb") as f:
        f.seek(img.data_offset)
        assert f.read(img.nbytes) == F.to_payload(raw)
    # 35 cards: END closes the first block
    path = _file(tmp_path, "c.fits", cards[:35], F.to_payload(raw))
    assert io_fits.scan_hdus(path)[0].data_offset == 2880


def test_write_fits_lays_down_the_cards_it_is_given(tmp_path):
    """the writer the GPU tests make their files with: raw samples as they are, BSCALE / BZERO / BLANK as cards that scan back"""
    for bitpix, sc, blank in ((8, (1.0, -128.0), 255), (16, (0.0125, 3.5), -32768), (32, (1.0, 2.0 ** 31), None),
                              (64, (1.0, 2.0 ** 63), -2 ** 63), (-32, (0.3, 1.7), None), (-64, None, None)):
        raw = F.generated(bitpix, 30).reshape(2, 3, 5)
        p = str(tmp_path / ("w%d.fits" % bitpix))
        io_fits.write_fits(p, raw, bitpix=bitpix, bscale=sc and sc[0], bzero=sc and sc[1], blank=blank)
        (img,) = io_fits.scan_hdus(p)
        assert (img.bitpix, img.bscale, img.bzero, img.blank) == (bitpix, (sc or (1.0, 0.0))[0], (sc or (1.0, 0.0))[1], blank)
        data = open(p, "rb").read()
        assert len(data) % 2880 == 0 and data[img.data_offset:img.data_offset + img.nbytes] == F.to_payload(raw)
        assert not any(data[img.data_offset + img.nbytes:])
