"""The host half of the PNG decoder (csrc/pngdec_host.h through thmr_png_probe / _inflate_window / _inflate / _decode_host), without a
device.  Every comparison is bit-exact.  The files are written at test time by tests/_png_dec_cases.py (given samples, given filters),
by Pillow and by this project's own encoder; the references are Pillow's decode of the same bytes and the contract computed from the
samples (for 16-bit grey + alpha the contract — the high byte of the grey sample — stands on its own: Pillow has no mode for it)."""
import ctypes
import io
import os
import struct
import zlib

import numpy as np
import pytest

import _eval_dataset_fixture as F
import _png_dec_cases as K
from tokenhmr_amd import _cabi


@pytest.fixture(scope="module")
def P(built_lib):
    from tokenhmr_amd import png
    return png


def check(P, data, want_rgb, ctype, depth, what):
    ref = K.pillow_rgb(data, ctype, depth)
    if ref is not None:
        assert np.array_equal(ref, want_rgb), ("Pillow against the contract", what)
    assert np.array_equal(P.decode_host(data, bgr=False), want_rgb), what
    assert np.array_equal(P.decode_host(data, bgr=True), want_rgb[:, :, ::-1]), what


def test_the_word_layouts_are_the_headers(P):
    """The info and the plan cross the C ABI as int32 words; png.py's named views of them follow the header's index constants."""
    import re
    with open(_cabi.HEADER) as f:
        header = f.read()
    consts = {k: int(v) for k, v in re.findall(r"\bTHMR_PNG_((?:INFO|PLAN)_[A-Z0-9_]+) = (\d+)\b", header)}
    assert consts["INFO_WORDS"] == _cabi.PNG_INFO_WORDS == ctypes.sizeof(P.PngInfo) // 4 and consts["PLAN_PALETTE"] == _cabi.PNG_PLAN_PALETTE
    assert 14 + 192 == _cabi.PNG_PLAN_WORDS == ctypes.sizeof(P.PngPlan) // 4 and "THMR_PNG_PLAN_WORDS = 14 + 192" in header
    for prefix, fields, view in (("INFO_", _cabi.PNG_INFO_FIELDS, P.PngInfo), ("PLAN_", _cabi.PNG_PLAN_FIELDS, P.PngPlan)):
        for k, name in enumerate(fields):
            assert consts[prefix + name.upper()] == k and getattr(view, name).offset == 4 * k and getattr(view, name).size == 4, name
        named = {k[len(prefix):].lower() for k in consts if k.startswith(prefix)} - {"words", "palette"}
        assert named == set(fields), prefix           # the header names no word that the view lacks
    assert P.PngPlan.palette.offset == 4 * consts["PLAN_PALETTE"] and P.PngPlan.palette.size == 768


def test_symbols_declared_bound_and_exported(built_lib):
    names = [n for n in _cabi.declared_symbols() if n.startswith("thmr_png_dec") or n in ("thmr_png_probe", "thmr_png_inflate", "thmr_png_inflate_window")]
    assert len(names) == 9
    for n in names:
        assert getattr(built_lib, n).argtypes is not None
    assert built_lib.thmr_png_decode_band_rows() == 64


@pytest.mark.parametrize("ctype,depth", K.KINDS)
def test_every_kind_and_size_equals_the_reference(ctype, depth, P):
    for k, (h, w) in enumerate([(1, 1), (1, 9), (9, 1), (5, 7), (150, 200)]):
        for f in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], 4, 3):
            data, rgb, _ = K.case(h, w, ctype, depth, f, seed=10 * k + depth, smooth=(h > 9), ancillary=(k == 3), idat=1 + k % 3,
                                  trns=(b"\x00\x07" if (ctype, k) == (0, 3) else bytes(range(9)) if (ctype, k) == (3, 3) else None))
            info = P.probe(data)
            assert (info["height"], info["width"], info["bit_depth"], info["colour_type"], info["bpp"]) == (h, w, depth, ctype, K.bpp_of(ctype, depth))
            check(P, data, rgb, ctype, depth, (h, w, f))


def test_every_filter_in_row_0_and_every_ordered_pair_of_filters(P):
    pairs = K.all_pairs()
    assert len(pairs) == 26 and {(int(a), int(b)) for a, b in zip(pairs[:-1], pairs[1:])} == {(a, b) for a in range(5) for b in range(5)}
    for ctype, depth in K.KINDS:
        data, rgb, _ = K.case(26, 11, ctype, depth, pairs, seed=3, smooth=False)
        check(P, data, rgb, ctype, depth, "pairs")
        for f0 in range(5):
            data, rgb, _ = K.case(3, 6, ctype, depth, [f0, 4, 3], seed=f0, smooth=False)
            check(P, data, rgb, ctype, depth, ("row 0", f0))


def test_constructed_arithmetic_cases(P):
    # Avg with a = b = 255: (a + b) >> 1 needs 9 bits; an 8-bit sum would give 127
    raw = np.full((2, 4), 255, np.uint8)
    data = K.write_png(raw, [0, 3], 0, 8)
    assert np.array_equal(P.decode_host(data)[:, :, 0], raw)
    assert K.residuals(raw, [0, 3], 1)[1, 2] == 0           # 255 - ((255 + 255) >> 1)
    # Paeth ties: pa == pb picks a, pb == pc (pa larger) picks b, all equal picks a.  Rows: c b / a x.
    for (c, b, a), want in (((10, 20, 20), 20), ((5, 5, 9), 9), ((4, 10, 7), 10), ((7, 7, 7), 7), ((0, 255, 255), 255), ((200, 100, 50), 50)):
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        pred = a if (pa <= pb and pa <= pc) else b if pb <= pc else c
        for x in (0, 1, 200, 255):
            raw = np.array([[c, b], [a, x]], np.uint8)
            stream = K.residuals(raw, [0, 4], 1)
            assert stream[1, 2] == (x - pred) & 255
            data = K.write_png(raw, [0, 4], 0, 8)
            assert np.array_equal(P.decode_host(data)[:, :, 0], raw), (c, b, a, x)
    # wrap-around sums: residuals chosen freely, the samples follow mod 256
    rng = np.random.default_rng(4)
    for f in range(5):
        raw = rng.integers(200, 256, (6, 9), dtype=np.uint8)
        raw[::2] = rng.integers(0, 40, (3, 9), dtype=np.uint8)
        data = K.write_png(raw, [f] * 6, 2, 8)
        assert np.array_equal(P.decode_host(data, bgr=False).reshape(6, 9), raw), f


def test_files_written_by_pillow_and_by_this_project(P):
    from PIL import Image
    rng = np.random.default_rng(8)
    y, x = np.mgrid[0:90, 0:120]
    img = np.stack([(2 * x + y) & 255, (x * y // 16) & 255, (3 * y) & 255], axis=2).astype(np.uint8) + rng.integers(0, 4, (90, 120, 3), dtype=np.uint8)
    for kw in ({"compress_level": 1}, {"compress_level": 6}, {"compress_level": 9}, {"optimize": True}):
        for mode, a in (("RGB", img), ("L", img[:, :, 0]), ("RGBA", np.dstack([img, img[:, :, :1]])), ("P", None)):
            b = io.BytesIO()
            im = Image.fromarray(img).quantize(40) if mode == "P" else Image.fromarray(a, mode)
            im.save(b, "PNG", **kw)
            data = b.getvalue()
            with Image.open(io.BytesIO(data)) as back:
                ref = np.asarray(back.convert("RGB"))
            assert np.array_equal(P.decode_host(data, bgr=False), ref), (kw, mode)
    for compression in ("fixed", "dynamic"):
        for a in (img, img[:, :, 0], np.dstack([img, img[:, :, :1]])):
            data = P.encode_host(a, bgr=False, compression=compression)
            want = a[:, :, :3] if a.ndim == 3 else np.repeat(a[:, :, None], 3, axis=2)
            assert np.array_equal(P.decode_host(data, bgr=False), want), compression
            assert np.array_equal(P.decode_host(data, (7, 50, 100, 33), bgr=False), want[50:83, 7:107]), compression


def test_windows_keep_what_they_need(P):
    H, W = 40, 30
    paeth = np.full(H, 4, np.uint8)
    for ctype, depth in ((2, 8), (6, 16), (3, 8)):
        bpp = K.bpp_of(ctype, depth)
        mixed = np.resize(np.array([4, 3, 1, 1, 4, 4, 0, 3, 2], np.uint8), H)
        below_none = paeth.copy()
        below_none[17] = 0
        for name, filters, win, row0 in (("1x1 odd", mixed, (7, 13, 1, 1), None), ("right and bottom edge", mixed, (W - 5, H - 6, 5, 6), None),
                                         ("right after a Sub row", mixed, (3, 12, 9, 4), None), ("all Paeth", paeth, (4, 20, 10, 5), 0),
                                         ("below a None row", below_none, (4, 25, 10, 5), 17), ("on the None row", below_none, (0, 17, W, 1), 17),
                                         ("whole", mixed, None, 0)):
            data, rgb, _ = K.case(H, W, ctype, depth, filters, seed=21, level=1, idat=3)
            x0, y0, w, h = win or (0, 0, W, H)
            it = P.inflate_window(data, win)
            if name == "right after a Sub row":          # rows 11 and 12 are Sub: the window's first row is its own restart row
                assert filters[11] == 1 and filters[12] == 1 and filters[13] > 1 and it.plan.row0 == 12 == it.window[1]
                assert P.inflate_window(data, (3, 13, 9, 4)).plan.row0 == 12           # one row lower: the Sub row above is kept
            want0 = max(r for r in range(y0 + 1) if filters[r] <= 1 or r == 0) if row0 is None else row0
            assert it.plan.row0 == want0, name
            assert it.plan.rows_kept == y0 + h - want0 and it.plan.kept_row_bytes == (x0 + w) * bpp and it.plan.rows_inflated == y0 + h
            assert it.rows.shape == (y0 + h - want0, 1 + (x0 + w) * bpp) and it.nbytes == it.rows.size
            assert np.array_equal(it.rows[:, 0], filters[want0:y0 + h]), name
            assert it.window == (x0, y0, w, h) and it.size == (H, W) and it.plan.bpp == bpp
            assert np.array_equal(P.decode_host(data, win, bgr=False), rgb[y0:y0 + h, x0:x0 + w]), name
        for win in ((5, 5, 0, 3), (5, 5, 3, 0), (0, 0, 0, 0), (W, H, 0, 0)):
            it = P.inflate_window(data, win)
            assert it.rows.size == 0 and it.plan.rows_kept == 0 and it.plan.rows_inflated == 0 and it.nbytes == 0
            assert P.decode_host(data, win).shape == (win[3], win[2], 3)
        for win in ((0, 0, W + 1, 1), (-1, 0, 2, 2), (0, H, 1, 1), (3, 3, -1, 2)):
            with pytest.raises(P.PngError, match="window"):
                P.inflate_window(data, win)
    # a size-only call inflates nothing and returns the bound
    plan, need = P.PngPlan(), ctypes.c_int64(0)
    win = (ctypes.c_int32 * 4)(4, 25, 10, 5)
    buf = np.frombuffer(data, np.uint8)
    assert _cabi.load().thmr_png_inflate_window(buf.ctypes.data, buf.size, win, None, 0, ctypes.byref(plan), need) == 0
    assert need.value == 30 * (1 + 14 * bpp) and plan.rows_inflated == 0 and plan.kept_row_bytes == 14 * bpp


def test_idat_splits_inside_a_code_and_of_one_byte(P):
    data0, rgb, raw = K.case(33, 21, 2, 8, [4, 3, 2, 1, 0], seed=2, level=9)
    f = np.resize(np.array([4, 3, 2, 1, 0], np.uint8), 33)
    z = zlib.compress(K.residuals(raw, f, 3).tobytes(), 9)
    for pieces in (1, 2, 7, len(z), [1], [2, 1, 1], [len(z) - 1], [3, 0, 0, 5]):
        data = K.write_png(raw, f, 2, 8, zstream=z, idat=pieces)
        assert np.array_equal(P.decode_host(data, bgr=False), rgb), pieces
        assert np.array_equal(P.decode_host(data, (2, 9, 11, 20), bgr=False), rgb[9:29, 2:13]), pieces


def test_the_own_inflate_equals_zlib(P):
    rng = np.random.default_rng(0)
    text = bytes(rng.integers(97, 105, 70000, dtype=np.uint8))
    noise = bytes(rng.integers(0, 256, 70000, dtype=np.uint8))
    for plain in (b"", b"a", bytes([7]) * 1000, text, noise, noise[:40000] + noise[:40000], text + noise + text):
        for level in (0, 1, 6, 9):
            z = zlib.compress(plain, level)
            assert P.inflate(z, len(plain)) == plain == zlib.decompress(z)
        c = zlib.compressobj(9, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
        z = c.compress(plain) + c.flush()
        assert P.inflate(z, len(plain)) == plain
        c = zlib.compressobj(6)          # a back-reference across a block boundary: Z_SYNC_FLUSH ends the block and keeps the history
        z = c.compress(plain[:len(plain) // 2]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(plain[len(plain) // 2:]) + c.flush()
        assert P.inflate(z, len(plain)) == plain
    # by hand: a distance-1 run of 258, the maximal distance of 32768, a back-reference across two fixed blocks, a single distance code
    w = K.Bits()
    K.fixed_block(w, [65, (258, 1), (258, 1), 66])
    z = K.zwrap(w.done(), b"A" * 517 + b"B")
    assert P.inflate(z, 518) == zlib.decompress(z) == b"A" * 517 + b"B"
    head = noise[:32768]
    w = K.Bits()
    w.bits(0, 1); w.bits(0, 2); w.bits(0, 5)                    # a stored block of 32768 bytes, not the last
    stored = w.done() + struct.pack("<HH", 32768, 32768 ^ 0xFFFF) + head
    w = K.Bits()
    K.fixed_block(w, [(258, 32768), (3, 32768), 67])
    z = K.zwrap(stored + w.done(), head + head[:261] + b"C")
    assert P.inflate(z, 40000) == zlib.decompress(z) == head + head[:261] + b"C"
    w = K.Bits()
    K.fixed_block(w, list(b"hello "), last=False)
    K.fixed_block(w, [(6, 6), (12, 3)])
    plain = b"hello hello " + b"lo lo lo lo "
    z = K.zwrap(w.done(), plain)
    assert P.inflate(z, 64) == zlib.decompress(z) == plain
    z, plain = K.single_distance_code_stream()
    assert P.inflate(z, 16) == zlib.decompress(z) == plain
    with pytest.raises(P.PngError, match="capacity"):
        P.inflate(zlib.compress(text), 100)


def _rc(lib, data, window=None):
    buf = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
    info = np.zeros(_cabi.PNG_INFO_WORDS, np.int32)
    rc = lib.thmr_png_probe(buf.ctypes.data, len(data), info.ctypes.data)
    if rc != 0:
        return rc, lib.thmr_png_decoder_last_error(None).decode()
    height, width = int(info[0]), int(info[1])
    out = np.zeros((height, width, 3), np.uint8)
    rc = lib.thmr_png_decode_host(buf.ctypes.data, len(data), None, 1, out.ctypes.data, width * 3)
    return rc, lib.thmr_png_decoder_last_error(None).decode() if rc else ""


def test_each_unsupported_kind_is_refused_by_name(P, built_lib):
    raw = np.zeros((4, 4), np.uint8)
    z = zlib.compress(bytes(20))
    body = [K.chunk(b"IDAT", z), K.chunk(b"IEND", b"")]
    for hdr, name in ((K.ihdr(4, 4, 8, 0, interlace=1), "Adam7 interlace"), (K.ihdr(4, 4, 1, 0), "bit depth 1"), (K.ihdr(4, 4, 2, 3), "bit depth 2"),
                      (K.ihdr(4, 4, 4, 0), "bit depth 4"), (K.ihdr(32768, 4, 8, 0), "a side above 32767"), (K.ihdr(4, 40000, 8, 2), "a side above 32767"),
                      (K.ihdr(4, 4, 8, 0, compression=1), "compression method 1"), (K.ihdr(4, 4, 8, 0, filt=1), "filter method 1")):
        data = b"".join([K.SIGNATURE, hdr] + body)
        rc, msg = _rc(built_lib, data)
        assert rc == _cabi.ERR_UNSUPPORTED and name in msg, (name, msg)
        with pytest.raises(P.PngUnsupported, match=name):
            P.probe(data)
        with pytest.raises(P.PngUnsupported, match=name):
            P.inflate_window(data)
    assert np.array_equal(P.decode_host(K.write_png(raw, [0] * 4, 0, 8))[:, :, 0], raw)


def malformed_files():
    raw = K.samples(6, 5, 2, 8, 1)
    f = np.array([0, 1, 2, 3, 4, 4], np.uint8)
    good = K.write_png(raw, f, 2, 8)
    stream = K.residuals(raw, f, 3).tobytes()
    idat_at = good.index(b"IDAT") - 4
    pal_raw = (K.samples(4, 4, 3, 8, 2) % 7).astype(np.uint8)
    pal = K.write_png(pal_raw, [0] * 4, 3, 8, plte=K.palette(7))
    pal_at = pal.index(b"PLTE") - 4
    bad_filter = bytearray(stream)
    bad_filter[16 * 2] = 5

    def with_stream(z):
        return K.write_png(raw, f, 2, 8, zstream=z)

    def deflate_of(w):
        return with_stream(K.zwrap(w.done()))

    w1 = K.Bits(); w1.bits(1, 1); w1.bits(0, 2); w1.bits(0, 5)
    stored_bad = with_stream(b"\x78\x01" + w1.done() + struct.pack("<HH", 96, 96) + stream + struct.pack(">I", zlib.adler32(stream)))
    w2 = K.Bits(); K.fixed_block(w2, [1, 2, (3, 3)])
    w3 = K.Bits(); K.dynamic_header(w3, {16: 1, 17: 1, 18: 1, 0: 1}, [], 257, 1)
    w4 = K.Bits(); K.dynamic_header(w4, {0: 1}, [], 257, 1)
    over = [0] * 258; over[0] = over[1] = over[256] = 1
    w5 = K.Bits(); K.dynamic_header(w5, {0: 1, 1: 1}, over, 257, 1)
    inc = [0] * 258; inc[0] = inc[256] = 2
    w6 = K.Bits(); K.dynamic_header(w6, {0: 1, 2: 1}, inc, 257, 1)
    dinc = [0] * 259; dinc[0] = dinc[256] = 1; dinc[257] = dinc[258] = 2
    w7 = K.Bits(); K.dynamic_header(w7, {0: 2, 1: 2, 2: 1}, dinc, 257, 2)
    w8 = K.Bits(); w8.bits(1, 1); w8.bits(3, 2)
    z = zlib.compress(stream, 6)
    return {
        "bad signature": b"\x89PNG\r\n\x1a\x0b" + good[8:],
        "truncated chunk": good[:idat_at + 20],
        "truncated length": good[:idat_at + 3],
        "a length beyond the file": good[:idat_at] + struct.pack(">I", 1 << 20) + good[idat_at + 4:],
        "wrong CRC on IHDR": good[:29] + bytes([good[29] ^ 1]) + good[30:],
        "wrong CRC on PLTE": pal[:pal_at + 9] + bytes([pal[pal_at + 9] ^ 1]) + pal[pal_at + 10:],
        "wrong CRC on IDAT": good[:idat_at + 12] + bytes([good[idat_at + 12] ^ 0x10]) + good[idat_at + 13:],
        "IDAT before IHDR": K.SIGNATURE + good[idat_at:-12] + good[8:33] + good[-12:],
        "PLTE missing": pal[:pal_at] + pal[pal_at + 12 + 21:],
        "palette index beyond PLTE": K.write_png(pal_raw, [0] * 4, 3, 8, plte=K.palette(6)),
        "colour type 5": K.SIGNATURE + K.ihdr(5, 6, 8, 5) + good[33:],
        "16-bit palette": K.SIGNATURE + K.ihdr(5, 6, 16, 3) + good[33:],
        "zero width": K.SIGNATURE + K.ihdr(0, 6, 8, 2) + good[33:],
        "no IDAT": good[:idat_at] + good[-12:],
        "IDAT not consecutive": K.SIGNATURE + good[8:33] + K.chunk(b"IDAT", z[:9]) + K.chunk(b"tEXt", b"k\x00v") + K.chunk(b"IDAT", z[9:]) + good[-12:],
        "zlib method 7": with_stream(b"\x77\x09" + z[2:]),
        "zlib window 64K": with_stream(b"\x88\x1c" + z[2:]),
        "zlib check bits": with_stream(b"\x78\x9d" + z[2:]),
        "zlib preset dictionary": with_stream(b"\x78\xbb" + z[2:]),
        "stored length check": stored_bad,
        "distance before the first byte": deflate_of(w2),
        "over-subscribed code-length code": deflate_of(w3),
        "incomplete code-length code": deflate_of(w4),
        "over-subscribed literal code": deflate_of(w5),
        "incomplete literal code": deflate_of(w6),
        "incomplete distance code of two bits": deflate_of(w7),
        "block type 3": deflate_of(w8),
        "stream ends early": with_stream(z[:len(z) // 2]),
        "too few rows": with_stream(zlib.compress(stream[:16 * 4])),
        "too many rows": with_stream(zlib.compress(stream + stream[:16])),
        "filter byte 5": with_stream(zlib.compress(bytes(bad_filter))),
        "wrong Adler-32": with_stream(z[:-1] + bytes([z[-1] ^ 1])),
    }


def test_each_malformed_kind_is_invalid(P, built_lib):
    files = malformed_files()
    for name, data in files.items():
        rc, msg = _rc(built_lib, data)
        assert rc == _cabi.ERR_INVALID and msg, (name, rc, msg)
    for name in ("wrong CRC on IHDR", "wrong CRC on PLTE", "wrong CRC on IDAT", "stored length check", "distance", "Adler-32", "filter byte 5"):
        key = next(k for k in files if name in k)
        assert name.split()[-1].lower() in _rc(built_lib, files[key])[1].lower(), key
    # a window that ends above the last row never reads the Adler-32, nor rows it does not need
    assert P.decode_host(files["wrong Adler-32"], (0, 0, 5, 5)).shape == (5, 5, 3)
    assert P.inflate_window(files["too many rows"], (0, 0, 5, 5)).plan.rows_inflated == 5
    with pytest.raises(P.PngError):
        P.decode_host(files["wrong Adler-32"])
    # an IDAT that the window does not reach is not read, so its CRC is not checked
    raw = K.samples(64, 64, 2, 8, 9, smooth=False)
    good = K.write_png(raw, [0] * 64, 2, 8, level=0, idat=4)
    last = good.rindex(b"IDAT")
    bad = good[:last + 10] + bytes([good[last + 10] ^ 1]) + good[last + 11:]
    assert np.array_equal(P.decode_host(bad, (0, 0, 64, 8), bgr=False).reshape(8, -1), raw[:8])
    with pytest.raises(P.PngError, match="CRC"):
        P.decode_host(bad)


def test_prefixes_and_byte_corruptions_never_crash(P, built_lib):
    lib = built_lib
    files = [K.case(5, 7, ct, d, [4, 3, 2, 1, 0], seed=1, idat=2, ancillary=True)[0] for ct, d in ((2, 8), (3, 8), (4, 16))]
    files.append(K.case(40, 30, 6, 8, [4, 1, 3], seed=2, level=9)[0])
    n = 0
    for data in files:
        for cut in range(len(data)):
            rc, _ = _rc(lib, data[:cut])
            assert rc <= 0
            n += 1
        for at in range(min(700, len(data))):
            for v in (0x00, 0xFF):
                if data[at] != v:
                    rc, _ = _rc(lib, data[:at] + bytes([v]) + data[at + 1:])
                    assert rc <= 0
                    n += 1
    # CRCs stop most of those early: the raw zlib streams corrupted the same way go straight to the inflate
    rng = np.random.default_rng(6)
    plains = [bytes(rng.integers(97, 101, 3000, dtype=np.uint8)), bytes(rng.integers(0, 256, 600, dtype=np.uint8)) * 3]
    out = np.zeros(16384, np.uint8)
    written = ctypes.c_int64(0)
    for plain in plains:
        for level in (0, 1, 9):
            z = zlib.compress(plain, level)
            variants = [z[:cut] for cut in range(len(z))]
            variants += [z[:at] + bytes([v]) + z[at + 1:] for at in range(min(700, len(z))) for v in (0x00, 0xFF) if z[at] != v]
            variants += [z[:at] + bytes([z[at] ^ (1 << (at % 8))]) + z[at + 1:] for at in range(min(700, len(z)))]
            for v in variants:
                buf = np.frombuffer(v, np.uint8) if len(v) else np.zeros(1, np.uint8)
                rc = lib.thmr_png_inflate(buf.ctypes.data, len(v), out.ctypes.data, out.size, written)
                assert rc <= 0 and 0 <= written.value <= out.size
                if rc == 0:
                    assert out[:written.value].tobytes() == zlib.decompress(v)
                n += 1
    assert n > 10000


class RecordingCropper:
    """Stand-in for preprocess.Cropper on the host, as tests/test_jpeg_host.py uses one."""

    def __init__(self):
        import torch
        self.device = torch.device("cpu")


def test_datasets_device_png_mode_on_the_host(tmp_path, built_lib):
    from PIL import Image
    from tokenhmr_amd import jpeg as J, png as P, preprocess as PP
    from tokenhmr_amd.datasets import DECODE_MODES
    assert DECODE_MODES == ("host", "device", "device+png")
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    fr = F.frames()
    Image.fromarray(fr["f0.jpg"][:, :, ::-1].copy()).save(str(imgs / "f0.jpg"), format="PNG")
    Image.fromarray(fr["f1.jpg"][:, :, ::-1].copy()).save(str(imgs / "f1.jpg"), quality=90)
    with open(str(imgs / "f2.jpg"), "wb") as f:           # an interlaced PNG by hand: the header says Adam7, which is all the probe reads
        f.write(K.SIGNATURE + K.ihdr(64, 48, 8, 2, interlace=1) + K.chunk(b"IDAT", zlib.compress(b"")) + K.chunk(b"IEND", b""))
    got = {}
    for mode in ("device+png", "device"):
        ds = F.make_dataset("image", tmp_path, "cpu", cropper=RecordingCropper(), decode=mode, img_dir=str(imgs))
        names = [os.path.basename(n) for n in ds._names(range(len(ds)))[1]]
        assert ds.decode == mode and ds.decode_stats == {"device": 0, "fallback": 0, "coef_bytes": 0}
        assert ds.png_stats == {"device": 0, "fallback": 0, "stream_bytes": 0}
        k0, k1, k2 = 5, names.index("f1.jpg"), names.index("f2.jpg")
        assert names[k0] == "f0.jpg"
        got[mode] = ds, k0, k1, k2
    ds, k0, k1, k2 = got["device+png"]
    it = ds.read_item(k0)
    assert isinstance(it, P.PlannedPng) and it.size == (48, 64)
    _, trans, _ = ds.host_batch([k0], [it.size])
    win = tuple(PP.source_window(trans[0], 256, 48, 64, 0.0, 3.0))
    assert it.window == win == ds._item_window(k0, 48, 64)
    x0, y0, w, h = win
    with open(str(imgs / "f0.jpg"), "rb") as f:
        data = f.read()
    assert np.array_equal(P.decode_host(data, win), fr["f0.jpg"][y0:y0 + h, x0:x0 + w])
    assert it.plan.rows_inflated == y0 + h and it.plan.kept_row_bytes == (x0 + w) * 3
    empty = ds.read_item(3)                     # this item's crop lies outside its frame: nothing is inflated
    assert isinstance(empty, P.PlannedPng) and empty.window == (0, 0, 0, 0) and empty.nbytes == 0
    assert isinstance(ds.read_item(k1), J.PlannedItem)
    ds._imread = lambda path: fr["f2.jpg"]      # the interlaced file falls back to imread, that item alone
    f2 = ds.read_item(k2)
    assert isinstance(f2, np.ndarray) and k2 in ds._png_fallbacks and k0 not in ds._png_fallbacks
    with open(str(imgs / "f0.jpg"), "wb") as f:
        f.write(data[:len(data) // 2])
    with pytest.raises(IOError, match="Fail to read"):
        ds.read_item(k0)
    # "device" on the same files behaves as today: a PNG goes to imread (here: the truncated one is unreadable, the other decodes)
    ds, k0, k1, k2 = got["device"]
    ds._imread = lambda path: fr["f2.jpg"] if path.endswith("f2.jpg") else None
    assert isinstance(ds.read_item(k2), np.ndarray) and isinstance(ds.read_item(k1), J.PlannedItem)
    with pytest.raises(IOError, match="Fail to read"):
        ds.read_item(k0)
    assert not ds._png_fallbacks and ds._png is None


def test_batch_entry_refuses_before_any_hip_call(P, built_lib):
    """Every argument is checked before the handle, and the handle before any HIP call: with a null handle a well-formed table gets as
    far as 'null handle', on a machine without a device."""
    lib = built_lib
    data, _, _ = K.case(12, 9, 2, 8, [1, 4, 3], seed=1)
    whole, part = P.inflate_window(data), P.inflate_window(data, (2, 5, 4, 3))

    def call(p, win=None, stride=None, out=4096, rows=True, plan=True, n=1, table=True):
        win = win or p.window
        tables = [(ctypes.c_void_p * 1)(p.rows.ctypes.data if rows else None), (ctypes.c_void_p * 1)(ctypes.addressof(p.plan) if plan else None),
                  (ctypes.c_int32 * 4)(*win), (ctypes.c_void_p * 1)(out), (ctypes.c_int64 * 1)(win[2] * 3 if stride is None else stride)]
        if table is not True:
            tables[table] = None
        rc = lib.thmr_png_decode_batch(None, *tables, n, 1, None)
        return rc, lib.thmr_png_decoder_last_error(None).decode()

    assert call(whole) == (_cabi.ERR_INVALID, "null handle")
    assert call(part) == (_cabi.ERR_INVALID, "null handle")
    assert call(whole, win=(1, 3, 5, 4))[1] == "null handle"                  # a smaller window inside what was kept
    assert call(part, win=(0, 0, 0, 0)) == (_cabi.ERR_INVALID, "null handle")
    for kw, text in (({"n": 0}, "n must be"), ({"table": 0}, "null item table"), ({"table": 3}, "null item table"), ({"table": 4}, "null item table"), ({"plan": False}, "item 0: null plan"),
                     ({"rows": False}, "item 0: null rows"), ({"out": None}, "null out_dev"), ({"stride": 5}, "row_stride"),
                     ({"win": (0, 0, 10, 12)}, "inside the frame"), ({"win": (-1, 0, 3, 3)}, "inside the frame")):
        rc, msg = call(whole, **kw)
        assert rc == _cabi.ERR_INVALID and text in msg, (kw, msg)
    for win in ((2, 2, 4, 3), (2, 5, 5, 3), (2, 5, 4, 4)):                        # above, right of and below what the plan kept
        rc, msg = call(part, win=win)
        assert rc == _cabi.ERR_INVALID and "outside what the plan kept" in msg, (win, msg)
    assert part.plan.row0 == 3 and part.rows[0, 0] == 1
    bad = P.inflate_window(data, (2, 5, 4, 3))
    bad.rows[1, 0] = 7
    assert "filter byte 7" in call(bad)[1]
    bad.rows[1, 0], bad.rows[0, 0] = 4, 4                                        # the first kept row now needs a row above it
    assert "not kept" in call(bad)[1]
    bad = P.inflate_window(data)
    bad.plan.bpp = 4
    assert "not one thmr_png_inflate_window produces" in call(bad)[1]
    bad.plan.bpp, bad.plan.kept_row_bytes = 3, 28
    assert "kept rows lie outside" in call(bad)[1]
    with pytest.raises(RuntimeError, match="needs a GPU"):
        P.PNGDecoder("cpu")
