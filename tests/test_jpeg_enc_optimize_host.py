"""The optimised mode of the JPEG encoder on the CPU (thmr_jpeg_encode_host_flags with THMR_JPEG_OPTIMIZE: Huffman tables from the
image's own statistics, csrc/jpegenc_math.h) against the files Pillow / libjpeg-turbo wrote with optimize=True — the stored ones of
tests/golden/jpeg_enc_opt_small.npz and, where the installed Pillow has libjpeg-turbo, live ones — WHOLE file, byte for byte; the table
routine thmr_jpeg_optimal_table on its own (its invariants, the DHT payloads of Pillow's files, the 16-bit limit); the unchanged default
bytes; every refusal by name; the mode's bound; and every file read back by Pillow with the default file's pixels.
tests/test_gpu_jpeg_enc_optimize.py holds the device against encode_host(optimize=True) byte for byte."""
import ctypes as C
import io
from fractions import Fraction

import numpy as np
import pytest

import _jpeg_enc_cases as K
import _jpeg_enc_opt_cases as KO


@pytest.fixture(scope="module")
def J(built_lib):
    from tokenhmr_amd import jpeg
    return jpeg


def pillow():
    Image = pytest.importorskip("PIL.Image")
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("Pillow without libjpeg-turbo: another libjpeg may round differently")
    return Image


def pillow_file(Image, img, quality, subsampling, optimize=True):
    buf = io.BytesIO()
    kw = {} if img.ndim == 2 else {"subsampling": K.PIL_SUBSAMPLING[subsampling]}
    Image.fromarray(np.ascontiguousarray(img)).save(buf, "JPEG", quality=quality, optimize=optimize, **kw)
    return buf.getvalue()


def check_table(freq, bits, huffval):
    """What every table of the routine satisfies for the frequencies it was made from."""
    used = [s for s in range(256) if freq[s] > 0]
    counts = [int(b) for b in bits[1:]]
    assert sum(counts) == len(used) == len(huffval) and sorted(int(s) for s in huffval) == used
    assert all(c >= 0 for c in counts) and 1 <= max(k + 1 for k, c in enumerate(counts) if c) <= 16
    # Kraft, with the all-ones code of the longest length reserved: it is the code the pseudo-symbol held
    longest = max(k + 1 for k, c in enumerate(counts) if c)
    assert sum(Fraction(c, 2 ** (k + 1)) for k, c in enumerate(counts)) + Fraction(1, 2 ** longest) <= 1
    assert bits[0] >= longest and (bits[0] == longest or bits[0] > 16)


def test_symbols_declared_bound_and_exported(built_lib):
    from tokenhmr_amd import _cabi
    assert _cabi.ABI_VERSION == 5 and built_lib.thmr_abi_version() == 5         # new symbols only
    names = {"thmr_jpeg_encode_bound_flags", "thmr_jpeg_encode_host_flags", "thmr_jpeg_encode_batch_flags", "thmr_jpeg_optimal_table",
             "thmr_jpeg_histogram_host"}
    assert names <= set(_cabi.declared_symbols())
    for exp in (False, True):
        lib = _cabi.load(exp=exp)
        for name in names:
            assert hasattr(lib, name) and isinstance(getattr(lib, name).argtypes, list), (exp, name)
    assert built_lib.thmr_jpeg_encode_batch_flags.argtypes == [C.c_void_p, C.POINTER(_cabi.PngItem), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    assert built_lib.thmr_jpeg_optimal_table.argtypes == [C.c_void_p] * 4
    assert _cabi.JPEG_OPTIMIZE == 1 and len(_cabi.STRUCTS) == 21


def test_golden_covers_what_it_should():
    table, arrays = KO.golden()
    default, _ = K.golden()
    assert table == default and len(arrays["versions"]) == 2          # the same cases and inputs as the default-mode archive
    assert {(c["width"], c["height"]) for c in table.values()} == set(K.SIZES)
    for mode in ("444", "420", "grey"):
        assert len({c["quality"] for c in table.values() if c["mode"] == mode}) >= 3
    for name in table:
        opt, plain = KO.golden_file(name), K.golden_file(name)
        assert KO.markers(opt) == KO.markers(plain) and len(opt) < len(plain), name


@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_equals_the_stored_pillow_file(J, size):
    table, _ = KO.golden()
    names = [n for n, c in table.items() if (c["width"], c["height"]) == size]
    assert len(names) >= 15
    for name in names:
        c = table[name]
        got = J.encode_host(K.golden_input(name), quality=c["quality"], subsampling=K.SUBSAMPLING[c["mode"]], optimize=True, bgr=False)
        want = KO.golden_file(name)
        assert got == want, (name, K.first_difference(got, want))


@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_equals_the_installed_pillow(J, size):
    Image = pillow()
    w, h = size
    for kind in ("noise", "smooth", "checker"):
        rgb = K.picture(kind, w, h)
        for q in (1, 50, 95, 100):
            for img, sub in ((rgb, "4:4:4"), (rgb, "4:2:0"), (rgb[..., 1], "4:2:0")):
                got, want = J.encode_host(img, quality=q, subsampling=sub, optimize=True, bgr=False), pillow_file(Image, img, q, sub)
                assert got == want, (kind, q, sub, img.ndim, K.first_difference(got, want))


def test_the_smallest_cases_that_can_go_wrong(J):
    table, _ = KO.golden()
    # 1 x 1 and the flat 8 x 8: a table holds one real symbol and the pseudo-symbol, so the one code has length 1.  (A DC table of a
    # colour image may hold two — Cb's and Cr's categories, or in 4:2:0 the real luma block's and the dummies' 0: lengths 1 and 2.)
    for name in [n for n, c in table.items() if (c["width"], c["height"]) == (1, 1) or ((c["width"], c["height"]) == (8, 8) and c["kind"] in ("black", "white"))]:
        data = J.encode_host(K.golden_input(name), quality=table[name]["quality"], subsampling=K.SUBSAMPLING[table[name]["mode"]], optimize=True, bgr=False)
        assert data == KO.golden_file(name), name
        segs = KO.dht_segments(data)
        assert [t for t, _, _ in segs] == ([0x00, 0x10] if table[name]["mode"] == "grey" else [0x00, 0x10, 0x01, 0x11]), name
        hist = J.symbol_histogram(K.golden_input(name), quality=table[name]["quality"], subsampling=K.SUBSAMPLING[table[name]["mode"]], bgr=False)
        for (t, counts, symbols), slot in zip(segs, range(4)):
            used = int((hist[slot] > 0).sum())
            assert used == len(symbols) and used == 1 or (used == 2 and slot in (0, 2) and table[name]["mode"] != "grey"), (name, t)
            assert counts == ([1] + [0] * 15 if used == 1 else [1, 1] + [0] * 14), (name, t)
        if table[name]["mode"] == "grey" or (table[name]["mode"] == "444" and table[name]["kind"] in ("black", "white")):
            assert all(len(symbols) == 1 for _, _, symbols in segs), name
    # 17 x 23 in 4:2:0: 2 x 2 MCUs, 7 of whose 16 luma blocks are dummies (3 x 3 are real).  They are coded, so they are counted: DC
    # category 0 and EOB each at least 7 times in table 0, and the histogram holds one DC symbol per block of the scan
    img = K.picture("noise", 17, 23)
    hist = J.symbol_histogram(img, quality=95, subsampling="4:2:0", bgr=False)
    assert hist.shape == (4, 256) and hist[0].sum() == 16 and hist[2].sum() == 8 and hist[0][0] >= 7 and hist[1][0] >= 7
    assert not hist[0][12:].any() and not hist[2][12:].any()
    # a grey image: two tables only
    grey = J.symbol_histogram(img[..., 1], quality=95, bgr=False)
    assert grey[0].sum() == 3 * 3 and not grey[2:].any()
    assert [t for t, _, _ in KO.dht_segments(J.encode_host(img[..., 1], quality=95, optimize=True))] == [0x00, 0x10]


def test_code_lengths_limited_to_16_bits(J):
    """The seeded 256 x 256 image of _jpeg_enc_opt_cases.long_code_image: the table routine itself reports (bits[0]) that the unlimited
    code of its luma AC statistics is longer than 16 bits, so libjpeg's adjustment ran; the file still equals Pillow's."""
    img = KO.long_code_image()
    hist = J.symbol_histogram(img, quality=95, subsampling="4:2:0", bgr=False)
    bits, huffval = J.optimal_table(hist[1])
    assert bits[0] > 16 and bits[16] > 0, bits
    check_table(hist[1], bits, huffval)
    data = J.encode_host(img, quality=95, subsampling="4:2:0", optimize=True, bgr=False)
    assert KO.dht_segments(data)[1] == (0x10, [int(b) for b in bits[1:]], [int(s) for s in huffval])
    want = pillow_file(pillow(), img, 95, "4:2:0")
    assert data == want, K.first_difference(data, want)


def test_optimal_table_alone(J, built_lib):
    from tokenhmr_amd import _cabi
    # powers of two: every merge joins the tree so far (1 + 1 + 2 + ... + 2^(k-1) = 2^k) with the next symbol, so the unlimited code
    # is as deep as the alphabet is large, far beyond 16; and Fibonacci numbers, the slowest-growing frequencies of a deep code
    freq = np.zeros(256, np.int32)
    freq[3:28] = 2 ** np.arange(25)
    bits, huffval = J.optimal_table(freq)
    assert bits[0] == 25 and len(huffval) == 25 and bits[16] > 0
    check_table(freq, bits, huffval)
    assert list(huffval[:3]) == [27, 26, 25]            # the most frequent symbols keep the shortest codes
    fib = [1, 2]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    freq = np.zeros(256, np.int32)
    freq[100:130] = fib
    bits, huffval = J.optimal_table(freq)
    assert bits[0] > 16
    check_table(freq, bits, huffval)
    # one symbol: a code of length 1; two symbols of one frequency: lengths 1 and 2 (the pseudo-symbol takes the 11), the larger
    # symbol, which is merged first, the longer code
    one = np.zeros(256, np.int32)
    one[0xF0] = 7
    bits, huffval = J.optimal_table(one)
    assert list(bits) == [1, 1] + [0] * 15 and list(huffval) == [0xF0]
    one[0x21] = 7
    bits, huffval = J.optimal_table(one)
    assert list(bits) == [2, 1, 1] + [0] * 14 and list(huffval) == [0x21, 0xF0]
    # flat statistics over all 256 symbols: 256 codes of 8 bits would leave no room for the reserved one
    bits, huffval = J.optimal_table(np.full(256, 5, np.int32))
    check_table(np.full(256, 5), bits, huffval)
    assert bits[0] == 9 and bits[9] >= 1 and list(huffval[:int(bits[8])]) == sorted(huffval[:int(bits[8])])
    rng = np.random.default_rng(11)
    for k in range(20):
        freq = (rng.pareto(0.6, 256) * (rng.random(256) < (k + 1) / 20)).astype(np.int64).clip(0, 10 ** 6).astype(np.int32)
        if not freq.any():
            freq[k] = 1
        check_table(freq, *J.optimal_table(freq))
    # the refusals of the C entry point
    f = lambda a, b=np.zeros(17, np.uint8), h=np.zeros(256, np.uint8), n=C.c_int32(): built_lib.thmr_jpeg_optimal_table(
        None if a is None else a.ctypes.data, None if b is None else b.ctypes.data, None if h is None else h.ctypes.data, None if n is None else C.addressof(n))
    last = built_lib.thmr_jpeg_encoder_last_error
    ok = np.ones(256, np.int32)
    assert f(ok) == 0
    assert f(None) == _cabi.ERR_INVALID and f(ok, None) == _cabi.ERR_INVALID and f(ok, h=None) == _cabi.ERR_INVALID and f(ok, n=None) == _cabi.ERR_INVALID
    assert f(np.zeros(256, np.int32)) == _cabi.ERR_INVALID and b"zero" in last(None)
    neg = ok.copy()
    neg[200] = -1
    assert f(neg) == _cabi.ERR_INVALID and b"200" in last(None)
    with pytest.raises(J.JpegError, match="zero"):
        J.optimal_table(np.zeros(256, np.int32))


def test_the_routine_reproduces_pillows_dht_payloads(J):
    """The tables of Pillow's stored files, parsed out of their DHT segments, from the histograms of the same inputs."""
    table, _ = KO.golden()
    seen = 0
    for name, c in table.items():
        hist = J.symbol_histogram(K.golden_input(name), quality=c["quality"], subsampling=K.SUBSAMPLING[c["mode"]], bgr=False)
        segs = KO.dht_segments(KO.golden_file(name))
        assert len(segs) == (2 if c["mode"] == "grey" else 4), name
        for (tc, counts, symbols), slot in zip(segs, (0, 1, 2, 3)):
            assert tc == ((slot & 1) << 4 | slot >> 1), name
            bits, huffval = J.optimal_table(hist[slot])
            check_table(hist[slot], bits, huffval)
            assert (counts, symbols) == ([int(b) for b in bits[1:]], [int(s) for s in huffval]), (name, slot)
            seen += 1
    assert seen >= 400


def test_default_bytes_and_params(J, built_lib, tmp_path):
    from tokenhmr_amd import _cabi
    table, _ = K.golden()
    for name in [n for n, c in table.items() if (c["width"], c["height"]) in ((17, 23), (1, 1), (100, 75))]:
        c = table[name]
        img = K.golden_input(name)
        kw = dict(quality=c["quality"], subsampling=K.SUBSAMPLING[c["mode"]], bgr=False)
        assert J.encode_host(img, optimize=False, **kw) == J.encode_host(img, **kw) == J.encode_host(img, flags=0, **kw) == K.golden_file(name), name
    # the two C entry points of the host encode side by side
    img = K.picture("noise", 17, 23)
    item = _cabi.PngItem()
    J._fill(item, img, 1.0, "nearest", True)
    out = np.zeros(J.encode_bound(17, 23, 3, optimize=True), np.uint8)
    item.pixels, item.out, item.capacity = img.ctypes.data, out.ctypes.data, out.size
    assert built_lib.thmr_jpeg_encode_host(C.byref(item), 90, _cabi.JPEG_420) == 0
    old = out[:item.written].tobytes()
    assert built_lib.thmr_jpeg_encode_host_flags(C.byref(item), 90, _cabi.JPEG_420, 0) == 0 and out[:item.written].tobytes() == old
    assert built_lib.thmr_jpeg_encode_host_flags(C.byref(item), 90, _cabi.JPEG_420, _cabi.JPEG_OPTIMIZE) == 0
    assert out[:item.written].tobytes() == J.encode_host(img, quality=90, optimize=True) != old
    assert J.encode_bound(17, 23, 3) == built_lib.thmr_jpeg_encode_bound_flags(17, 23, 3, _cabi.JPEG_420, 0)
    # cv2's params
    assert (J.IMWRITE_JPEG_QUALITY, J.IMWRITE_JPEG_OPTIMIZE) == (1, 3)
    assert J._params([3, 1], 95, False) == (95, True) and J._params([1, 40, 3, 1], 95, False) == (40, True)
    assert J._params([3, 0], 95, True) == (95, False) and J._params([3, 7, 1, 60], 95, False) == (60, True) and J._params(None, 80, True) == (80, True)
    assert J._params_quality([1, 40, 3, 1], 95) == 40
    with pytest.raises(ValueError, match="pairs"):
        J._params([3], 95, False)
    for params, flag in (([3, 1, 2, 1], 2), ([16, 3, 3, 1], 16), ([3, 1, 4, 0], 4), ([0, 1], 0)):
        with pytest.raises(ValueError, match=f"flag {flag} "):
            J.imwrite(str(tmp_path / "a.jpg"), img, params)
    assert not list(tmp_path.iterdir())


def test_refusals_by_name(J, built_lib):
    from tokenhmr_amd import _cabi
    img = K.picture("noise", 5, 4)
    with pytest.raises(J.JpegUnsupported, match="4:2:2"):
        J.encode_host(img, subsampling="4:2:2", optimize=True)
    with pytest.raises(J.JpegUnsupported, match="2 channels"):
        J.encode_host(np.zeros((4, 5, 2), np.uint8), optimize=True)
    with pytest.raises(J.JpegError, match="quality must be 1 ... 100"):
        J.encode_host(img, quality=0, optimize=True)
    for bad in (1, "yes", None, 2):
        with pytest.raises(ValueError, match="optimize"):
            J.encode_host(img, optimize=bad)
    for flags in (2, 3, 4, -1, 1 << 30):
        with pytest.raises(J.JpegError, match="flag"):
            J.encode_host(img, flags=flags)
        assert built_lib.thmr_jpeg_encode_bound_flags(5, 4, 3, _cabi.JPEG_420, flags) == 0
    item = (_cabi.PngItem * 3)()
    out = np.empty(J.encode_bound(5, 4, 3, optimize=True), np.uint8)
    q, s = (C.c_int32 * 3)(95, 95, 95), (C.c_int32 * 3)(_cabi.JPEG_420, _cabi.JPEG_420, _cabi.JPEG_420)
    fl = (C.c_int32 * 3)(0, _cabi.JPEG_OPTIMIZE, _cabi.JPEG_OPTIMIZE)
    for k in range(3):
        J._fill(item[k], img, 1.0, "nearest", True)
        item[k].pixels, item[k].out, item[k].capacity = img.ctypes.data, out.ctypes.data, out.size
    batch, last = built_lib.thmr_jpeg_encode_batch_flags, built_lib.thmr_jpeg_encoder_last_error
    fl[2] = 2
    assert batch(None, item, q, s, fl, 3, None) == _cabi.ERR_INVALID and b"item 2" in last(None) and b"flag" in last(None)
    fl[2] = _cabi.JPEG_OPTIMIZE | 4
    assert batch(None, item, q, s, fl, 3, None) == _cabi.ERR_INVALID and b"item 2" in last(None) and b"flag" in last(None)
    fl[2], s[2] = _cabi.JPEG_OPTIMIZE, _cabi.JPEG_422
    assert batch(None, item, q, s, fl, 3, None) == _cabi.ERR_UNSUPPORTED and b"item 2" in last(None) and b"4:2:2" in last(None)
    s[2], item[1].compression = _cabi.JPEG_420, 1
    assert batch(None, item, q, s, fl, 3, None) == _cabi.ERR_INVALID and b"item 1" in last(None) and b"compression" in last(None)
    item[1].compression, item[1].capacity = 0, out.size - 1
    assert batch(None, item, q, s, fl, 3, None) == _cabi.ERR_INVALID and b"item 1" in last(None) and b"thmr_jpeg_encode_bound_flags" in last(None)
    item[1].capacity = out.size
    assert batch(None, item, q, s, None, 3, None) == _cabi.ERR_INVALID and b"null flags" in last(None)
    # every item is fine: only now is the handle looked at.  No handle, no device.
    assert batch(None, item, q, s, fl, 3, None) == _cabi.ERR_INVALID and b"null handle" in last(None)
    # an optimised image of more than 2^23 blocks: refused before a pixel is read
    item[0].width = item[0].height = 32768
    item[0].channels, item[0].capacity = 1, 1 << 40
    assert built_lib.thmr_jpeg_encode_host_flags(C.byref(item[0]), 95, _cabi.JPEG_420, _cabi.JPEG_OPTIMIZE) == _cabi.ERR_INVALID and b"2^23 blocks" in last(None)


def test_the_modes_bound_holds_and_is_enforced(J):
    for w, h in K.SIZES:
        for img in (K.picture("checker", w, h), K.picture("noise", w, h), K.picture("checker", w, h, 0)):
            for sub in ("4:4:4", "4:2:0"):
                c = 1 if img.ndim == 2 else 3
                bound = J.encode_bound(w, h, c, sub, optimize=True)
                m = 8 if (sub == "4:4:4" or c == 1) else 16
                blocks = -(-w // m) * -(-h // m) * (1 if c == 1 else 3 if m == 8 else 6)
                assert bound == (328 if c == 1 else 623) + 2 * -(-blocks * (23 + 63 * 26) // 8) + 2 >= J.encode_bound(w, h, c, sub)
                assert len(J.encode_host(img, quality=100, subsampling=sub, optimize=True, capacity=bound)) <= bound
                with pytest.raises(J.JpegError, match="capacity .* thmr_jpeg_encode_bound_flags"):
                    J.encode_host(img, quality=100, subsampling=sub, optimize=True, capacity=bound - 1)
    assert J.encode_bound(0, 4, 3, optimize=True) == 0 and J.encode_bound(4, 4, 2, optimize=True) == 0 and J.encode_bound(65535, 65535, 3, optimize=True) > 0


def test_every_file_decodes_to_the_default_files_pixels(J):
    Image = pytest.importorskip("PIL.Image")
    for (w, h) in K.SIZES:
        for kind, q in (("smooth", 90), ("noise", 100), ("checker", 100), ("noise", 1), ("white", 75)):
            rgb = K.picture(kind, w, h)
            for img, sub in ((rgb, "4:4:4"), (rgb, "4:2:0"), (rgb[..., 1], "4:2:0")):
                opt = J.encode_host(img, quality=q, subsampling=sub, optimize=True, bgr=False)
                plain = J.encode_host(img, quality=q, subsampling=sub, bgr=False)
                assert KO.markers(opt) == KO.markers(plain) and len(opt) < len(plain), (w, h, kind, q, sub)
                a, b = Image.open(io.BytesIO(opt)), Image.open(io.BytesIO(plain))
                assert a.size == (w, h) and a.mode == b.mode == ("L" if img.ndim == 2 else "RGB")
                assert np.array_equal(np.asarray(a), np.asarray(b)), (w, h, kind, q, sub)
                assert np.array_equal(J.decode_host(opt, bgr=False), J.decode_host(plain, bgr=False)), (w, h, kind, q, sub)
