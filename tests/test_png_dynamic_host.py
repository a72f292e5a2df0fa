"""The PNG encoder's opt-in compression="dynamic" on the CPU (thmr_png_encode_host with compression = THMR_PNG_DYNAMIC; the block rule of
csrc/png_math.h, which the kernels share): every file inflates under zlib and Pillow to the pixels and the filtered stream of the
fixed-mode file and is never longer; tests/_deflate_walk.py reads the blocks (which are dynamic, which stored, whether every declared
code is complete); thmr_png_code_lengths is held against a heapq Huffman tree and the Kraft equality on histograms no image gives; the
size against zlib level 1; the refusals.  tests/test_gpu_png_dynamic.py holds the device against these very files byte for byte."""
import ctypes as C
import functools
import heapq
import io
import zlib
from fractions import Fraction

import numpy as np
import pytest

import _deflate_walk as D
import _png_cases as K
import _png_reader as R


@pytest.fixture(scope="module")
def P(built_lib):
    from tokenhmr_amd import png
    return png


def zstream(data):
    """The zlib stream of a file the encoder wrote: 41 bytes of signature, IHDR and IDAT framing before it, the IDAT CRC and IEND behind."""
    return data[41:len(data) - 16]


@functools.lru_cache(maxsize=None)
def dynamic_file(group, name):
    """The host encoder's dynamic-mode file of one named case of tests/_png_cases.py, computed once (K.host_file is the fixed one)."""
    from tokenhmr_amd import png as P
    if group == "roundtrip":
        return P.encode_host(dict(K.roundtrip_cases())[name], bgr=False, compression="dynamic")
    if group == "edge":
        return P.encode_host(dict(K.edge_cases(P.segment_bytes()))[name], bgr=False, compression="dynamic")
    if group == "conversion":
        _, img, scale, rounding = next(c for c in K.conversion_cases() if c[0] == name)
        return P.encode_host(img, scale=scale, rounding=rounding, compression="dynamic")
    _, view, kw = next(c for c in K.stride_cases() if c[0] == name)
    return P.encode_host(view, compression="dynamic", **kw)


def all_cases():
    # named before the library is loaded: with another segment size dynamic_file() finds no edge case of these names
    return ([("roundtrip", n) for n, _ in K.roundtrip_cases()] + [("edge", n) for n, _ in K.edge_cases(16384)] +
            [("conversion", c[0]) for c in K.conversion_cases()] + [("stride", c[0]) for c in K.stride_cases()])


@pytest.mark.parametrize("group,name", all_cases())
def test_dynamic_stream_is_valid_and_pixels_unchanged(P, group, name):
    Image = pytest.importorskip("PIL.Image")
    fixed, dyn = K.host_file(group, name), dynamic_file(group, name)
    pixels, filters, stream = R.read(fixed)
    got, dfilters, dstream = R.read(dyn)
    assert np.array_equal(got, pixels) and np.array_equal(dfilters, filters)
    assert zlib.decompress(zstream(dyn)) == zlib.decompress(zstream(fixed)) == stream == dstream
    assert len(dyn) <= len(fixed), (len(dyn), len(fixed))
    h, w, c = pixels.shape
    assert len(dyn) <= P.bound(w, h, c)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(dyn))).reshape(pixels.shape), np.asarray(Image.open(io.BytesIO(fixed))).reshape(pixels.shape))
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(dyn))).reshape(pixels.shape), pixels)


def test_default_is_the_fixed_mode(P):
    img = K.image("render", 64, 64, 3)
    assert P.encode_host(img) == P.encode_host(img, compression="fixed") != P.encode_host(img, compression="dynamic")
    assert all(b["btype"] != 2 for b in D.blocks(zstream(P.encode_host(img))))


def segments_of(blocks):
    """The walker's blocks grouped by segment: a coded segment but the last is followed by an empty stored block."""
    segs, i = [], 0
    while i < len(blocks):
        b = blocks[i]
        if b["btype"] != 0 and not b["final"]:
            assert blocks[i + 1]["btype"] == 0 and blocks[i + 1]["bytes"] == 0, "no sync marker behind a coded segment"
            i += 1
        segs.append(b)
        i += 1
    return segs


def check_blocks(P, data, raw):
    S = P.segment_bytes()
    segs = segments_of(D.blocks(zstream(data)))
    assert [b["bytes"] for b in segs] == [min(S, raw - o) for o in range(0, raw, S)]
    assert [b["final"] for b in segs] == [False] * (len(segs) - 1) + [True]
    for b in segs:
        if b["btype"] == 2:
            assert b["complete"] == (True, True, True), b["complete"]
            assert max(b["ll"]) <= 15 and max(b["d"]) <= 15 and max(b["cl"]) <= 7
            assert len(b["ll"]) == 257 or b["ll"][-1] != 0            # HLIT trimmed
            assert len(b["d"]) == 1 or b["d"][-1] != 0                # HDIST trimmed
            assert sum(n > 0 for n in b["d"]) >= 2                    # padded to two leaves
    return segs


@pytest.mark.parametrize("kind", K.EDGE_KINDS)
def test_block_types_at_the_segment_edges(P, kind):
    for name, pixels in K.edge_cases(P.segment_bytes()):
        if not name.startswith(kind):
            continue
        segs = check_blocks(P, dynamic_file("edge", name), pixels.shape[0] * (1 + pixels.shape[1]))
        if kind == "noise":
            # incompressible: stored blocks in either mode (the one-byte tail of the S + 1 and 2 S + 1 shapes is 3 bytes as a fixed
            # block against 6 stored, in either mode too)
            assert all(b["btype"] == (1 if b["bytes"] == 1 else 0) for b in segs), (name, [(b["btype"], b["bytes"]) for b in segs])
            assert dynamic_file("edge", name) == K.host_file("edge", name)


def test_block_types_of_the_round_trip_cases(P):
    seen = {(final, btype): 0 for final in (False, True) for btype in (0, 1, 2)}
    for name, pixels in K.roundtrip_cases():
        h, w, c = pixels.shape
        if h * w > 64 * 64 and c != 3:
            continue                                              # the walker is pure Python: the large shapes once
        segs = check_blocks(P, dynamic_file("roundtrip", name), h * (1 + w * c))
        for b in segs:
            seen[(b["final"], b["btype"])] += 1
        if (h, w) == (1, 1):
            assert all(b["btype"] != 2 for b in segs), name       # a header costs more than it saves
        if name.startswith("render") and h * w >= 64 * 64:
            assert all(b["btype"] == 2 for b in segs), (name, [b["btype"] for b in segs])
    # the last segment of an image and a segment before it end differently: both occur as dynamic blocks
    assert seen[(True, 2)] > 0 and seen[(False, 2)] > 0, seen
    assert seen[(True, 0)] > 0 and seen[(True, 1)] > 0, seen


# ---- wide images: row distances beyond 4096, tokens of more than 33 bits ----

def long_match_image(seed, h, w, c):
    """Rows of small signed noise (the filters leave them nearly alone), each with one stretch of 131 ... 250 bytes copied from the
    row above: a few rare long length symbols per segment, at a row distance that takes 11 or 12 extra bits."""
    rng = np.random.default_rng([seed, h, w, c])
    mag = rng.geometric(0.35, (h, w * c)) - 1
    sign = rng.integers(0, 2, (h, w * c)) * 2 - 1
    img = ((mag * sign) & 255).astype(np.uint8)
    for y in range(1, h):
        n = int(rng.integers(131, 251))
        x = int(rng.integers(0, w * c - n))
        img[y, x:x + n] = img[y - 1, x:x + n]
    return img.reshape(h, w, c)


@functools.lru_cache(maxsize=None)
def wide_cases():
    """[(name, image)]: "long-*" hold a token of more than 33 bits that starts so late in a 32-bit word that it reaches a third one (the
    seeds were searched for that; test_wide_images holds them to it), the others are render-like frames a few rows high."""
    return ([(f"long-{h}x{w}x{c}-seed{seed}", long_match_image(seed, h, w, c)) for seed, h, w, c in ((6, 12, 1920, 3), (8, 12, 1920, 3), (3, 8, 3840, 3))] +
            [(f"render-{h}x{w}x{c}", K.image("render", h, w, c)) for h, w, c in ((6, 1920, 3), (4, 3840, 3), (5, 1292, 3))])


@functools.lru_cache(maxsize=None)
def wide_file(name):
    from tokenhmr_amd import png as P
    return P.encode_host(dict(wide_cases())[name], bgr=False, compression="dynamic")


@pytest.mark.parametrize("name", [n for n, _ in wide_cases()])
def test_wide_images(P, name):
    pixels = dict(wide_cases())[name]
    h, w, c = pixels.shape
    dyn, fixed = wide_file(name), P.encode_host(pixels, bgr=False)
    assert zlib.decompress(zstream(dyn)) == zlib.decompress(zstream(fixed)) and len(dyn) < len(fixed)
    assert np.array_equal(R.read(dyn)[0], pixels)
    segs = check_blocks(P, dyn, h * (1 + w * c))
    assert all(b["btype"] == 2 for b in segs)
    if name.startswith("long"):
        # a segment starts on a word of the device's bit buffer, so the offset from the block's first bit is the offset there: such a
        # token does not fit 64 bits once shifted to its place in a word, and has to go in as two pieces
        spill = [(at, n) for b in segs for at, n in b["long_tokens"] if (at & 31) + n > 64]
        assert spill and all(n <= 48 for _, n in spill), [b["long_tokens"] for b in segs]


def test_constant_images_decode_in_both_block_kinds(P):
    for pixels in (K.image("flat", 256, 256, 3), K.edge_image("constant", 255, 128)):
        data = P.encode_host(pixels, bgr=False, compression="dynamic")
        assert np.array_equal(R.read(data)[0], pixels)
        check_blocks(P, data, pixels.shape[0] * (1 + pixels.shape[1] * pixels.shape[2]))
        assert len(data) <= len(P.encode_host(pixels, bgr=False))


# ---- thmr_png_code_lengths ----

def code_lengths(lib, freq, max_bits):
    f = (C.c_int32 * len(freq))(*freq)
    lens = (C.c_int32 * len(freq))(*([-1] * len(freq)))
    assert lib.thmr_png_code_lengths(f, len(freq), max_bits, lens) == 0, lib.thmr_png_last_error(None)
    return list(lens)


def heapq_huffman(freq):
    """(cost in bits, deepest leaf) of a Huffman tree of the non-zero frequencies; of equal weights the shallower subtree is merged first,
    which gives the optimal tree of the smallest height."""
    heap = [(f, 0) for f in freq if f > 0]
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return cost, heap[0][1]


def check_lengths(lib, freq, max_bits):
    lens = code_lengths(lib, freq, max_bits)
    used = [s for s, f in enumerate(freq) if f > 0]
    assert all(lens[s] == 0 for s, f in enumerate(freq) if f == 0)
    assert all(1 <= lens[s] <= max_bits for s in used), (max(lens), max_bits)
    assert sum(Fraction(1, 1 << lens[s]) for s in used) == 1, "Kraft sum"
    order = sorted(used, key=lambda s: (-freq[s], s))
    for s, t in zip(order, order[1:]):             # more frequent, or as frequent with the lower index: never the longer code
        assert lens[s] <= lens[t], (s, t, freq[s], freq[t], lens[s], lens[t])
    cost, height = heapq_huffman(freq)
    ours = sum(freq[s] * lens[s] for s in used)
    if height <= max_bits:                         # the limit does not bind: the cost is the optimum
        assert ours == cost, (ours, cost)
    else:
        assert ours > cost
    return lens


def test_code_lengths_on_random_histograms(built_lib):
    rng = np.random.default_rng(2024)
    for n in [2, 3, 19, 30, 286] + [int(v) for v in rng.integers(2, 287, 60)]:
        shape = rng.integers(0, 3)
        if shape == 0:
            freq = rng.integers(1, 1000, n)
        elif shape == 1:                            # skewed, with zeros
            freq = (rng.exponential(1.0, n) ** 4 * 3).astype(np.int64)
        else:                                       # many ties
            freq = rng.integers(0, 4, n)
        freq = [int(f) for f in freq]
        while sum(f > 0 for f in freq) < 2:
            freq[int(rng.integers(0, n))] += 1
        check_lengths(built_lib, freq, 15)


def fibonacci(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def test_code_lengths_where_the_limit_binds(built_lib):
    fib = fibonacci(16)                             # 1, 1, 2, 3 ... 987: a tree 15 deep, the sum 2583 below a segment's token count
    assert fib[-1] == 987 and sum(fib) < 16384 // 3 and heapq_huffman(fib)[1] == 15
    assert sorted(check_lengths(built_lib, fib, 15)) == sorted([15, 15] + list(range(1, 15)))
    for limit in (14, 12, 9, 5, 4):                 # the same shape under a limit that binds
        assert heapq_huffman(fib)[1] > limit
        assert max(check_lengths(built_lib, fib, limit)) == limit
    # in the middle of the literal / length alphabet, among zeros and beside a flat floor of rare symbols
    freq = [0] * 286
    for k, f in enumerate(fibonacci(26)):
        freq[40 + 3 * k] = f
    for s in range(200, 286):
        freq[s] = 1
    assert heapq_huffman(freq)[1] > 15
    assert max(check_lengths(built_lib, freq, 15)) == 15
    # the code-length alphabet: 19 symbols, 7 bits
    skew = fibonacci(19)
    assert heapq_huffman(skew)[1] == 18
    assert max(check_lengths(built_lib, skew, 7)) == 7
    assert max(check_lengths(built_lib, skew[::-1], 7)) == 7
    # 2^max_bits symbols fill the limit exactly
    assert check_lengths(built_lib, [5, 1, 1, 9], 2) == [2, 2, 2, 2]


def test_code_lengths_edges_and_refusals(built_lib):
    from tokenhmr_amd import _cabi
    assert code_lengths(built_lib, [0, 7, 0], 15) == [0, 1, 0]             # one symbol in use: one bit
    assert code_lengths(built_lib, [0, 0], 15) == [0, 0]
    assert code_lengths(built_lib, [3, 3], 15) == [1, 1]
    one = (C.c_int32 * 1)(1)
    for n, bits in ((0, 15), (287, 15), (1, 0), (1, 16)):
        assert built_lib.thmr_png_code_lengths(one, n, bits, one) == _cabi.ERR_INVALID
    assert built_lib.thmr_png_code_lengths(None, 1, 15, one) == _cabi.ERR_INVALID
    five = (C.c_int32 * 5)(1, 1, 1, 1, 1)
    assert built_lib.thmr_png_code_lengths(five, 5, 2, five) == _cabi.ERR_INVALID          # five codes of two bits do not exist
    neg = (C.c_int32 * 2)(-1, 4)
    assert built_lib.thmr_png_code_lengths(neg, 2, 15, neg) == _cabi.ERR_INVALID
    assert "thmr_png_code_lengths" in _cabi.declared_symbols()
    assert hasattr(_cabi.load(exp=True), "thmr_png_code_lengths")          # exported from both libraries


# ---- size ----

def test_render_like_size_against_zlib_dynamic(P):
    # As tests/test_png_host.py::test_render_like_size_against_zlib: the file over zlib.compress(level 1) of the SAME filtered bytes, so
    # the filter choice cancels.  The encoder is deterministic: in the dynamic mode this image gives 164914 bytes against zlib's 171136,
    # ratio 0.9636 (the fixed mode: 225940 bytes, 1.3202; zlib's level 1 also writes dynamic blocks, and its hash chains see less than
    # the row and pixel distances tried here); the cap leaves 10 % for later matcher changes, not for noise.
    RATIO_MEASURED = 0.9637
    pixels = K.image("render", 256, 512, 3)
    data = P.encode_host(pixels, bgr=False, compression="dynamic")
    fixed = P.encode_host(pixels, bgr=False)
    got, _, stream = R.read(data)
    assert np.array_equal(got, pixels)
    z = len(zlib.compress(stream, 1))
    ratio, fixed_ratio = len(data) / z, len(fixed) / z
    print(f"render-like 256x512x3: dynamic {len(data)} bytes, fixed {len(fixed)} bytes, zlib level 1 {z} bytes, ratios {ratio:.4f} and {fixed_ratio:.4f}")
    assert ratio <= RATIO_MEASURED * 1.10, ratio
    assert ratio < fixed_ratio, (ratio, fixed_ratio)


# ---- refusals ----

def test_refusals(P, built_lib, tmp_path):
    from tokenhmr_amd import _cabi
    img = K.image("noise", 4, 5, 3)
    for bad in ("best", "Dynamic", 1, None):
        with pytest.raises(ValueError, match="compression"):
            P.encode_host(img, compression=bad)
    with pytest.raises(ValueError, match="compression"):
        P._fill(_cabi.PngItem(), img, 1.0, "nearest", True, compression="best")
    assert (_cabi.PNG_FIXED, _cabi.PNG_DYNAMIC) == (0, 1) and C.sizeof(_cabi.PngItem) == 88
    # the five positional arguments still fill a fixed-mode item
    item = (_cabi.PngItem * 2)()
    out = np.empty(P.bound(5, 4, 3), np.uint8)
    for it in item:
        P._fill(it, img, 1.0, "nearest", True)
        assert it.compression == _cabi.PNG_FIXED
        it.pixels, it.out, it.capacity = img.ctypes.data, out.ctypes.data, out.size
    P._fill(item[0], img, 1.0, "nearest", True, compression="dynamic")
    assert item[0].compression == _cabi.PNG_DYNAMIC
    # any other value is refused by both entry points, the batch one naming the item before it looks at the handle
    for bad in (2, -1):
        item[1].compression = bad
        assert built_lib.thmr_png_encode_host(C.byref(item[1])) == _cabi.ERR_INVALID
        assert b"compression" in built_lib.thmr_png_last_error(None) and item[1].written == 0
        assert built_lib.thmr_png_encode_batch(None, item, 2, None) == _cabi.ERR_INVALID
        assert b"item 1" in built_lib.thmr_png_last_error(None) and b"compression" in built_lib.thmr_png_last_error(None)
    item[1].compression = _cabi.PNG_DYNAMIC
    assert built_lib.thmr_png_encode_batch(None, item, 2, None) == _cabi.ERR_INVALID
    assert b"null handle" in built_lib.thmr_png_last_error(None)
    assert built_lib.thmr_png_encode_host(C.byref(item[1])) == 0 and 0 < item[1].written <= out.size
    # imwrite still accepts and ignores cv2's params, and refuses a bad mode before it needs a device or writes a file
    with pytest.raises(ValueError, match="compression"):
        P.PNGEncoder.encode(None, [img], compression=["fixed", "dynamic"])
    assert not list(tmp_path.iterdir())
