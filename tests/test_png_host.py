"""The PNG encoder on the CPU (thmr_png_encode_host, the restatement of the kernels that shares their arithmetic: csrc/png_math.h) and the
facade's refusals.  Files are read back by tests/_png_reader.py (zlib.decompress + a NumPy unfilter, every CRC checked) and, where it
imports, by Pillow.  tests/test_gpu_png.py holds the device against these very files byte for byte."""
import ctypes as C
import io
import zlib

import numpy as np
import pytest

import _png_cases as K
import _png_reader as R


@pytest.fixture(scope="module")
def P(built_lib):
    from tokenhmr_amd import png
    return png


def check_file(P, data, pixels):
    got, filters, stream = R.read(data)
    assert np.array_equal(got, pixels)
    assert np.array_equal(filters, R.expected_filters(pixels))
    h, w, c = pixels.shape
    assert len(data) <= P.bound(w, h, c)
    return stream


def test_symbols_declared_bound_and_exported(built_lib):
    import __graft_entry__
    from tokenhmr_amd import _cabi
    assert _cabi.ABI_VERSION == 5 and built_lib.thmr_abi_version() == 5
    # (exported and typed in both builds, like every declared function: tests/test_cabi_header.py)
    assert {"thmr_png_segment_bytes", "thmr_png_bound", "thmr_png_encode_host", "thmr_png_create", "thmr_png_destroy", "thmr_png_last_error",
            "thmr_png_encode_batch"} <= set(_cabi.declared_symbols())
    assert "png.hip" in __graft_entry__.SOURCES
    assert C.sizeof(_cabi.PngItem) == 88
    import tokenhmr_amd
    for name in ("PNGEncoder", "imwrite", "imwrite_batch"):
        assert hasattr(tokenhmr_amd, name)


def test_segment_and_bound(P):
    S = P.segment_bytes()
    assert 1 <= S <= 32768
    for (w, h, c) in ((1, 1, 1), (192, 256, 3), (4680, 7, 1), (127, 128, 1)):
        raw = h * (1 + w * c)
        assert P.bound(w, h, c) == raw + 5 * -(-raw // S) + 6 + 57
    assert P.bound(0, 4, 3) == 0 and P.bound(4, 4, 2) == 0 and P.bound(1 << 20, 1 << 12, 1) == 0


@pytest.mark.parametrize("name", [n for n, _ in K.roundtrip_cases()])
def test_round_trip(P, name):
    pixels = dict(K.roundtrip_cases())[name]
    data = K.host_file("roundtrip", name)
    check_file(P, data, pixels)
    if name.endswith(("17x33x3", "64x64x4", "3x5x1")):
        Image = pytest.importorskip("PIL.Image")
        got = np.asarray(Image.open(io.BytesIO(data)))
        assert np.array_equal(got.reshape(pixels.shape), pixels)


def test_filter_tie_goes_to_the_lowest_number(P):
    # two equal constant rows: on row 0 Sub and Paeth tie (both predict the left byte), on row 1 Up and Paeth tie at zero cost
    pixels = np.full((2, 6, 1), 77, np.uint8)
    costs = R.filter_costs(pixels)
    assert costs[0, 1] == costs[0, 4] == costs[0].min() and costs[1, 2] == costs[1, 4] == costs[1].min() == 0
    _, filters, _ = R.read(P.encode_host(pixels))
    assert filters.tolist() == [1, 2]
    # an all-zero image ties all five: filter 0
    _, filters, _ = R.read(P.encode_host(np.zeros((3, 4, 3), np.uint8)))
    assert filters.tolist() == [0, 0, 0]


def test_edge_shapes_hit_the_segment_size(P):
    S = P.segment_bytes()
    assert [h * (1 + w) for h, w in K.edge_shapes(S)] == [S - 1, S, S + 1, 2 * S, 2 * S + 1]


@pytest.mark.parametrize("kind", K.EDGE_KINDS)
def test_segment_edges(P, kind):
    S = P.segment_bytes()
    for name, pixels in K.edge_cases(S):
        if not name.startswith(kind):
            continue
        data = K.host_file("edge", name)
        stream = check_file(P, data, pixels)
        raw = len(stream)
        if kind == "constant":
            assert len(data) <= raw // 30 + 57 + 6, (name, len(data))
        elif kind in ("period2", "period3"):
            assert len(data) < raw // 2, (name, len(data))          # whole-row matches are found: well under the stored size
        else:
            assert raw < len(data) <= P.bound(pixels.shape[1], pixels.shape[0], 1), (name, len(data))       # noise: stored blocks


def test_constant_image_is_compressed(P):
    pixels = K.image("flat", 256, 256, 3)
    data = P.encode_host(pixels)
    check_file(P, data, pixels[..., ::-1])
    assert len(data) <= 256 * (1 + 256 * 3) // 30, len(data)


def test_render_like_size_against_zlib(P):
    # The file over zlib.compress(level 1) of the SAME filtered bytes, so the filter choice cancels.  The encoder is deterministic:
    # this image gives 225940 bytes against zlib's 171136, ratio 1.3202 (zlib itself held to fixed-Huffman blocks in 32 KiB segments
    # gives about 1.32 on such content); the cap leaves 10 % for later matcher changes, not for noise.
    RATIO_MEASURED = 1.3203
    pixels = K.image("render", 256, 512, 3)
    data = P.encode_host(pixels, bgr=False)
    stream = check_file(P, data, pixels)
    ratio = len(data) / len(zlib.compress(stream, 1))
    print(f"render-like 256x512x3: file {len(data)} bytes, zlib level 1 {len(zlib.compress(stream, 1))} bytes, ratio {ratio:.4f}")
    assert ratio <= RATIO_MEASURED * 1.10, ratio


@pytest.mark.parametrize("name", [c[0] for c in K.conversion_cases()])
def test_conversion(P, name):
    _, img, scale, rounding = next(c for c in K.conversion_cases() if c[0] == name)
    got, _, _ = R.read(K.host_file("conversion", name))
    want = K.convert_expected(img, scale, rounding)
    assert np.array_equal(got, want), (img.ravel()[(got != want).ravel()], got[got != want], want[got != want])
    if name.startswith("edges"):
        v = K.conversion_values()
        halves = got.ravel()[:255]
        if rounding == "nearest":         # halves go to the even neighbour
            assert halves.tolist() == [k + (k & 1) for k in range(255)]
        else:
            assert halves.tolist() == list(range(255))
        assert got.ravel()[255:].tolist() == ([0, 0, 255, 255, 255, 255, 0, 255, 0, 0] if rounding == "nearest" else [0, 0, 255, 255, 255, 255, 0, 255, 0, 0])
        assert len(v) == 265


@pytest.mark.parametrize("name", [c[0] for c in K.stride_cases()])
def test_strides_equal_the_contiguous_copy(P, name):
    _, view, kw = next(c for c in K.stride_cases() if c[0] == name)
    assert not view.flags["C_CONTIGUOUS"]
    assert K.host_file("stride", name) == P.encode_host(np.ascontiguousarray(view), **kw)
    R.read(K.host_file("stride", name))


@pytest.mark.parametrize("c", [3, 4])
def test_swap_rb(P, c):
    img = K.image("render", 19, 23, c)
    order = [2, 1, 0, 3][:c]
    swapped = np.ascontiguousarray(img[..., order])
    assert P.encode_host(img, bgr=True) == P.encode_host(swapped, bgr=False)
    assert P.encode_host(img, bgr=True) != P.encode_host(img, bgr=False)
    assert np.array_equal(R.read(P.encode_host(img, bgr=True))[0], swapped)
    grey = K.image("render", 19, 23, 1)
    assert P.encode_host(grey, bgr=True) == P.encode_host(grey, bgr=False)


def test_refusals_by_name(P, built_lib, tmp_path):
    from tokenhmr_amd import _cabi
    img = K.image("noise", 4, 5, 3)
    with pytest.raises(ValueError, match=r"\.jpg"):
        P.imwrite(str(tmp_path / "a.jpg"), img)
    with pytest.raises(ValueError, match=r"\.jpeg"):
        P.imwrite_batch([str(tmp_path / "a.png"), str(tmp_path / "b.jpeg")], [img, img])
    assert not list(tmp_path.iterdir())
    with pytest.raises(P.PngUnsupported, match="16-bit"):
        P.encode_host(np.zeros((4, 5, 3), np.uint16))
    with pytest.raises(P.PngUnsupported, match="2 channels"):
        P.encode_host(np.zeros((4, 5, 2), np.uint8))
    with pytest.raises(P.PngError, match="width and height"):
        P.encode_host(np.zeros((4, 0, 3), np.uint8))
    with pytest.raises(P.PngError, match="capacity"):
        P.encode_host(img, capacity=P.bound(5, 4, 3) - 1)
    assert len(P.encode_host(img, capacity=P.bound(5, 4, 3))) <= P.bound(5, 4, 3)
    with pytest.raises(ValueError, match="rounding"):
        P.encode_host(img, rounding="floor")
    # the batch entry refuses a bad item before it looks at the handle: no handle, no device
    item = (_cabi.PngItem * 1)()
    out = np.empty(P.bound(5, 4, 3), np.uint8)
    P._fill(item[0], img, 1.0, "nearest", True)
    item[0].pixels, item[0].out, item[0].capacity = img.ctypes.data, out.ctypes.data, out.size - 1
    assert built_lib.thmr_png_encode_batch(None, item, 1, None) == _cabi.ERR_INVALID
    assert b"item 0" in built_lib.thmr_png_last_error(None) and b"capacity" in built_lib.thmr_png_last_error(None)
    item[0].capacity, item[0].channels = out.size, 2
    assert built_lib.thmr_png_encode_batch(None, item, 1, None) == _cabi.ERR_UNSUPPORTED
    item[0].channels = 3
    assert built_lib.thmr_png_encode_batch(None, item, 1, None) == _cabi.ERR_INVALID
    assert b"null handle" in built_lib.thmr_png_last_error(None)
