"""The JPEG encoder on the CPU (thmr_jpeg_encode_host, the restatement of the kernels that shares their arithmetic: csrc/jpegenc_math.h)
against the files Pillow / libjpeg-turbo wrote — the stored ones of tests/golden/jpeg_enc_small.npz and, where the installed Pillow has
libjpeg-turbo, live ones — WHOLE file, byte for byte; the conversions and layouts; every refusal by name; the bound; and every file read
back by the repository's own decoder and by Pillow.  tests/test_gpu_jpeg_enc.py holds the device against encode_host byte for byte."""
import ctypes as C
import io

import numpy as np
import pytest

import _jpeg_enc_cases as K


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


def pillow_file(Image, img, quality, subsampling):
    buf = io.BytesIO()
    kw = {} if img.ndim == 2 else {"subsampling": K.PIL_SUBSAMPLING[subsampling]}
    Image.fromarray(np.ascontiguousarray(img)).save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def test_symbols_declared_bound_and_exported(built_lib):
    import __graft_entry__
    from tokenhmr_amd import _cabi
    assert _cabi.ABI_VERSION == 5 and built_lib.thmr_abi_version() == 5
    names = {"thmr_jpeg_encode_bound", "thmr_jpeg_encode_host", "thmr_jpeg_encoder_create", "thmr_jpeg_encoder_destroy", "thmr_jpeg_encoder_last_error",
             "thmr_jpeg_encode_batch"}
    assert names <= set(_cabi.declared_symbols())           # the header parses, and every parameter type is one the binding rule knows
    for name in names:
        assert hasattr(built_lib, name) and isinstance(getattr(built_lib, name).argtypes, list)
    assert built_lib.thmr_jpeg_encode_batch.argtypes == [C.c_void_p, C.POINTER(_cabi.PngItem), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    assert "jpegenc.hip" in __graft_entry__.SOURCES
    assert (_cabi.JPEG_444, _cabi.JPEG_422, _cabi.JPEG_420) == (0, 1, 2)
    assert len(_cabi.STRUCTS) == 21                         # an image is a thmr_png_item: no new struct


def test_golden_covers_what_it_should():
    table, arrays = K.golden()
    assert len(arrays["versions"]) == 2
    assert {(c["width"], c["height"]) for c in table.values()} == set(K.SIZES)
    for mode in ("444", "420", "grey"):
        assert {c["quality"] for c in table.values() if c["mode"] == mode} == set(K.QUALITIES)
        for size in K.SIZES:
            kinds = {c["kind"] for c in table.values() if c["mode"] == mode and (c["width"], c["height"]) == size}
            assert kinds == {"smooth", "noise", "black", "white", "checker"}
    assert all(c["quality"] == 100 for c in table.values() if c["kind"] == "checker")


@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_equals_the_stored_pillow_file(J, size):
    table, _ = K.golden()
    names = [n for n, c in table.items() if (c["width"], c["height"]) == size]
    assert len(names) >= 15
    for name in names:
        c = table[name]
        got = J.encode_host(K.golden_input(name), quality=c["quality"], subsampling=K.SUBSAMPLING[c["mode"]], bgr=False)
        want = K.golden_file(name)
        assert got == want, (name, K.first_difference(got, want))


@pytest.mark.parametrize("size", K.SIZES + [(256, 512)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_equals_the_installed_pillow(J, size):
    Image = pillow()
    w, h = size
    kinds = ("smooth", "noise") if size == (256, 512) else ("smooth", "noise", "black", "white", "checker")
    for kind in kinds:
        rgb = K.picture(kind, w, h)
        for q in ((30, 95) if size == (256, 512) else K.QUALITIES):
            for img, sub in ((rgb, "4:4:4"), (rgb, "4:2:0"), (rgb[..., 1], "4:2:0")):
                got, want = J.encode_host(img, quality=q, subsampling=sub, bgr=False), pillow_file(Image, img, q, sub)
                assert got == want, (kind, q, sub, img.ndim, K.first_difference(got, want))


def test_container(J):
    data = J.encode_host(K.picture("smooth", 17, 23), quality=75, subsampling="4:2:0")
    assert data[:20] == bytes([0xFF, 0xD8, 0xFF, 0xE0, 0, 16]) + b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]) and data[-2:] == b"\xff\xd9"
    markers, i = [], 2
    while data[i + 1] != 0xDA:
        markers.append((data[i + 1], data[i + 4]))
        i += 2 + data[i + 2] * 256 + data[i + 3]
    assert [m for m, _ in markers] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4]
    assert [b for m, b in markers if m == 0xDB] == [0, 1] and [b for m, b in markers if m == 0xC4] == [0x00, 0x10, 0x01, 0x11]
    sof = data.index(b"\xff\xc0")
    assert data[sof + 4:sof + 19] == bytes([8, 0, 23, 0, 17, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert data[i:i + 14] == bytes([0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    grey = J.encode_host(K.picture("smooth", 17, 23, 0), quality=75)
    assert grey.count(b"\xff\xdb") == 1 and grey.count(b"\xff\xc4") == 2 and len(grey) - len(grey[grey.index(b"\xff\xda") + 10:]) == 328


def test_channel_swap_alpha_and_grey_layouts(J):
    rgb = K.picture("smooth", 19, 23)
    bgr = np.ascontiguousarray(rgb[..., ::-1])
    want = J.encode_host(rgb, bgr=False)
    assert J.encode_host(bgr, bgr=True) == want != J.encode_host(rgb, bgr=True)
    rgba = K.picture("smooth", 19, 23, 4)
    assert np.array_equal(rgba[..., :3], rgb)
    assert J.encode_host(rgba, bgr=False) == want                               # the alpha is dropped
    assert J.encode_host(np.ascontiguousarray(rgba[..., [2, 1, 0, 3]]), bgr=True) == want
    grey = K.picture("smooth", 19, 23, 0)
    assert J.encode_host(grey) == J.encode_host(grey[..., None]) == J.encode_host(grey, bgr=False, subsampling="4:4:4")


def test_float_chw_both_roundings_and_strided_panels(J):
    rng = np.random.default_rng(3)
    chw = rng.random((3, 21, 37), dtype=np.float32) * np.float32(1.02) - np.float32(0.01)         # some values outside [0, 1]
    chw[0, 0, :4] = [np.nan, np.inf, -np.inf, 0.5 / 255]
    hwc = chw.transpose(1, 2, 0)
    assert not hwc.flags["C_CONTIGUOUS"]
    v = hwc * np.float32(255)
    with np.errstate(invalid="ignore"):
        nearest = np.where(np.isnan(v), 0, np.clip(np.rint(v), 0, 255)).astype(np.uint8)
        trunc = np.where(np.isnan(v), 0, np.clip(v, 0, 255)).astype(np.uint8)
    assert (nearest != trunc).any()
    assert J.encode_host(hwc, scale=255.0, rounding="nearest", bgr=False) == J.encode_host(nearest, bgr=False)
    assert J.encode_host(hwc, scale=255.0, rounding="trunc", bgr=False) == J.encode_host(trunc, bgr=False)
    sheet = K.picture("noise", 200, 64)
    for view in (sheet[3:50, 20:133, :], sheet[::2, ::3, :], sheet[::-1, :, :], sheet[5:30, 7:40, 1]):
        assert not view.flags["C_CONTIGUOUS"]
        assert J.encode_host(view, quality=90) == J.encode_host(np.ascontiguousarray(view), quality=90)


def test_bound_holds_on_the_largest_codes_and_is_enforced(J):
    for w, h in K.SIZES:
        for img in (K.picture("noise", w, h), K.picture("checker", w, h), K.picture("noise", w, h, 0)):
            for sub in ("4:4:4", "4:2:0"):
                c = 1 if img.ndim == 2 else 3
                bound = J.encode_bound(w, h, c, sub)
                m = 8 if (sub == "4:4:4" or c == 1) else 16
                blocks = -(-w // m) * -(-h // m) * (1 if c == 1 else 3 if m == 8 else 6)
                assert bound == (328 if c == 1 else 623) + 2 * -(-blocks * (22 + 63 * 26) // 8) + 2
                assert len(J.encode_host(img, quality=100, subsampling=sub)) <= bound
                assert len(J.encode_host(img, quality=100, subsampling=sub, capacity=bound)) <= bound
                with pytest.raises(J.JpegError, match="capacity"):
                    J.encode_host(img, quality=100, subsampling=sub, capacity=bound - 1)
    assert J.encode_bound(0, 4, 3) == 0 and J.encode_bound(4, 4, 2) == 0 and J.encode_bound(65536, 4, 3) == 0 and J.encode_bound(65535, 65535, 3) > 0


def test_refusals_by_name(J, built_lib, tmp_path):
    from tokenhmr_amd import _cabi
    img = K.picture("noise", 5, 4)
    with pytest.raises(J.JpegUnsupported, match="16-bit"):
        J.encode_host(np.zeros((4, 5, 3), np.uint16))
    with pytest.raises(J.JpegUnsupported, match="2 channels"):
        J.encode_host(np.zeros((4, 5, 2), np.uint8))
    with pytest.raises(J.JpegUnsupported, match="4:2:2"):
        J.encode_host(img, subsampling="4:2:2")
    with pytest.raises(ValueError, match="subsampling"):
        J.encode_host(img, subsampling="4:1:1")
    for q in (0, 101, -5):
        with pytest.raises(J.JpegError, match="quality must be 1 ... 100"):
            J.encode_host(img, quality=q)
    with pytest.raises(ValueError, match="quality"):
        J.encode_host(img, quality=75.5)
    with pytest.raises(J.JpegError, match="width and height"):
        J.encode_host(np.zeros((4, 0, 3), np.uint8))
    with pytest.raises(ValueError, match="rounding"):
        J.encode_host(img, rounding="floor")
    # the C entry points: sides above 65535, compression != 0, null pointers
    item = (_cabi.PngItem * 2)()
    out = np.empty(J.encode_bound(5, 4, 3), np.uint8)
    q, s = (C.c_int32 * 2)(95, 95), (C.c_int32 * 2)(_cabi.JPEG_420, _cabi.JPEG_420)
    for k in range(2):
        J._fill(item[k], img, 1.0, "nearest", True)
        item[k].pixels, item[k].out, item[k].capacity = img.ctypes.data, out.ctypes.data, out.size
    host, batch, last = built_lib.thmr_jpeg_encode_host, built_lib.thmr_jpeg_encode_batch, built_lib.thmr_jpeg_encoder_last_error
    assert host(C.byref(item[0]), 95, _cabi.JPEG_420) == 0 and item[0].written > 623
    item[1].width = 65536
    assert batch(None, item, q, s, 2, None) == _cabi.ERR_INVALID and b"item 1" in last(None) and b"65535" in last(None)
    item[1].width, item[1].compression = 5, 1
    assert batch(None, item, q, s, 2, None) == _cabi.ERR_INVALID and b"item 1" in last(None) and b"compression" in last(None)
    assert host(C.byref(item[1]), 95, _cabi.JPEG_420) == _cabi.ERR_INVALID
    item[1].compression, item[1].out = 0, None
    assert batch(None, item, q, s, 2, None) == _cabi.ERR_INVALID and b"null out" in last(None)
    item[1].out, item[1].pixels = out.ctypes.data, None
    assert batch(None, item, q, s, 2, None) == _cabi.ERR_INVALID and b"null pixels" in last(None)
    item[1].pixels, item[1].capacity = img.ctypes.data, out.size - 1
    assert batch(None, item, q, s, 2, None) == _cabi.ERR_INVALID and b"item 1" in last(None) and b"capacity" in last(None)
    item[1].capacity, item[1].channels = out.size, 2
    assert batch(None, item, q, s, 2, None) == _cabi.ERR_UNSUPPORTED and b"2 channels" in last(None)
    item[1].channels, item[1].dtype = 3, _cabi.PNG_U16
    assert batch(None, item, q, s, 2, None) == _cabi.ERR_UNSUPPORTED and b"16-bit" in last(None)
    item[1].dtype, s[1] = _cabi.PNG_U8, _cabi.JPEG_422
    assert batch(None, item, q, s, 2, None) == _cabi.ERR_UNSUPPORTED and b"item 1" in last(None) and b"4:2:2" in last(None)
    s[1], q[1] = _cabi.JPEG_444, 0
    assert batch(None, item, q, s, 2, None) == _cabi.ERR_INVALID and b"quality" in last(None)
    q[1] = 100
    assert batch(None, item, None, s, 2, None) == _cabi.ERR_INVALID and batch(None, None, q, s, 2, None) == _cabi.ERR_INVALID
    assert batch(None, item, q, s, 0, None) == _cabi.ERR_INVALID
    # every item is fine: only now is the handle looked at.  No handle, no device.
    assert batch(None, item, q, s, 2, None) == _cabi.ERR_INVALID and b"null handle" in last(None)
    # the facade: extensions and cv2's params, refused before a device is asked for
    for name in ("a.png", "a.jpg.png", "a", "a.jp2"):
        with pytest.raises(ValueError, match="extension"):
            J.imwrite(str(tmp_path / name), img)
    with pytest.raises(ValueError, match=r"\.png"):
        J.imwrite_batch([str(tmp_path / "a.jpg"), str(tmp_path / "b.png")], [img, img])
    with pytest.raises(ValueError, match="flag 2 "):
        J.imwrite(str(tmp_path / "a.jpg"), img, [1, 90, 2, 1])          # IMWRITE_JPEG_PROGRESSIVE
    with pytest.raises(ValueError, match="flag 16 "):
        J.imwrite(str(tmp_path / "a.jpeg"), img, [16, 3])               # IMWRITE_PNG_COMPRESSION
    assert J._params_quality([1, 40], 95) == 40 and J._params_quality(None, 95) == 95
    assert not list(tmp_path.iterdir())


def test_every_file_decodes_to_the_same_pixels_here_and_in_pillow(J):
    Image = pytest.importorskip("PIL.Image")
    for (w, h) in K.SIZES:
        for kind, q in (("smooth", 90), ("noise", 100), ("checker", 100), ("noise", 1)):
            rgb = K.picture(kind, w, h)
            for img, sub in ((rgb, "4:4:4"), (rgb, "4:2:0"), (rgb[..., 1], "4:2:0")):
                data = J.encode_host(img, quality=q, subsampling=sub, bgr=False)
                info = J.probe(data)
                assert (info["width"], info["height"], info["components"]) == (w, h, 1 if img.ndim == 2 else 3)
                assert (info["h_samp"], info["v_samp"]) == ((2, 2) if (sub == "4:2:0" and img.ndim == 3) else (1, 1))
                ours = J.decode_host(data, bgr=False)
                theirs = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
                assert np.array_equal(ours, theirs), (w, h, kind, q, sub)
                if kind == "smooth" and min(w, h) >= 16:                # and they are the picture, not merely equal
                    ref = rgb if img.ndim == 3 else np.repeat(img[..., None], 3, -1)
                    assert np.abs(ours.astype(int) - ref).mean() < 12, (w, h, sub)
