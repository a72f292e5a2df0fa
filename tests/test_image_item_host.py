"""The part of the item check that the PNG and the JPEG encoder share (csrc/image_item_host.h), through both host entry points: one
mutated field per row, the same status from both, each message with the words the encoders' own tests look for; and an item with two
faults, which both refuse for the first."""
import ctypes as C

import numpy as np
import pytest

from tokenhmr_amd import _cabi

W, H = 5, 4

# (field, value or a function of the entry's bound, status, fragment of the message)
ROWS = [
    ("dtype", _cabi.PNG_U16, _cabi.ERR_UNSUPPORTED, b"16-bit"),
    ("dtype", 7, _cabi.ERR_INVALID, b"dtype must be"),
    ("channels", 2, _cabi.ERR_UNSUPPORTED, b"2 channels"),
    ("channels", 5, _cabi.ERR_INVALID, b"channels must be 1, 3 or 4"),
    ("pixels", None, _cabi.ERR_INVALID, b"null pixels"),
    ("out", None, _cabi.ERR_INVALID, b"null out"),
    ("capacity", lambda bound: bound - 1, _cabi.ERR_INVALID, b"capacity"),
]


@pytest.fixture(scope="module")
def entries(built_lib):
    """(name, encode(item) -> status, last_error(), bound of a W x H x 3 image, the bound's name) of each encoder."""
    lib = built_lib
    return [("png", lambda it: lib.thmr_png_encode_host(C.byref(it)), lambda: lib.thmr_png_last_error(None), lib.thmr_png_bound(W, H, 3), b"thmr_png_bound"),
            ("jpeg", lambda it: lib.thmr_jpeg_encode_host(C.byref(it), 95, _cabi.JPEG_420), lambda: lib.thmr_jpeg_encoder_last_error(None),
             lib.thmr_jpeg_encode_bound(W, H, 3, _cabi.JPEG_420), b"thmr_jpeg_encode_bound")]


def good_item(img, out):
    it = _cabi.PngItem()
    it.pixels, it.dtype, it.width, it.height, it.channels = img.ctypes.data, _cabi.PNG_U8, W, H, 3
    it.stride_y, it.stride_x, it.stride_c = W * 3, 3, 1
    it.scale, it.rounding, it.swap_rb, it.compression = 1.0, _cabi.PNG_ROUND_NEAREST, 0, 0
    it.out, it.capacity = out.ctypes.data, out.size
    return it


@pytest.mark.parametrize("row", range(len(ROWS)))
def test_one_mutated_field_is_refused_alike_by_both_encoders(entries, row):
    field, value, status, fragment = ROWS[row]
    img = np.arange(H * W * 3, dtype=np.uint8).reshape(H, W, 3)
    got = []
    for name, encode, last, bound, bound_name in entries:
        out = np.empty(bound, np.uint8)
        it = good_item(img, out)
        assert encode(it) == 0 and it.written > 0, name
        setattr(it, field, value(bound) if callable(value) else value)
        rc = encode(it)
        assert rc == status and fragment in last() and it.written == 0, (name, field, rc, last())
        if field == "capacity":
            assert bound_name in last() and str(bound).encode() in last(), (name, last())
        got.append(rc)
    assert got[0] == got[1]


def test_two_faults_are_refused_for_the_channels_by_both(entries):
    img = np.zeros((H, W, 3), np.uint8)
    texts = []
    for name, encode, last, bound, _ in entries:
        out = np.empty(bound, np.uint8)
        it = good_item(img, out)
        it.channels, it.out = 2, None
        assert encode(it) == _cabi.ERR_UNSUPPORTED and b"2 channels" in last() and b"null out" not in last(), (name, last())
        texts.append(last())
    # the one word in which the two texts differ stays
    assert b"the encoder writes 1, 3 or 4" in texts[0] and b"the encoder reads 1, 3 or 4" in texts[1]
