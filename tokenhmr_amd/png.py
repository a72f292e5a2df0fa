"""PNG encoding of device images: the drop-in for cv2.imwrite(".png") (include/tokenhmr_hip.h; csrc/png.hip, png_host.h, png_math.h).

    imwrite("panel.png", panel)                          # device tensor or numpy array, (H, W), (H, W, 1 | 3 | 4); BGR(A) like cv2
    imwrite_batch(paths, panels)                         # ONE device call, the files written from a small thread pool
    files = PNGEncoder("cuda:0").encode([a, b, ...], scale=255, rounding="trunc", bgr=False)      # list[bytes]
    data = encode_host(array)                            # the same bytes on the CPU (thmr_png_encode_host)

An image is uint8 or float32 with any strides (a CHW tensor permuted to HWC, a panel sliced from a sheet: no copy is made).  Float
values are multiplied by `scale` and converted by `rounding`: "nearest" is cv2.imwrite's saturate_cast (nearest even, saturated),
"trunc" is np.clip(x, 0, 255).astype(np.uint8).  The file is 8-bit grey / RGB / RGBA, filtered per row by libpng's default heuristic
and deflated in independent segments; the device and the host path write the same bytes.

compression="fixed" (the default) codes every segment as one fixed-Huffman block; compression="dynamic" gives a segment its own Huffman
code where that is smaller (the pixels, the filters and the segments are the same, the file is about a quarter smaller on render-like
images and costs a second pass over the tokens).  Every entry takes the keyword; PNGEncoder.encode also takes one mode per image.

PNG decoding, split between host and device (csrc/pngdec.hip, pngdec_host.h, pngdec_math.h):

    info = probe(data)                                   # size, bit depth, colour type, bytes per pixel — no device
    item = inflate_window(data, window=(x0, y0, w, h))   # host: chunks + inflate -> the filtered rows the window needs (releases the GIL)
    frames = PNGDecoder("cuda:0").decode([data, ...], windows=[...], bgr=True)        # device uint8 (win_h, win_w, 3) tensors
    frame = decode_host(data, window=None, bgr=True)     # the same arithmetic on the CPU: numpy (h, w, 3) uint8

The pixels are cv2.imread's for the file (IMREAD_COLOR): grey replicated, palette looked up, alpha dropped, a 16-bit sample's high byte —
for 8-bit files Pillow's convert("RGB"), bit for bit.  A file of a kind the decoder does not handle (interlaced, 1 / 2 / 4 bits, ...)
raises PngUnsupported — callers fall back to their host decoder for that file; a malformed one raises PngError.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _cabi, _imwrite


class PngError(_cabi.EngineError):
    """A refused argument (THMR_ERR_INVALID) or a HIP failure."""


class PngUnsupported(PngError):
    """An image of a kind the encoder does not write (THMR_ERR_UNSUPPORTED): 16-bit samples, 2 channels."""


_BY_CODE = {_cabi.ERR_UNSUPPORTED: PngUnsupported}
WRITE_THREADS = _imwrite.WRITE_THREADS


def segment_bytes(lib=None):
    return int((lib or _cabi.load()).thmr_png_segment_bytes())


def bound(width, height, channels, lib=None):
    """The largest file the encoder writes for an image of this size (0 for a size it refuses)."""
    return int((lib or _cabi.load()).thmr_png_bound(int(width), int(height), int(channels)))


def _fill(item, img, scale, rounding, bgr, compression="fixed"):
    """One image -> the fields of a thmr_png_item but the pointers; returns (height, width, channels) as the facade sees them."""
    return _imwrite.fill_item(item, img, scale, rounding, bgr, compression, error=PngError)


def _out(item, h, w, c, lib, capacity=None):
    return _imwrite.out_buffer(item, bound(w, h, c, lib) if capacity is None else capacity)


def encode_host(img, *, scale=1.0, rounding="nearest", bgr=True, compression="fixed", capacity=None, lib=None):
    """One numpy image -> the file's bytes, on the CPU with the kernels' arithmetic: the oracle of PNGEncoder, and what a caller without
    a device gets.  capacity: the output buffer's size (default thmr_png_bound), for the refusal test."""
    lib = lib or _cabi.load()
    img = np.asarray(img)
    item = _cabi.PngItem()
    h, w, c = _fill(item, img, scale, rounding, bgr, compression=compression)
    item.pixels = img.ctypes.data
    buf = _out(item, h, w, c, lib, capacity)
    rc = lib.thmr_png_encode_host(C.byref(item))
    if rc != 0:
        _cabi.raise_error(rc, "thmr_png_encode_host", lib.thmr_png_last_error(None), PngError, _BY_CODE)
    return buf[:item.written].tobytes()


# ---- decoding ----
class PngInfo(C.Structure):
    """The info words of thmr_png_probe by name (header: THMR_PNG_INFO_*)."""
    _fields_ = [(n, C.c_int32) for n in _cabi.PNG_INFO_FIELDS] + [("reserved", C.c_int32 * (_cabi.PNG_INFO_WORDS - len(_cabi.PNG_INFO_FIELDS)))]


class PngPlan(C.Structure):
    """The plan words of thmr_png_inflate_window by name (header: THMR_PNG_PLAN_*), the palette as 256 x (R, G, B) bytes behind them."""
    _fields_ = [(n, C.c_int32) for n in _cabi.PNG_PLAN_FIELDS] + [("palette", (C.c_uint8 * 3) * 256)]


assert C.sizeof(PngInfo) == 4 * _cabi.PNG_INFO_WORDS and C.sizeof(PngPlan) == 4 * _cabi.PNG_PLAN_WORDS and PngPlan.palette.offset == 4 * _cabi.PNG_PLAN_PALETTE


def _raise_dec(lib, rc, what):
    _cabi.raise_error(rc, what, lib.thmr_png_decoder_last_error(None), PngError, _BY_CODE)


def _buf(data):
    """bytes-like -> (object that keeps the memory alive, address, length) without a copy where the buffer allows it."""
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    return a, a.ctypes.data, a.size


def _window(window):
    if window is None:
        return None
    return (C.c_int32 * 4)(*[int(v) for v in window])


def band_rows(lib=None):
    """Rows the un-filter kernel takes at once (thmr_png_decode_band_rows): the tests put their heights around it."""
    return int((lib or _cabi.load()).thmr_png_decode_band_rows())


def probe(data, lib=None):
    """dict(height, width, bit_depth, colour_type, interlace, bpp) of a supported file; PngUnsupported / PngError otherwise."""
    lib = lib or _cabi.load()
    keep, ptr, n = _buf(data)
    info = PngInfo()
    rc = lib.thmr_png_probe(C.c_void_p(ptr), n, C.byref(info))
    if rc != 0:
        _raise_dec(lib, rc, "thmr_png_probe")
    return {k: int(getattr(info, k)) for k in ("height", "width", "bit_depth", "colour_type", "interlace", "bpp")}


def inflate(zdata, capacity, lib=None):
    """The decoder's own inflate on a whole zlib stream (thmr_png_inflate) -> bytes; PngError for a malformed stream or one that holds
    more than `capacity` bytes."""
    lib = lib or _cabi.load()
    keep, ptr, n = _buf(zdata)
    out = np.empty(max(int(capacity), 1), dtype=np.uint8)
    written = C.c_int64(0)
    rc = lib.thmr_png_inflate(C.c_void_p(ptr), n, C.c_void_p(out.ctypes.data), int(capacity), C.byref(written))
    if rc != 0:
        _raise_dec(lib, rc, "thmr_png_inflate")
    return out[:written.value].tobytes()


class PlannedPng:
    """One inflated window: `rows` (rows_kept, 1 + kept_row_bytes) uint8, the filter byte first in each row, `plan` the PngPlan
    that says which rows they are, `window` (x0, y0, w, h) and `size` (H, W) of the frame."""

    __slots__ = ("rows", "plan", "window", "size")

    def __init__(self, rows, plan, window, size):
        self.rows, self.plan, self.window, self.size = rows, plan, window, size

    @property
    def nbytes(self):
        return self.rows.nbytes


def inflate_window(data, window=None, lib=None):
    """The host half for one file: walks the chunks and inflates the rows down to the last one `window` (default: the whole frame)
    needs, keeping what can influence it.  Thread-safe, and the GIL is released while it runs."""
    lib = lib or _cabi.load()
    keep, ptr, n = _buf(data)
    win = _window(window)
    plan, need = PngPlan(), C.c_int64(0)
    rc = lib.thmr_png_inflate_window(C.c_void_p(ptr), n, win, None, 0, C.byref(plan), C.byref(need))          # the size first
    if rc != 0:
        _raise_dec(lib, rc, "thmr_png_inflate_window")
    buf = np.empty(need.value, dtype=np.uint8)
    if need.value:
        rc = lib.thmr_png_inflate_window(C.c_void_p(ptr), n, win, C.c_void_p(buf.ctypes.data), need.value, C.byref(plan), C.byref(need))
        if rc != 0:
            _raise_dec(lib, rc, "thmr_png_inflate_window")
    rows = buf[:need.value].reshape(plan.rows_kept, 1 + plan.kept_row_bytes) if need.value else buf.reshape(0, 1)
    return PlannedPng(rows, plan, (plan.win_x0, plan.win_y0, plan.win_w, plan.win_h), (plan.height, plan.width))


def decode_host(data, window=None, bgr=True, lib=None):
    """The full decode of a window on the CPU (thmr_png_decode_host): (h, w, 3) uint8.  The oracle of the device path, and what a
    caller without a device gets."""
    lib = lib or _cabi.load()
    keep, ptr, n = _buf(data)
    if window is None:
        info = probe(data, lib)
        window = (0, 0, info["width"], info["height"])
    w, h = int(window[2]), int(window[3])
    out = np.empty((max(h, 0), max(w, 0), 3), dtype=np.uint8)
    rc = lib.thmr_png_decode_host(C.c_void_p(ptr), n, _window(window), int(bool(bgr)), C.c_void_p(out.ctypes.data), max(w, 0) * 3)
    if rc != 0:
        _raise_dec(lib, rc, "thmr_png_decode_host")
    return out


class PNGDecoder(_cabi.Handle):
    """Owns a thmr_png_decoder handle: two grow-only sets of pinned + device staging, used alternately, and the scratch of unfiltered
    rows.  One stream at a time; a call captured in a graph keeps reading its staging set, so give a captured call a decoder of its own."""
    error, error_by_code = PngError, _BY_CODE

    def __init__(self, device="cuda:0"):
        super().__init__(device, "thmr_png_decoder", "PNGDecoder needs a GPU device; decode_host() is the CPU decode")
        self.last_row_bytes = 0
        self._open(self._index())

    def decode_planned(self, planned, bgr=True, out=None, row_strides=None):
        """Items already inflated (in worker threads) -> one device tensor (win_h, win_w, 3) uint8 each, in ONE batch call on the current
        stream.  out: a list of uint8 device tensors to write into instead (1-D or any shape; item i starts at out[i]'s first byte)
        with row_strides[i] bytes per row, default win_w * 3; bytes of a row beyond win_w * 3 are left alone."""
        n = len(planned)
        if n == 0:
            return []
        if out is None:
            out = [torch.empty(p.window[3], p.window[2], 3, dtype=torch.uint8, device=self.device) for p in planned]
        rows, plans, outs = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
        wins, strides = (C.c_int32 * (4 * n))(), (C.c_int64 * n)()
        for i, p in enumerate(planned):
            x0, y0, w, h = p.window
            stride = int(row_strides[i]) if row_strides is not None else w * 3
            o = out[i]
            if o.dtype != torch.uint8 or o.device != self.device or not o.is_contiguous():
                raise ValueError(f"out[{i}] must be a contiguous uint8 tensor on {self.device}")
            if h > 0 and w > 0 and o.numel() < (h - 1) * stride + w * 3:
                raise ValueError(f"out[{i}] holds {o.numel()} bytes, the window needs {(h - 1) * stride + w * 3}")
            rows[i] = p.rows.ctypes.data if p.rows.size else None
            plans[i] = C.addressof(p.plan)
            wins[4 * i:4 * i + 4] = [x0, y0, w, h]
            outs[i] = o.data_ptr() if o.numel() else None
            strides[i] = stride
        self.last_row_bytes = sum(p.nbytes for p in planned)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            rc = self.lib.thmr_png_decode_batch(self.h, rows, plans, wins, outs, strides, n, int(bool(bgr)), C.c_void_p(stream.cuda_stream))
        self._check(rc, "thmr_png_decode_batch")
        return out

    def decode(self, datas, windows=None, bgr=True):
        """A list of PNG files (bytes) -> a list of device uint8 tensors (win_h, win_w, 3); windows: one (x0, y0, w, h) or None (the
        whole frame) per file.  The inflate runs here, one file after the other; use inflate_window in worker threads and
        decode_planned to overlap it."""
        windows = [None] * len(datas) if windows is None else windows
        return self.decode_planned([inflate_window(d, w, self.lib) for d, w in zip(datas, windows)], bgr=bgr)


class PNGEncoder(_cabi.Handle):
    """Owns a thmr_png handle: grow-only device scratch and pinned staging.  One stream at a time; encode() synchronises it."""
    error, error_by_code = PngError, _BY_CODE

    def __init__(self, device="cuda:0"):
        super().__init__(device, "thmr_png", "PNGEncoder needs a GPU device; encode_host() is the CPU encode")
        self._open(self._index())

    def encode(self, images, *, scale=1.0, rounding="nearest", bgr=True, compression="fixed"):
        """A list of images — device tensors, or host tensors / numpy arrays (uploaded) — of any sizes, dtypes and strides -> the files,
        list[bytes], in ONE batch call on the current stream.  bgr: the images hold B, G, R(, A) like cv2's; False: R, G, B(, A).
        compression: "fixed" or "dynamic" for all images, or a list with one of them per image."""
        n = len(images)
        if not isinstance(compression, (str, list, tuple)):
            raise ValueError(f"compression must be 'fixed', 'dynamic' or a list of them, one per image, got {compression!r}")
        modes = _imwrite.per_image(compression, n, "compression modes")
        if n == 0:
            return []
        items = (_cabi.PngItem * n)()
        keep, bufs = [], []
        for i, img in enumerate(images):
            img = _imwrite.to_device_image(img, i, self.device, PngError, PngUnsupported)
            h, w, c = _fill(items[i], img, scale, rounding, bgr, compression=modes[i])
            items[i].pixels = img.data_ptr()
            keep.append(img)
            bufs.append(_out(items[i], h, w, c, self.lib))
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            rc = self.lib.thmr_png_encode_batch(self.h, items, n, C.c_void_p(stream.cuda_stream))
        self._check(rc, "thmr_png_encode_batch")
        return [bufs[i][:items[i].written].tobytes() for i in range(n)]


_encoders = _imwrite.encoders          # keyed (encoder class, device): jpeg.py's live in the same cache


def _decoder(cls, device):
    device = _cabi.Handle.cuda_device("cuda" if device is None else device, "imread needs a GPU device; decode_host() is the CPU decode", resolve=True)
    if (cls, device) not in _encoders:
        _encoders[(cls, device)] = cls(device)
    return _encoders[(cls, device)]


def imread(path, device=None, bgr=True):
    """cv2.imread(path, IMREAD_COLOR | IMREAD_IGNORE_ORIENTATION) onto the device: an (H, W, 3) uint8 device tensor, B, G, R (bgr=False:
    R, G, B), or None for an unreadable file, as cv2 answers.  A PNG file goes through PNGDecoder and a baseline JPEG through
    jpeg.JpegDecoder, whole frame, both bit-equal to the host decoders; a file of any other kind (or of a kind neither handles) is
    decoded by datasets.default_imread() and uploaded once.  device: default the current GPU."""
    from . import jpeg as J
    try:
        with open(path, "rb") as f:
            data = f.read()
    except OSError:
        return None
    planned = None
    try:                                        # the host halves need no device: what they refuse as malformed is an unreadable file
        if data[:8] == b"\x89PNG\r\n\x1a\n":
            planned = (PNGDecoder, inflate_window(data))
        elif data[:2] == b"\xff\xd8":
            planned = (J.JpegDecoder, J.entropy_decode(data))
    except (PngUnsupported, J.JpegUnsupported):
        pass                                    # a kind neither decoder handles: the host decoder below
    except (PngError, J.JpegError):
        return None
    if planned is not None:
        return _decoder(planned[0], device).decode_planned([planned[1]], bgr=bgr)[0]
    from .datasets import default_imread
    frame = default_imread()(os.fspath(path))
    if frame is None:
        return None
    dev = _cabi.Handle.cuda_device("cuda" if device is None else device, "imread needs a GPU device", resolve=True)
    return torch.from_numpy(np.ascontiguousarray(frame if bgr else frame[:, :, ::-1])).to(dev)


def _check_path(path):
    _imwrite.check_extension(path, (".png",), "imwrite")


def imwrite(path, img, params=None, *, scale=1.0, rounding="nearest", bgr=True, compression="fixed", device=None):
    """cv2.imwrite for .png: a device tensor or a numpy array, (H, W) or (H, W, C), channels in cv2's B, G, R(, A) order.  params is
    accepted and ignored (cv2's compression level has no counterpart; `compression` chooses between the two block kinds).  A numpy
    array goes to `device` (default: the current GPU).  Returns True; raises ValueError naming the extension for anything but .png."""
    return imwrite_batch([path], [img], scale=scale, rounding=rounding, bgr=bgr, compression=compression, device=device)


def imwrite_batch(paths, images, *, scale=1.0, rounding="nearest", bgr=True, compression="fixed", device=None, threads=None):
    """imwrite for many files: ONE device call for all images, then the files are written from a thread pool (at most WRITE_THREADS)."""
    return _imwrite.imwrite_batch(PNGEncoder, _check_path, paths, images, device, threads, scale=scale, rounding=rounding, bgr=bgr, compression=compression)
