"""Baseline JPEG decoding, split between host and device (include/tokenhmr_hip.h; csrc/jpeg.hip, jpeg_host.h, jpeg_math.h).

    info = probe(data)                                   # size, components, sampling, restart interval — no device
    item = entropy_decode(data, window=(x0, y0, w, h))   # host: markers + Huffman -> quantised blocks of the window (releases the GIL)
    frames = JpegDecoder("cuda:0").decode([data, ...], windows=[...], bgr=True)       # device uint8 (win_h, win_w, 3) tensors
    frame = decode_host(data, window=None, bgr=True)     # the same arithmetic on the CPU: numpy (h, w, 3) uint8

The pixels are libjpeg's default pipeline bit for bit (JDCT_ISLOW, fancy upsampling, fixed-point YCbCr -> RGB): what PIL and cv2.imread
give.  A file of a kind the decoder does not handle (progressive, arithmetic, CMYK, ...) raises JpegUnsupported — callers fall back to
their host decoder for that file; a malformed one raises JpegError.
"""
import ctypes as C

import numpy as np
import torch

from . import _cabi


class JpegError(_cabi.EngineError):
    """A malformed file or a refused argument (THMR_ERR_INVALID), or a HIP failure."""


class JpegUnsupported(JpegError):
    """A well-formed file of a kind the decoder does not handle (THMR_ERR_UNSUPPORTED); the message names what was found."""


_BY_CODE = {_cabi.ERR_UNSUPPORTED: JpegUnsupported}


def _raise(lib, rc, what):
    _cabi.raise_error(rc, what, lib.thmr_jpeg_last_error(None), JpegError, _BY_CODE)


def _buf(data):
    """bytes-like -> (object that keeps the memory alive, address, length) without a copy where the buffer allows it."""
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    return a, a.ctypes.data, a.size


def _window(window):
    if window is None:
        return None
    return (C.c_int32 * 4)(*[int(v) for v in window])


def probe(data, lib=None):
    """dict(height, width, components, h_samp, v_samp, restart_interval) of a supported file; JpegUnsupported / JpegError otherwise."""
    lib = lib or _cabi.load()
    keep, ptr, n = _buf(data)
    info = _cabi.JpegInfo()
    rc = lib.thmr_jpeg_probe(C.c_void_p(ptr), n, C.byref(info))
    if rc != 0:
        _raise(lib, rc, "thmr_jpeg_probe")
    return {k: int(getattr(info, k)) for k in ("height", "width", "components", "h_samp", "v_samp", "restart_interval")}


class PlannedItem:
    """One entropy-decoded window: `coef` (n_blocks, 64) int16 quantised coefficients in natural order, `plan` the _cabi.JpegPlan that
    says which blocks they are, `window` (x0, y0, w, h) and `size` (H, W) of the frame."""

    __slots__ = ("coef", "plan", "window", "size")

    def __init__(self, coef, plan, window, size):
        self.coef, self.plan, self.window, self.size = coef, plan, window, size

    @property
    def nbytes(self):
        return self.coef.nbytes


def entropy_decode(data, window=None, lib=None):
    """The host half for one file: parses the markers and Huffman-decodes the MCU rows down to the last one `window` (default: the whole
    frame) needs, keeping the blocks that cover it.  Thread-safe, and the GIL is released while it runs."""
    lib = lib or _cabi.load()
    keep, ptr, n = _buf(data)
    win = _window(window)
    plan = _cabi.JpegPlan()
    rc = lib.thmr_jpeg_entropy_decode(C.c_void_p(ptr), n, win, None, 0, C.byref(plan))         # the size first
    if rc != 0:
        _raise(lib, rc, "thmr_jpeg_entropy_decode")
    coef = np.empty((plan.n_blocks, 64), dtype=np.int16)
    rc = lib.thmr_jpeg_entropy_decode(C.c_void_p(ptr), n, win, C.c_void_p(coef.ctypes.data), plan.n_blocks, C.byref(plan))
    if rc != 0:
        _raise(lib, rc, "thmr_jpeg_entropy_decode")
    return PlannedItem(coef, plan, (plan.win_x0, plan.win_y0, plan.win_w, plan.win_h), (plan.height, plan.width))


def decode_host(data, window=None, bgr=True, lib=None):
    """The full decode of a window on the CPU (thmr_jpeg_decode_host): (h, w, 3) uint8.  The oracle of the device path, and what a
    caller without a device gets."""
    lib = lib or _cabi.load()
    keep, ptr, n = _buf(data)
    if window is None:
        info = probe(data, lib)
        window = (0, 0, info["width"], info["height"])
    w, h = int(window[2]), int(window[3])
    out = np.empty((h, w, 3), dtype=np.uint8)
    rc = lib.thmr_jpeg_decode_host(C.c_void_p(ptr), n, _window(window), int(bool(bgr)), C.c_void_p(out.ctypes.data), w * 3)
    if rc != 0:
        _raise(lib, rc, "thmr_jpeg_decode_host")
    return out


class JpegDecoder(_cabi.Handle):
    """Owns a thmr_jpeg handle: two grow-only sets of pinned + device staging, used alternately, and the component-plane scratch.
    One stream at a time; a call captured in a graph keeps reading its staging set, so give a captured call a decoder of its own."""
    error, error_by_code = JpegError, _BY_CODE

    def __init__(self, device="cuda:0"):
        super().__init__(device, "thmr_jpeg", "JpegDecoder needs a GPU device; decode_host() is the CPU decode")
        self.last_coef_bytes = 0
        self._open(self._index())

    def decode_planned(self, planned, bgr=True, out=None, row_strides=None):
        """Items already entropy-decoded (in worker threads) -> one device tensor (win_h, win_w, 3) uint8 each, in ONE batch call on the
        current stream.  out: a list of uint8 device tensors to write into instead (1-D or any shape; item i starts at out[i]'s first
        byte) with row_strides[i] bytes per row, default win_w * 3; bytes of a row beyond win_w * 3 are left alone."""
        n = len(planned)
        if n == 0:
            return []
        if out is None:
            out = [torch.empty(p.window[3], p.window[2], 3, dtype=torch.uint8, device=self.device) for p in planned]
        items = (_cabi.JpegItem * n)()
        for i, p in enumerate(planned):
            x0, y0, w, h = p.window
            stride = int(row_strides[i]) if row_strides is not None else w * 3
            o = out[i]
            if o.dtype != torch.uint8 or o.device != self.device or not o.is_contiguous():
                raise ValueError(f"out[{i}] must be a contiguous uint8 tensor on {self.device}")
            if h > 0 and w > 0 and o.numel() < (h - 1) * stride + w * 3:
                raise ValueError(f"out[{i}] holds {o.numel()} bytes, the window needs {(h - 1) * stride + w * 3}")
            it = items[i]
            it.coef = p.coef.ctypes.data if p.coef.size else None
            it.plan = C.pointer(p.plan)
            it.win_x0, it.win_y0, it.win_w, it.win_h = x0, y0, w, h
            it.out_dev = o.data_ptr() if o.numel() else None
            it.row_stride = stride
        self.last_coef_bytes = sum(p.nbytes for p in planned)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            rc = self.lib.thmr_jpeg_decode_batch(self.h, items, n, int(bool(bgr)), C.c_void_p(stream.cuda_stream))
        self._check(rc, "thmr_jpeg_decode_batch")
        return out

    def decode(self, datas, windows=None, bgr=True):
        """A list of JPEG files (bytes) -> a list of device uint8 tensors (win_h, win_w, 3); windows: one (x0, y0, w, h) or None (the
        whole frame) per file.  The entropy decode runs here, one file after the other; use entropy_decode in worker threads and
        decode_planned to overlap it."""
        windows = [None] * len(datas) if windows is None else windows
        return self.decode_planned([entropy_decode(d, w, self.lib) for d, w in zip(datas, windows)], bgr=bgr)
