"""Baseline JPEG decoding, split between host and device (include/tokenhmr_hip.h; csrc/jpeg.hip, jpeg_host.h, jpeg_math.h).

    info = probe(data)                                   # size, components, sampling, restart interval — no device
    item = entropy_decode(data, window=(x0, y0, w, h))   # host: markers + Huffman -> quantised blocks of the window (releases the GIL)
    frames = JpegDecoder("cuda:0").decode([data, ...], windows=[...], bgr=True)       # device uint8 (win_h, win_w, 3) tensors
    frame = decode_host(data, window=None, bgr=True)     # the same arithmetic on the CPU: numpy (h, w, 3) uint8

The pixels are libjpeg's default pipeline bit for bit (JDCT_ISLOW, fancy upsampling, fixed-point YCbCr -> RGB): what PIL and cv2.imread
give.  A file of a kind the decoder does not handle (progressive, arithmetic, CMYK, ...) raises JpegUnsupported — callers fall back to
their host decoder for that file; a malformed one raises JpegError.

Baseline JPEG encoding of device images, the drop-in for cv2.imwrite(".jpg") (csrc/jpegenc.hip, jpegenc_host.h, jpegenc_math.h):

    imwrite("frame.jpg", frame)                          # device tensor or numpy array, (H, W), (H, W, 1 | 3 | 4); BGR(A) like cv2; q 95, 4:2:0
    imwrite_batch(paths, frames, quality=90)             # ONE device call, the files written from a small thread pool
    files = JpegEncoder("cuda:0").encode([a, b, ...], quality=[95, 50, ...], subsampling="4:4:4", bgr=False)      # list[bytes]
    data = encode_host(array, quality=75)                # the same bytes on the CPU (thmr_jpeg_encode_host)

The file is the one libjpeg-turbo writes for the same pixels (Pillow's save(format="JPEG", quality=q, subsampling=s)), byte for byte:
baseline JFIF, Annex-K Huffman tables, no restart markers.  optimize=True (per image in encode / imwrite_batch; cv2's
params=[IMWRITE_JPEG_OPTIMIZE, 1] in imwrite) codes an image with Huffman tables made from its own statistics — libjpeg's
optimize_coding, Pillow's save(..., optimize=True), again byte for byte: smaller files, the same pixels, a little more device time.  Samples are converted as png.py converts them
(`scale`, `rounding`); the alpha of a 4-channel image is dropped, as cv2 does.  "4:2:2" is refused by name.
"""
import ctypes as C

import numpy as np
import torch

from . import _cabi, _imwrite


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


# ---- encoding ----
_SUBSAMPLING = {"4:4:4": _cabi.JPEG_444, "4:2:2": _cabi.JPEG_422, "4:2:0": _cabi.JPEG_420}
IMWRITE_JPEG_QUALITY, IMWRITE_JPEG_OPTIMIZE = 1, 3          # cv2's flags, the two imwrite honours


def encode_bound(width, height, channels, subsampling="4:2:0", lib=None, optimize=False):
    """The largest file the encoder writes for an image of this size (0 for arguments it refuses).  optimize: the bound of that mode,
    one bit per block more (a DC code of an image's own table can take 12 bits)."""
    lib = lib or _cabi.load()
    if not optimize:
        return int(lib.thmr_jpeg_encode_bound(int(width), int(height), int(channels), _subsampling(subsampling)))
    return int(lib.thmr_jpeg_encode_bound_flags(int(width), int(height), int(channels), _subsampling(subsampling), _cabi.JPEG_OPTIMIZE))


def _subsampling(s):
    if s not in _SUBSAMPLING:
        raise ValueError(f"subsampling must be '4:4:4' or '4:2:0' ('4:2:2' is refused by the encoder), got {s!r}")
    return _SUBSAMPLING[s]


def _quality(q):
    if isinstance(q, bool) or not isinstance(q, (int, np.integer)):
        raise ValueError(f"quality must be an integer 1 ... 100, got {q!r}")
    return int(q)


def _fill(item, img, scale, rounding, bgr, what="image"):
    return _imwrite.fill_item(item, img, scale, rounding, bgr, error=JpegError, what=what)


def _flags(optimize):
    if not isinstance(optimize, (bool, np.bool_)):
        raise ValueError(f"optimize must be True or False, got {optimize!r}")
    return _cabi.JPEG_OPTIMIZE if optimize else 0


def _out(item, h, w, c, sub, lib, capacity=None, flags=0):
    return _imwrite.out_buffer(item, lib.thmr_jpeg_encode_bound_flags(w, h, c, sub, flags) if capacity is None else capacity)


def encode_host(img, *, quality=95, subsampling="4:2:0", optimize=False, scale=1.0, rounding="nearest", bgr=True, capacity=None, flags=None, lib=None):
    """One numpy image -> the file's bytes, on the CPU with the kernels' arithmetic: the oracle of JpegEncoder, and what a caller without
    a device gets.  optimize: Huffman tables from the image's own statistics (Pillow's optimize=True).  capacity: the output buffer's
    size (default the mode's bound) and flags: the raw flag word instead of `optimize` — both for the refusal tests."""
    lib = lib or _cabi.load()
    img = np.asarray(img)
    item = _cabi.PngItem()
    q, sub = _quality(quality), _subsampling(subsampling)
    flags = _flags(optimize) if flags is None else int(flags)
    h, w, c = _fill(item, img, scale, rounding, bgr)
    item.pixels = img.ctypes.data
    buf = _out(item, h, w, c, sub, lib, capacity, flags & _cabi.JPEG_OPTIMIZE)
    rc = lib.thmr_jpeg_encode_host_flags(C.byref(item), q, sub, flags)
    if rc != 0:
        _cabi.raise_error(rc, "thmr_jpeg_encode_host_flags", lib.thmr_jpeg_encoder_last_error(None), JpegError, _BY_CODE)
    return buf[:item.written].tobytes()


def symbol_histogram(img, *, quality=95, subsampling="4:2:0", scale=1.0, rounding="nearest", bgr=True, lib=None):
    """The statistics encode_host(optimize=True) builds the image's tables from (thmr_jpeg_histogram_host): int32 (4, 256), the
    frequency of every symbol of the tables DC0, AC0, DC1, AC1 — DC categories 0 ... 11, AC run << 4 | size with ZRL 0xF0 and EOB 0."""
    lib = lib or _cabi.load()
    img = np.asarray(img)
    item = _cabi.PngItem()
    h, w, c = _fill(item, img, scale, rounding, bgr)
    item.pixels = img.ctypes.data
    freq = np.zeros((4, 256), dtype=np.int32)
    rc = lib.thmr_jpeg_histogram_host(C.byref(item), _quality(quality), _subsampling(subsampling), C.c_void_p(freq.ctypes.data))
    if rc != 0:
        _cabi.raise_error(rc, "thmr_jpeg_histogram_host", lib.thmr_jpeg_encoder_last_error(None), JpegError, _BY_CODE)
    return freq


def optimal_table(freq, lib=None):
    """thmr_jpeg_optimal_table, the routine of the table kernel: 256 frequencies by symbol -> (bits, huffval).  bits: uint8 (17,),
    bits[1:] the codes per length 1 ... 16 as a DHT segment holds them, bits[0] the longest code size BEFORE the limit to 16 (above 16:
    libjpeg's adjustment ran); huffval: the symbols in use in code order."""
    lib = lib or _cabi.load()
    freq = np.ascontiguousarray(freq, dtype=np.int32)
    if freq.shape != (256,):
        raise ValueError(f"freq must hold 256 frequencies, got shape {freq.shape}")
    bits, huffval, nsym = np.zeros(17, np.uint8), np.zeros(256, np.uint8), C.c_int32(0)
    rc = lib.thmr_jpeg_optimal_table(C.c_void_p(freq.ctypes.data), C.c_void_p(bits.ctypes.data), C.c_void_p(huffval.ctypes.data), C.cast(C.byref(nsym), C.c_void_p))
    if rc != 0:
        _cabi.raise_error(rc, "thmr_jpeg_optimal_table", lib.thmr_jpeg_encoder_last_error(None), JpegError, _BY_CODE)
    return bits, huffval[:nsym.value].copy()


class JpegEncoder(_cabi.Handle):
    """Owns a thmr_jpeg_encoder handle: grow-only device scratch and pinned staging, and a grow-only host buffer the files of a call are
    written into before they become bytes (the bound of a frame is tens of MB: allocated once, not per call).  One stream at a time;
    encode() synchronises it."""
    error, error_by_code = JpegError, _BY_CODE

    def __init__(self, device="cuda:0"):
        super().__init__(device, "thmr_jpeg_encoder", "JpegEncoder needs a GPU device; encode_host() is the CPU encode")
        self._files = np.empty(0, dtype=np.uint8)
        self._open(self._index())

    def encode(self, images, *, quality=95, subsampling="4:2:0", optimize=False, scale=1.0, rounding="nearest", bgr=True):
        """A list of images — device tensors, or host tensors / numpy arrays (uploaded) — of any sizes, dtypes and strides -> the files,
        list[bytes], in ONE batch call on the current stream.  quality (1 ... 100), subsampling ("4:4:4", "4:2:0") and optimize (Huffman
        tables from the image's own statistics, built on the device) hold for all images, or are lists with one entry per image.  bgr:
        the images hold B, G, R(, A) like cv2's; False: R, G, B(, A)."""
        n = len(images)
        qs = [_quality(q) for q in _imwrite.per_image(quality, n, "quality settings")]
        subs = [_subsampling(s) for s in _imwrite.per_image(subsampling, n, "subsampling settings")]
        fls = [_flags(o) for o in _imwrite.per_image(optimize, n, "optimize settings")]
        if n == 0:
            return []
        items = (_cabi.PngItem * n)()
        keep, at, total = [], [], 0
        for i, img in enumerate(images):
            img = _imwrite.to_device_image(img, i, self.device, JpegError, JpegUnsupported)
            h, w, c = _fill(items[i], img, scale, rounding, bgr, f"image {i}")
            items[i].pixels = img.data_ptr()
            keep.append(img)
            bound = self.lib.thmr_jpeg_encode_bound_flags(w, h, c, subs[i], fls[i]) if fls[i] else self.lib.thmr_jpeg_encode_bound(w, h, c, subs[i])
            items[i].capacity = int(bound)          # 0 for an image the call refuses: it names it
            at.append(total)
            total += (items[i].capacity + 63) & ~63
        if self._files.size < total:
            self._files = np.empty(total + total // 4, dtype=np.uint8)
        for i in range(n):
            items[i].out = self._files.ctypes.data + at[i]
        qa, sa, fa = (C.c_int32 * n)(*qs), (C.c_int32 * n)(*subs), (C.c_int32 * n)(*fls)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            if any(fls):
                rc = self.lib.thmr_jpeg_encode_batch_flags(self.h, items, qa, sa, fa, n, C.c_void_p(stream.cuda_stream))
            else:               # today's entry point, today's launches
                rc = self.lib.thmr_jpeg_encode_batch(self.h, items, qa, sa, n, C.c_void_p(stream.cuda_stream))
        self._check(rc, "thmr_jpeg_encode_batch_flags" if any(fls) else "thmr_jpeg_encode_batch")
        return [self._files[at[i]:at[i] + items[i].written].tobytes() for i in range(n)]


_encoders = _imwrite.encoders          # keyed (encoder class, device): png.py's live in the same cache


def _check_path(path):
    _imwrite.check_extension(path, (".jpg", ".jpeg"), "jpeg.imwrite")


def _params(params, quality, optimize):
    """cv2's params list [flag, value, ...] -> (quality, optimize): IMWRITE_JPEG_QUALITY sets the quality, IMWRITE_JPEG_OPTIMIZE
    optimize = bool(value); any other flag is refused by its number."""
    if params is None:
        return quality, optimize
    params = [int(p) for p in params]
    if len(params) % 2:
        raise ValueError(f"params must hold (flag, value) pairs, got {len(params)} entries")
    for flag, value in zip(params[::2], params[1::2]):
        if flag == IMWRITE_JPEG_OPTIMIZE:
            optimize = bool(value)
        elif flag == IMWRITE_JPEG_QUALITY:
            quality = value
        else:
            raise ValueError(f"params flag {flag} is not supported: jpeg.imwrite honours IMWRITE_JPEG_QUALITY ({IMWRITE_JPEG_QUALITY}) and "
                             f"IMWRITE_JPEG_OPTIMIZE ({IMWRITE_JPEG_OPTIMIZE}) only")
    return quality, optimize


def _params_quality(params, quality):
    """The quality of a params list alone."""
    return _params(params, quality, False)[0]


def imwrite(path, img, params=None, *, quality=95, subsampling="4:2:0", optimize=False, scale=1.0, rounding="nearest", bgr=True, device=None):
    """cv2.imwrite for .jpg / .jpeg: a device tensor or a numpy array, (H, W) or (H, W, C), channels in cv2's B, G, R(, A) order; the
    defaults are cv2's (quality 95, 4:2:0, no optimisation).  params=[cv2.IMWRITE_JPEG_QUALITY, q] and [cv2.IMWRITE_JPEG_OPTIMIZE, v]
    are honoured, alone or together; any other flag raises ValueError naming it, and so does any other extension.  A numpy array goes
    to `device` (default: the current GPU).  Returns True."""
    _check_path(path)
    quality, optimize = _params(params, quality, optimize)
    return imwrite_batch([path], [img], quality=quality, subsampling=subsampling, optimize=optimize, scale=scale, rounding=rounding, bgr=bgr, device=device)


def imwrite_batch(paths, images, *, quality=95, subsampling="4:2:0", optimize=False, scale=1.0, rounding="nearest", bgr=True, device=None, threads=None):
    """imwrite for many files: ONE device call for all images, then the files are written from a thread pool (at most png.WRITE_THREADS)."""
    return _imwrite.imwrite_batch(JpegEncoder, _check_path, paths, images, device, threads, quality=quality, subsampling=subsampling, optimize=optimize,
                                  scale=scale, rounding=rounding, bgr=bgr)
