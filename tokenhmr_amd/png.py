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
"""
import ctypes as C

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
