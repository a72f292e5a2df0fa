"""What the two image writers (png.py, jpeg.py) share: both describe an image by a thmr_png_item (include/tokenhmr_hip.h), upload host
images the same way, keep one encoder per device and write their files from the same small thread pool."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _cabi

ROUNDING = {"nearest": _cabi.PNG_ROUND_NEAREST, "trunc": _cabi.PNG_ROUND_TRUNC}
COMPRESSION = {"fixed": _cabi.PNG_FIXED, "dynamic": _cabi.PNG_DYNAMIC}
DTYPES = {torch.uint8: _cabi.PNG_U8, torch.float32: _cabi.PNG_F32, np.dtype(np.uint8): _cabi.PNG_U8, np.dtype(np.float32): _cabi.PNG_F32,
          np.dtype(np.uint16): _cabi.PNG_U16}
if hasattr(torch, "uint16"):
    DTYPES[torch.uint16] = _cabi.PNG_U16
WRITE_THREADS = 16      # what one command gets on the GPU boxes, whatever os.cpu_count() says of the whole machine


def fill_item(item, img, scale, rounding, bgr, compression="fixed", *, error=_cabi.EngineError, what=None):
    """One image -> the fields of a thmr_png_item but the pointers; returns (height, width, channels) as the facade sees them.
    error: the class raised for a dtype no encoder reads; what: names the image in that message."""
    if rounding not in ROUNDING:
        raise ValueError(f"rounding must be 'nearest' or 'trunc', got {rounding!r}")
    if not isinstance(compression, str) or compression not in COMPRESSION:
        raise ValueError(f"compression must be 'fixed' or 'dynamic', got {compression!r}")
    if img.ndim == 2:
        h, w = img.shape
        c, sc = 1, 0
        sy, sx = (img.stride() if isinstance(img, torch.Tensor) else [s // img.itemsize for s in img.strides])
    elif img.ndim == 3:
        h, w, c = img.shape
        sy, sx, sc = (img.stride() if isinstance(img, torch.Tensor) else [s // img.itemsize for s in img.strides])
    else:
        raise ValueError(f"an image is (H, W) or (H, W, C), got shape {tuple(img.shape)}")
    if img.dtype not in DTYPES:
        raise error((f"{what}: " if what else "") + f"dtype must be uint8 or float32, got {img.dtype}")
    item.dtype = DTYPES[img.dtype]
    item.width, item.height, item.channels = int(w), int(h), int(c)
    item.stride_y, item.stride_x, item.stride_c = int(sy), int(sx), int(sc)
    item.scale, item.rounding, item.swap_rb = float(scale), ROUNDING[rounding], int(bool(bgr))
    item.compression = COMPRESSION[compression]
    return int(h), int(w), int(c)


def out_buffer(item, capacity):
    """A host buffer of `capacity` bytes as the item's output."""
    buf = np.empty(max(int(capacity), 1), dtype=np.uint8)
    item.out, item.capacity = buf.ctypes.data, int(capacity)
    return buf


def to_device_image(img, i, device, error, unsupported):
    """Image i of a batch as a tensor on `device`: a numpy array is uploaded (float64, what 255 * img gives in demo.py, as the float32
    the device reads), a tensor elsewhere is moved.  A numpy dtype no encoder reads raises `error`, 16-bit samples `unsupported`."""
    if isinstance(img, np.ndarray):
        if img.dtype == np.float64:
            img = img.astype(np.float32)
        if img.dtype not in DTYPES or DTYPES[img.dtype] == _cabi.PNG_U16:
            raise (unsupported if img.dtype == np.uint16 else error)(
                f"image {i}: dtype must be uint8 or float32, got {img.dtype}" + (" (16-bit samples are unsupported)" if img.dtype == np.uint16 else ""))
        img = torch.from_numpy(np.ascontiguousarray(img))
    return img if img.device == device else img.to(device)


def per_image(value, n, what):
    """One setting for all images, or a list with one per image.  what: the plural that names the settings in the refusal."""
    if isinstance(value, (list, tuple)):
        if len(value) != n:
            raise ValueError(f"{len(value)} {what} for {n} images")
        return list(value)
    return [value] * n


def device_of(images, device):
    if device is not None:
        return device
    for img in images:
        if isinstance(img, torch.Tensor) and img.device.type == "cuda":
            return img.device
    return "cuda"


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)


def write_files(paths, files, threads=None):
    """The files go out from a thread pool (at most WRITE_THREADS); one file is written here."""
    if len(paths) == 1:
        return _write(paths[0], files[0])
    with ThreadPoolExecutor(max(1, min(WRITE_THREADS if threads is None else int(threads), len(paths)))) as pool:
        list(pool.map(_write, paths, files))


encoders = {}       # (encoder class, device) -> the encoder imwrite uses there


def encoder(cls, device):
    device = _cabi.Handle.cuda_device(device, "imwrite needs a GPU device; encode_host() is the CPU encode", resolve=True)
    if (cls, device) not in encoders:
        encoders[(cls, device)] = cls(device)
    return encoders[(cls, device)]


def check_extension(path, extensions, who):
    ext = os.path.splitext(os.fspath(path))[1]
    if ext.lower() not in extensions:
        raise ValueError(f"{who} writes {' / '.join(extensions)} files only, got extension {ext!r} ({os.fspath(path)!r})")


def imwrite_batch(cls, check_path, paths, images, device, threads, **encode):
    """The body of both modules' imwrite and imwrite_batch: every path is checked before a device is asked for, ONE encode call on the
    images' device (cls.encode(images, **encode)), then the files are written."""
    paths = list(paths)
    if len(paths) != len(images):
        raise ValueError(f"{len(paths)} paths for {len(images)} images")
    for p in paths:
        check_path(p)
    if paths:
        write_files(paths, encoder(cls, device_of(images, device)).encode(list(images), **encode), threads)
    return True
