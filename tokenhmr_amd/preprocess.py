"""Crop preprocessing on the GPU — drop-in for the reference's per-crop CPU code.

    from tokenhmr_amd.preprocess import ViTDetDataset          # instead of lib.datasets.vitdet_dataset.ViTDetDataset (demo.py:71)
    batch = ViTDetDataset(model_cfg, img_cv2, boxes, device="cuda:0").batch()      # == next(iter(DataLoader(dataset, ...)))
    out = model(batch)

`ViTDetDataset` mirrors tokenhmr/lib/datasets/vitdet_dataset.py:16-88: same constructor arguments, `len()`, `ds[i]` items with
the same keys ('img', 'personid', 'box_center', 'box_size', 'img_size'), plus `.batch()` which produces all crops of the frame
in ONE GPU call, already collated and resident on the device.  `crop_examples` is the same for the eval.py crop
(`get_example` without augmentation, lib/datasets/utils.py:501-638).

The box -> affine arithmetic (3 points, float32, lib/datasets/utils.py:81-128 + cv2.getAffineTransform) runs here on the host
in numpy; warp, anti-alias blur, channel flip and normalisation run in csrc/crop.hip through the C ABI (thmr_cropper_run).
torch is used only to hold device memory.  There is no CPU fallback.

`Cropper.warp_frames` is the eval.py shape: B items from B frames of B sizes, one crop each, in ONE call
(thmr_cropper_run_frames), uploading only the window of each frame its crop can touch (`source_window`).
"""
import ctypes as C

import numpy as np
import torch

from . import _cabi

DEFAULT_MEAN = (0.485, 0.456, 0.406)
DEFAULT_STD = (0.229, 0.224, 0.225)


def get_affine_transform(src, dst):
    """cv2.getAffineTransform: the affine map through three point pairs (6x6 system, LU, double)."""
    src = np.asarray(src, dtype=np.float32).astype(np.float64)
    dst = np.asarray(dst, dtype=np.float32).astype(np.float64)
    A = np.zeros((6, 6))
    b = np.zeros(6)
    for i in range(3):
        A[2 * i, 0:3] = (src[i, 0], src[i, 1], 1.0)
        A[2 * i + 1, 3:6] = (src[i, 0], src[i, 1], 1.0)
        b[2 * i], b[2 * i + 1] = dst[i]
    return np.linalg.solve(A, b).reshape(2, 3)


def gen_trans_from_patch_cv(c_x, c_y, src_width, src_height, dst_width, dst_height, scale=1.0, rot=0.0):
    """lib/datasets/utils.py:81-128 — centre, centre+down, centre+right of the box mapped onto the patch (float32 points)."""
    f32 = np.float32
    rad = np.pi * rot / 180
    sn, cs = np.sin(rad), np.cos(rad)

    def rot2(v):
        return np.array([v[0] * cs - v[1] * sn, v[0] * sn + v[1] * cs], dtype=f32)

    center = np.array([c_x, c_y], dtype=np.float64)
    down = rot2(np.array([0, src_height * scale * 0.5], dtype=f32))
    right = rot2(np.array([src_width * scale * 0.5, 0], dtype=f32))
    src = np.stack([center, center + down, center + right]).astype(f32)
    dc = np.array([dst_width * 0.5, dst_height * 0.5], dtype=f32)
    dst = np.stack([dc, dc + np.array([0, dst_height * 0.5], dtype=f32), dc + np.array([dst_width * 0.5, 0], dtype=f32)]).astype(f32)
    return get_affine_transform(src, dst)


def expand_to_aspect_ratio(input_shape, target_aspect_ratio=None):
    """lib/datasets/utils.py:14-33.  w, h are numpy float32 scalars and w_t, h_t Python ints; under the numpy the reference
    pins (1.23.1, legacy scalar promotion) `w * h_t / w_t` is evaluated in float64, so the expanded side — and with it the
    bbox size, the anti-alias sigma and the affine — is a double-precision function of the float32 box.  Python floats
    reproduce exactly that (verified against the reference's code run under numpy 1.26: tests/golden/crop_numpy1.npz)."""
    if target_aspect_ratio is None:
        return input_shape
    w, h = input_shape
    w_t, h_t = target_aspect_ratio
    if h / w < h_t / w_t:
        return np.array([w, max(float(w) * h_t / w_t, h)])
    return np.array([max(float(h) * w_t / h_t, w), h])


def source_window(M, patch, H, W, sigma=0.0, truncate=3.0):
    """The box of frame texels a crop can touch — (x0, y0, w, h), or None when every output pixel is border — as
    thmr_cropper_run_frames computes it (include/tokenhmr_hip.h), restated in Python floats (IEEE double, no fused operations) and
    integers: the fixed-point source coordinate of the four patch corners, [lo - 1, hi + 2] on each axis, clipped to the frame; for a
    blurred crop (sigma > 1e-15) widened by the kernel radius int(truncate * sigma + 0.5) on all four sides, clipped again.
    Raises ValueError where the C side refuses the crop itself (singular affine, bad sigma / truncate, a blur radius above 4096)."""
    m = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(6)]
    sigma, truncate, patch, H, W = float(sigma), float(truncate), int(patch), int(H), int(W)
    # cv::warpAffine: invert the forward 2x3 matrix in double
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11; m[1] *= -D; m[3] *= -D; m[4] = A22
    b1, b2 = -m[0] * m[2] - m[1] * m[5], -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    if not all(np.isfinite(m)):
        raise ValueError("singular or non-finite affine")
    if not (sigma >= 0) or not np.isfinite(sigma) or not (truncate > 0):
        raise ValueError("bad sigma / truncate")
    xs, ys = [], []
    for y in (0.0, float(patch - 1)):
        for x in (0.0, float(patch - 1)):
            xs.append((round((m[1] * y + m[2]) * 1024.0) + 16 + round(m[0] * x * 1024.0)) >> 10)        # round(): half to even, as llrint
            ys.append((round((m[4] * y + m[5]) * 1024.0) + 16 + round(m[3] * x * 1024.0)) >> 10)
    x0, x1 = max(min(xs) - 1, 0), min(max(xs) + 2, W - 1)
    y0, y1 = max(min(ys) - 1, 0), min(max(ys) + 2, H - 1)
    if x0 > x1 or y0 > y1:
        return None
    if sigma > 1e-15:
        r = truncate * sigma + 0.5
        if not r < 4097.0:                    # inf and NaN included, before int() meets them
            raise ValueError("blur radius too large")
        lw = int(r)
        x0, x1, y0, y1 = max(x0 - lw, 0), min(x1 + lw, W - 1), max(y0 - lw, 0), min(y1 + lw, H - 1)
    return x0, y0, x1 - x0 + 1, y1 - y0 + 1


def _scaled(triple):
    """mean / std of 0 ... 1 pixel values as the kernels take them: float32(255 v), three of them."""
    return (C.c_float * 3)(*[np.float32(255.0 * v) for v in triple])


class _Staging:
    """One set of staging buffers of warp_frames: pinned host bytes, their device twin, and the event behind their last use."""

    def __init__(self):
        self.host = self.dev = self.event = None


class Cropper(_cabi.Handle):
    """Owns a thmr_cropper handle (device scratch for blurred regions) and, for warp_frames, two grow-only sets of staging buffers."""

    def __init__(self, device="cuda:0"):
        super().__init__(device, "thmr_cropper", "Cropper needs a GPU device: the crop kernels have no CPU fallback")
        self._stage, self._turn = (_Staging(), _Staging()), 0
        self.last_staged_bytes = 0
        self._open(self._index())

    def close(self):
        if getattr(self, "h", None):
            for st in self._stage:          # the copies and kernels that read the staging are done before anything is freed
                if st.event is not None:
                    st.event.synchronize()
        super().close()

    def to_device(self, frame):
        """(H, W, 3) uint8 numpy array or tensor -> contiguous device tensor (one H2D copy per frame, shared by its crops)."""
        t = torch.as_tensor(np.ascontiguousarray(frame) if isinstance(frame, np.ndarray) else frame)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("frame must be (H, W, 3) uint8")
        return t.to(self.device).contiguous()

    def warp(self, frame, trans, sigmas=None, truncate=4.0, patch=256, mean=DEFAULT_MEAN, std=DEFAULT_STD, is_bgr=True, out=None):
        """frame (H,W,3) uint8; trans (n,2,3) forward affines as given to cv2.warpAffine; sigmas (n,) anti-alias sigma or 0.
        Returns (n,3,patch,patch) float32 on the device: gaussian -> warpAffine -> [::-1] -> CHW -> (x - 255 mean)/(255 std)."""
        fr = self.to_device(frame)
        trans = np.asarray(trans, dtype=np.float64).reshape(-1, 6)
        n = trans.shape[0]
        sig = np.zeros(n) if sigmas is None else np.asarray(sigmas, dtype=np.float64).reshape(n)
        descs = (_cabi.CropDesc * n)()
        for i in range(n):
            descs[i].M[:] = trans[i].tolist()
            descs[i].sigma, descs[i].truncate = float(sig[i]), float(truncate)
        out = self._out(out, n, patch)
        H, W = int(fr.shape[0]), int(fr.shape[1])
        with torch.cuda.device(self.device):
            rc = self.lib.thmr_cropper_run(self.h, C.c_void_p(fr.data_ptr()), H, W, W * 3, descs, n, int(patch), int(bool(is_bgr)),
                                           _scaled(mean), _scaled(std), C.c_void_p(out.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        self._check(rc, "thmr_cropper_run")
        return out

    def _out(self, out, n, patch):
        """The caller's output tensor, validated, or a fresh one."""
        if out is None:
            return torch.empty(n, 3, patch, patch, device=self.device, dtype=torch.float32)
        if out.shape != (n, 3, patch, patch) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError("out must be a contiguous (n,3,patch,patch) float32 tensor on the cropper's device")
        return out

    @staticmethod
    def _item(it, win_dev, stride, size, win, M, sigma, truncate):
        """Fills one thmr_frame_crop; an empty window carries no pointer."""
        x0, y0, w, h = win
        it.win_dev = win_dev if w * h else None
        it.row_stride, it.H, it.W = stride, int(size[0]), int(size[1])
        it.win_x0, it.win_y0, it.win_w, it.win_h = x0, y0, w, h
        it.M[:] = M.tolist()
        it.sigma, it.truncate = float(sigma), float(truncate)

    def _run_frames(self, items, n, patch, is_bgr, mean, std, out, stream):
        """thmr_cropper_run_frames on `stream` of this device; the caller raises through _check once its own bookkeeping is done."""
        return self.lib.thmr_cropper_run_frames(self.h, items, n, int(patch), int(bool(is_bgr)), _scaled(mean), _scaled(std),
                                                C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream))

    def warp_frames(self, frames, trans, sigmas=None, truncate=3.0, patch=256, mean=DEFAULT_MEAN, std=DEFAULT_STD, is_bgr=True,
                    windows=True, out=None, extra=None):
        """n items from n frames, one crop each, in one call: frames is a list of (H_i, W_i, 3) uint8 arrays (the same array object
        may appear several times), trans (n,2,3) and sigmas (n,) as for `warp`.  Returns (n,3,patch,patch) float32 on the device,
        item i bit-equal to `warp(frames[i], trans[i:i+1], ...)`.
        windows=True uploads of each frame only `source_window` of its crop, windows=False whole frames; a list gives one
        (x0, y0, w, h) or None per item (the C side refuses a window that does not cover what the crop can touch).  Everything is
        packed back to back, each start 256-byte aligned, into one pinned staging buffer and uploaded with ONE non-blocking copy on
        the current stream.  There are two sets of staging buffers, used alternately, so the host may pack the next batch while this
        one's copy is in flight; a set is reused only after the event recorded behind its last use has completed.
        Memory: each of the two sets holds up to 1.25 x the largest batch staged so far, pinned on the host and again on the device,
        until close() — with windows=False at 64 full-HD frames that is 2 x 0.5 GB of each; with windows, 2 x 66 MB.
        extra: a 1-D uint8 array that rides in the same upload (a batch's small host arrays); the call then returns
        (crops, a fresh device copy of those bytes) — fresh, because the staging it arrived in is recycled two calls later."""
        n = len(frames)
        trans = np.asarray(trans, dtype=np.float64).reshape(-1, 6)
        if n == 0 or trans.shape[0] != n:
            raise ValueError("warp_frames needs one affine per frame and at least one frame")
        sig = np.zeros(n) if sigmas is None else np.asarray(sigmas, dtype=np.float64).reshape(n)
        wins, offs, placed, total = [], [], {}, 0
        for i, fr in enumerate(frames):
            if not isinstance(fr, np.ndarray) or fr.dtype != np.uint8 or fr.ndim != 3 or fr.shape[2] != 3:
                raise ValueError(f"frame {i} must be an (H, W, 3) uint8 array")
            H, W = fr.shape[:2]
            if windows is True:
                w = source_window(trans[i], patch, H, W, sig[i], truncate)
            elif windows is False:
                w = (0, 0, W, H)
            else:
                w = windows[i]
            w = (0, 0, 0, 0) if w is None else tuple(int(v) for v in w)
            if w[0] < 0 or w[1] < 0 or w[2] < 0 or w[3] < 0 or w[0] + w[2] > W or w[1] + w[3] > H:
                raise ValueError(f"item {i}: the window {w} does not lie inside the {W}x{H} frame")
            wins.append(w)
            key = (id(fr), w)
            if key not in placed:          # items that share a frame object and a window share its bytes
                placed[key] = total
                total = (total + w[2] * w[3] * 3 + 255) & ~255
            offs.append(placed[key])
        if extra is not None:
            extra = np.ascontiguousarray(extra, dtype=np.uint8).reshape(-1)
            extra_off = total
            total = (total + extra.size + 255) & ~255
        st = self._stage[self._turn]
        self._turn ^= 1
        if st.event is not None:
            st.event.synchronize()         # the copy and the kernels that last read this set are done
        if st.host is None or st.host.numel() < total:
            cap = max(total + total // 4, 1 << 20)          # 25 % headroom: see the docstring for what whole frames cost
            st.host = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
            st.dev = torch.empty(cap, dtype=torch.uint8, device=self.device)
        hbuf = st.host.numpy()
        done = set()
        for i, fr in enumerate(frames):
            (x0, y0, w, h), o = wins[i], offs[i]
            if o in done or w * h == 0:
                continue
            done.add(o)
            hbuf[o:o + w * h * 3].reshape(h, w, 3)[...] = fr[y0:y0 + h, x0:x0 + w]
        if extra is not None:
            hbuf[extra_off:extra_off + extra.size] = extra
        self.last_staged_bytes = total
        items = (_cabi.FrameCrop * n)()
        for i, fr in enumerate(frames):
            self._item(items[i], st.dev.data_ptr() + offs[i], wins[i][2] * 3, fr.shape[:2], wins[i], trans[i], sig[i], truncate)
        out = self._out(out, n, patch)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            if total:
                st.dev[:total].copy_(st.host[:total], non_blocking=True)
            rc = self._run_frames(items, n, patch, is_bgr, mean, std, out, stream)
            extra_dev = st.dev[extra_off:extra_off + extra.size].clone() if extra is not None else None
            if st.event is None:
                st.event = torch.cuda.Event()
            st.event.record(stream)
        self._check(rc, "thmr_cropper_run_frames")
        return out if extra is None else (out, extra_dev)

    def warp_device_windows(self, windows_dev, frame_sizes, wins, trans, sigmas=None, truncate=3.0, patch=256, mean=DEFAULT_MEAN,
                            std=DEFAULT_STD, is_bgr=True, out=None, row_strides=None):
        """`warp_frames` for windows that are ALREADY on the device (tokenhmr_amd.jpeg.JpegDecoder writes them there): windows_dev[i] a
        contiguous uint8 device tensor holding item i's (win_h, win_w, 3) window with row_strides[i] bytes per row (default win_w * 3),
        frame_sizes[i] the (H, W) of its full frame, wins[i] = (x0, y0, w, h) where the window sits in it (None or an empty window: every
        output pixel is border, windows_dev[i] may be None).  Nothing is staged or uploaded but the descriptors; the kernels are enqueued
        on the current stream, behind whatever filled the windows there.  Item i is bit-equal to `warp_frames` on the same pixels."""
        n = len(windows_dev)
        trans = np.asarray(trans, dtype=np.float64).reshape(-1, 6)
        if n == 0 or trans.shape[0] != n or len(frame_sizes) != n or len(wins) != n:
            raise ValueError("warp_device_windows needs one frame size, one window and one affine per item and at least one item")
        sig = np.zeros(n) if sigmas is None else np.asarray(sigmas, dtype=np.float64).reshape(n)
        items = (_cabi.FrameCrop * n)()
        for i in range(n):
            x0, y0, w, h = (0, 0, 0, 0) if wins[i] is None else tuple(int(v) for v in wins[i])
            stride = int(row_strides[i]) if row_strides is not None else w * 3
            t = windows_dev[i]
            if w * h:
                if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.device != self.device or not t.is_contiguous():
                    raise ValueError(f"item {i}: the window must be a contiguous uint8 tensor on {self.device}")
                if t.numel() < (h - 1) * stride + w * 3:
                    raise ValueError(f"item {i}: the tensor holds {t.numel()} bytes, the window needs {(h - 1) * stride + w * 3}")
            self._item(items[i], t.data_ptr() if w * h else None, stride, frame_sizes[i], (x0, y0, w, h), trans[i], sig[i], truncate)
        out = self._out(out, n, patch)
        with torch.cuda.device(self.device):
            rc = self._run_frames(items, n, patch, is_bgr, mean, std, out, torch.cuda.current_stream(self.device))
        self._check(rc, "thmr_cropper_run_frames")
        return out


class ViTDetDataset:
    """Mirror of lib/datasets/vitdet_dataset.py:16-88 (inference only).  cfg needs MODEL.IMAGE_SIZE / IMAGE_MEAN / IMAGE_STD and
    optionally MODEL.BBOX_SHAPE, exactly as the reference reads them."""

    def __init__(self, cfg, img_cv2, boxes, train=False, device="cuda:0", cropper=None, **kwargs):
        assert train is False, "ViTDetDataset is only for inference"
        self.cfg = cfg
        self.img_cv2 = img_cv2
        self.img_size = cfg.MODEL.IMAGE_SIZE
        self.mean_rgb, self.std_rgb = tuple(cfg.MODEL.IMAGE_MEAN), tuple(cfg.MODEL.IMAGE_STD)
        self.mean, self.std = 255.0 * np.array(self.mean_rgb), 255.0 * np.array(self.std_rgb)
        boxes = np.asarray(boxes).astype(np.float32).reshape(-1, 4)
        self.center = (boxes[:, 2:4] + boxes[:, 0:2]) / 2.0
        self.scale = (boxes[:, 2:4] - boxes[:, 0:2]) / 200.0
        self.personid = np.arange(len(boxes), dtype=np.int32)
        self._cropper, self._device = cropper, device       # the GPU handle is created on first use
        self._frame_dev = None
        get = cfg.MODEL.get if hasattr(cfg.MODEL, "get") else (lambda k, d=None: getattr(cfg.MODEL, k, d))
        self.bbox_shape = get("BBOX_SHAPE", None)

    def __len__(self):
        return len(self.personid)

    @property
    def cropper(self):
        if self._cropper is None:
            self._cropper = Cropper(self._device)
        return self._cropper

    def _params(self, idx):
        """vitdet_dataset.py:46-68: bbox size, anti-alias sigma, affine of crop idx."""
        center = self.center[idx].copy()
        bbox_size = expand_to_aspect_ratio(self.scale[idx] * 200, target_aspect_ratio=self.bbox_shape).max()
        # bbox_size is a float32 scalar; the reference's pinned numpy (1.23.1) promotes `bbox_size*1.0` to float64, so the
        # down-sampling factor, sigma and the gaussian weights are double-precision functions of that float32 value
        f = (float(bbox_size) / self.img_size) / 2.0
        sigma = (f - 1) / 2 if f > 1.1 else 0.0
        trans = gen_trans_from_patch_cv(center[0], center[1], bbox_size, bbox_size, self.img_size, self.img_size, 1.0, 0)
        return bbox_size, float(sigma), trans

    def _frame(self):
        if self._frame_dev is None:
            self._frame_dev = self.cropper.to_device(self.img_cv2)
        return self._frame_dev

    def _crops(self, idxs):
        ps = [self._params(i) for i in idxs]
        img = self.cropper.warp(self._frame(), np.stack([p[2] for p in ps]), [p[1] for p in ps], truncate=4.0, patch=self.img_size,
                                mean=self.mean_rgb, std=self.std_rgb, is_bgr=True)
        return img, ps

    def __getitem__(self, idx):
        img, ps = self._crops([idx])
        H, W = self.img_cv2.shape[:2]
        return {"img": img[0], "personid": int(self.personid[idx]), "box_center": self.center[idx].copy(), "box_size": ps[0][0],
                "img_size": 1.0 * np.array([W, H])}

    def batch(self, idxs=None):
        """All (or the given) crops of the frame in one GPU call, collated like torch's default_collate would."""
        idxs = list(range(len(self))) if idxs is None else list(idxs)
        img, ps = self._crops(idxs)
        H, W = self.img_cv2.shape[:2]
        dev = self.cropper.device
        return {"img": img,
                "personid": torch.as_tensor(self.personid[idxs].astype(np.int64), device=dev),
                "box_center": torch.as_tensor(self.center[idxs], device=dev),
                "box_size": torch.as_tensor(np.array([float(p[0]) for p in ps], dtype=np.float64), device=dev),   # float64, as collated under the pinned numpy
                "img_size": torch.as_tensor(np.tile(1.0 * np.array([W, H]), (len(idxs), 1)), device=dev)}


def crop_examples(cropper, cvimg, centers, sizes, patch=256, mean=DEFAULT_MEAN, std=DEFAULT_STD, use_skimage_antialias=False,
                  is_bgr=True):
    """The image part of `get_example` with do_augment=False (lib/datasets/utils.py:501-638) for n boxes of ONE frame:
    centers (n,2), sizes (n,2) = (width, height) of each box.  Returns ((n,3,patch,patch) device tensor, (n,2,3) affines)."""
    centers, sizes = np.asarray(centers, dtype=np.float64).reshape(-1, 2), np.asarray(sizes, dtype=np.float64).reshape(-1, 2)
    trans, sig = [], []
    for (cx, cy), (w, h) in zip(centers, sizes):
        s = 0.0
        if use_skimage_antialias:
            f = patch / (w * 1.0)                      # utils.py:585, as written in the reference
            if f > 1.1:
                s = (f - 1) / 2
        sig.append(s)
        trans.append(gen_trans_from_patch_cv(cx, cy, w, h, patch, patch, 1.0, 0))
    trans = np.stack(trans)
    return cropper.warp(cvimg, trans, sig, truncate=3.0, patch=patch, mean=mean, std=std, is_bgr=is_bgr), trans
