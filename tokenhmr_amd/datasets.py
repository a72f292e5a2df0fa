"""The evaluation datasets on the device — drop-ins for the reference's `ImageDataset` / `EMDBDataset` and the `DataLoader` around them.

    from tokenhmr_amd.datasets import create_dataset           # instead of lib.datasets.create_dataset (eval.py:123)
    dataset = create_dataset(model_cfg, dataset_cfg, train=False)
    dataloader = dataset.batches(args.batch_size, num_workers=args.num_workers)     # instead of torch.utils.data.DataLoader (eval.py:124)
    for batch in dataloader:            # the reference's batch after default_collate + recursive_to, already resident on the device
        out = model(batch); evaluator(out, batch)

Both classes restate the reference's `__init__` and `__getitem__` with do_augment=False (tokenhmr/lib/datasets/image_dataset.py:56-271,
emdb_dataset.py:25-200, utils.py:501-638) per BATCH instead of per sample:

  host     the .npz arrays, the box -> bbox size -> affine arithmetic and the 44 keypoints (vectorised numpy in the reference's dtypes:
           M.[x, y, 1] in float64 as (M0 x + M1 y) + M2, stored back into the array's dtype, / patch - 0.5 in that dtype);
  device   the crops of the whole batch in ONE call from B frames of B sizes (Cropper.warp_frames -> thmr_cropper_run_frames), of which
           only the window each crop can touch is uploaded; the ground-truth meshes as one thmr_smpl_forward per gender group
           (tokenhmr_amd.smpl.SMPL), scattered back into item order with index_copy_; for EMDB thmr_regress_joints with that group's
           regressor.  Every small host array rides in the same single upload as the frames.

Departures from the reference, stated:
  * `global_orient` passes through unchanged.  The reference sends it through rot_aa(aa, 0), i.e. cv2.Rodrigues there and back
    (utils.py:463-481): the same rotation, but its float rounding and its choice of representative for angles >= pi are not reproduced
    (cv2 stays unpinned).
  * `extra_info` (EMDB) is the list of per-item dicts, not collated.
  * train=True (augmentation) and the other dataset types are refused.
  * Images are decoded by `imread(path) -> (H, W, 3) uint8 BGR`: cv2.imread(path, IMREAD_COLOR | IMREAD_IGNORE_ORIENTATION) where cv2
    imports, else PIL (no EXIF transpose, convert('RGB'), channel-reversed), else ImportError.  Two JPEG decoders (libjpeg versions, IDCT
    choices) may differ by a grey level on some pixels; bit-parity with the reference's crops holds for the same decoded frame.
    That is decode="host", the default.  decode="device" (opt-in) leaves the decode threads only the marker parsing and Huffman decoding
    of a baseline JPEG file, for the window the item's crop reads, and finishes it on the device (tokenhmr_amd/jpeg.py) with libjpeg's
    default arithmetic bit for bit; any other file goes to `imread`, that item alone.  decode="device+png" (opt-in) treats JPEG files
    as "device" does, and a PNG file likewise: the decode threads walk its chunks and inflate the rows the item's window needs, the
    device un-filters and converts them (tokenhmr_amd/png.py), bit-equal to cv2's / Pillow's pixels; a PNG of a kind the decoder does
    not handle (interlaced, 1 / 2 / 4 bits) goes to `imread`, that item alone.
There is no CPU fallback for the device half.
"""
import os
import queue
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import preprocess as PP

MAX_WORKERS = 16      # decode threads: a fixed cap, never derived from the machine's CPU count
DECODE_MODES = ("host", "device", "device+png")
_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def dataset_eval_config(path):
    """The reference's `dataset_eval_config()` (lib/configs/__init__.py:72-85) for a datasets_eval.yaml the caller points to (the
    reference's own file is not shipped): name -> node with TYPE / DATASET_FILE / IMG_DIR / KEYPOINT_LIST / ..."""
    from .model import _read_yaml_cfg
    return _read_yaml_cfg(path, merge=False)[0]


def default_imread():
    """The decoder `imread=None` stands for: cv2 where it imports, else PIL, else ImportError naming both."""
    try:
        import cv2
        flags = cv2.IMREAD_COLOR | cv2.IMREAD_IGNORE_ORIENTATION
        return lambda path: cv2.imread(path, flags)
    except ImportError:
        pass
    try:
        from PIL import Image
    except ImportError:
        raise ImportError("decoding dataset images needs cv2 (opencv-python) or PIL (pillow); neither imports. "
                          "Pass imread=callable(path) -> (H, W, 3) uint8 BGR to use another decoder.") from None

    def pil_imread(path):
        try:
            with Image.open(path) as im:            # no ImageOps.exif_transpose: IMREAD_IGNORE_ORIENTATION
                return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])
        except OSError:
            return None                             # cv2.imread's answer to an unreadable file

    return pil_imread


def _get(node, key, default=None):
    return node.get(key, default) if hasattr(node, "get") else getattr(node, key, default)


class _Pack:
    """Small host arrays laid out back to back (16-byte aligned) in one uint8 buffer, and read back as views of its device copy."""

    def __init__(self):
        self.parts, self.size = [], 0

    def add(self, key, a):
        a = np.ascontiguousarray(a)
        self.parts.append((key, a, self.size))
        self.size = (self.size + a.nbytes + 15) & ~15

    def bytes(self):
        buf = np.zeros(self.size, dtype=np.uint8)
        for _, a, off in self.parts:
            buf[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
        return buf

    def views(self, dev):
        out = {}
        for key, a, off in self.parts:
            dt = torch.from_numpy(np.empty(0, dtype=a.dtype)).dtype
            out[key] = dev[off:off + a.nbytes].view(dt).reshape(a.shape)
        return out


class _EvalDataset:
    """What ImageDataset and EMDBDataset share: the crop, the keypoints, the ground-truth meshes and the batching."""

    kind = ""

    def _init_common(self, cfg, dataset_file, img_dir, train, device, imread, cropper, smpl_male, smpl_female, decode="host"):
        if train:
            raise NotImplementedError("train=True: the device datasets are evaluation-only (augmentation stays with the reference)")
        if decode not in DECODE_MODES:
            raise ValueError(f"decode={decode!r}: the decoders are {DECODE_MODES}")
        self.decode, self._jpeg, self._png = decode, None, None
        self.decode_stats = {"device": 0, "fallback": 0, "coef_bytes": 0}
        self.png_stats = {"device": 0, "fallback": 0, "stream_bytes": 0}          # decode="device+png": the PNG files among the items
        self._png_fallbacks = set()               # items whose PNG file the decoder does not handle (read_item, in the decode threads)
        self.train, self.cfg = False, cfg
        self.img_size = int(cfg.MODEL.IMAGE_SIZE)
        self.mean_rgb, self.std_rgb = tuple(cfg.MODEL.IMAGE_MEAN), tuple(cfg.MODEL.IMAGE_STD)
        self.mean, self.std = 255.0 * np.array(self.mean_rgb), 255.0 * np.array(self.std_rgb)
        self.bbox_shape = _get(cfg.MODEL, "BBOX_SHAPE", None)
        self.img_dir = img_dir
        self.data = np.load(dataset_file, allow_pickle=True)
        self.imgname = self.data["imgname"]
        self.personid = np.zeros(len(self.imgname), dtype=np.int32)
        self.device = torch.device(device)
        self._imread, self._cropper = imread, cropper
        self._smpl_const = {0: smpl_male, 1: smpl_female}
        self._smpl, self._J = {}, {}

    # ---- host half -------------------------------------------------------------------------------------------------------------
    def _load_box(self, divide):
        self.center = self.data["center"]
        self.scale = self.data["scale"].reshape(len(self.center), -1)
        if divide:
            self.scale = self.scale / 200.0
        if self.scale.shape[1] == 1:
            self.scale = np.tile(self.scale, (1, 2))
        assert self.scale.shape == (len(self.center), 2)

    def _load_keypoints_3d(self):
        n = len(self.center)
        try:
            body = self.data["body_keypoints_3d"].astype(np.float32)
        except KeyError:
            body = np.zeros((n, 25, 4), dtype=np.float32)
        try:
            extra = self.data["extra_keypoints_3d"].astype(np.float32)
        except KeyError:
            extra = np.zeros((n, 19, 4), dtype=np.float32)
        body[:, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14], -1] = 0
        self.keypoints_3d = np.concatenate((body, extra), axis=1).astype(np.float32)

    def _load_gender(self):
        try:
            gender = self.data["gender"]
            self.gender = np.array([0 if str(g) == "m" or str(g) == "male" else 1 for g in gender]).astype(np.int32)
            return True
        except KeyError:
            self.gender = -1 * np.ones(len(self.imgname)).astype(np.int32)
            return False

    def __len__(self):
        return len(self.scale)

    def _names(self, idxs):
        rel = []
        for i in idxs:
            try:
                rel.append(self.imgname[i].decode("utf-8"))
            except AttributeError:
                rel.append(str(self.imgname[i]))
        return rel, [os.path.join(self.img_dir, r) for r in rel]

    def read_frame(self, i):
        """The decoded frame of item i: (H, W, 3) uint8 BGR."""
        if self._imread is None:
            self._imread = default_imread()
        path = self._names([i])[1][0]
        fr = self._imread(path)
        if not isinstance(fr, np.ndarray):
            raise IOError("Fail to read %s" % path)
        if fr.dtype != np.uint8 or fr.ndim != 3 or fr.shape[2] != 3:
            raise ValueError(f"imread({path!r}) must give an (H, W, 3) uint8 BGR array, got {fr.dtype} {fr.shape}")
        return fr

    def _item_window(self, i, H, W):
        """The window of its (H, W) frame that item i's crop can touch — what `warp_frames` uploads of it — or the whole frame with
        windows=False; (0, 0, 0, 0) when every output pixel is border."""
        if self.windows is False:
            return (0, 0, W, H)
        s, c, P = self.scale[i], self.center[i], self.img_size
        b = PP.expand_to_aspect_ratio(s * 200, target_aspect_ratio=self.bbox_shape).max()
        w = PP.source_window(PP.gen_trans_from_patch_cv(c[0], c[1], b, b, P, P, 1.0, 0), P, H, W, 0.0, 3.0)
        return (0, 0, 0, 0) if w is None else w

    def read_item(self, i):
        """What the decode threads produce for item i.  decode="host": the decoded frame (read_frame).  decode="device": the file's
        bytes are read, probed and entropy-decoded for the item's window only (tokenhmr_amd.jpeg.entropy_decode: ctypes releases the
        GIL) -> a PlannedItem the batch call finishes on the device; a file that is no JPEG, or a JPEG of a kind the decoder does not
        handle, is decoded by `imread` instead (that item alone, counted in decode_stats["fallback"]); a malformed JPEG raises what an
        unreadable file raises.  decode="device+png": a file with the PNG signature is probed and inflated for the item's window
        (tokenhmr_amd.png.inflate_window) -> a PlannedPng; an unsupported PNG goes to `imread`, a malformed one raises likewise."""
        if self.decode == "host":
            return self.read_frame(i)
        from . import jpeg as J
        path = self._names([i])[1][0]
        try:
            with open(path, "rb") as f:
                data = f.read()
        except OSError:
            raise IOError("Fail to read %s" % path) from None
        if data[:2] == b"\xff\xd8":
            try:
                info = J.probe(data)
                return J.entropy_decode(data, self._item_window(int(i), info["height"], info["width"]))
            except J.JpegUnsupported:
                pass
            except J.JpegError:
                raise IOError("Fail to read %s" % path) from None
        elif self.decode == "device+png" and data[:8] == _PNG_SIGNATURE:
            from . import png as P
            try:
                info = P.probe(data)
                return P.inflate_window(data, self._item_window(int(i), info["height"], info["width"]))
            except P.PngUnsupported:
                self._png_fallbacks.add(int(i))
            except P.PngError:
                raise IOError("Fail to read %s" % path) from None
        return self.read_frame(i)

    def host_batch(self, idxs, sizes):
        """Everything of a batch but the crops and the meshes, as numpy arrays in the dtypes default_collate gives the reference's
        items: `sizes` is the (H, W) of each item's frame.  Returns (arrays, affines (n,2,3), strings)."""
        idxs = [int(i) for i in idxs]
        P = self.img_size
        scale = self.scale[idxs]
        bbox = np.array([PP.expand_to_aspect_ratio(s * 200, target_aspect_ratio=self.bbox_shape).max() for s in scale], dtype=np.float64)
        center = self.center[idxs]
        trans = np.stack([PP.gen_trans_from_patch_cv(c[0], c[1], b, b, P, P, 1.0, 0) for c, b in zip(center, bbox)])
        kp = self.keypoints_2d[idxs].copy()
        x, y = kp[:, :, 0].astype(np.float64), kp[:, :, 1].astype(np.float64)
        M = trans.reshape(-1, 1, 6)
        kp[:, :, 0] = (M[:, :, 0] * x + M[:, :, 1] * y) + M[:, :, 2]            # trans_point2d, rounded into the array's dtype
        kp[:, :, 1] = (M[:, :, 3] * x + M[:, :, 4] * y) + M[:, :, 5]
        kp[:, :, :-1] = kp[:, :, :-1] / P - 0.5
        body_pose = self.body_pose[idxs].astype(np.float32)
        hbp, hb = self.has_body_pose[idxs], self.has_betas[idxs]
        n = len(idxs)
        a = {"keypoints_2d": kp.astype(np.float32),
             "orig_keypoints_2d": self.keypoints_2d[idxs].copy(),
             "box_center": center.copy(),
             "box_size": bbox,
             "bbox_expand_factor": bbox / (scale * 200).max(axis=1),
             "img_size": 1.0 * np.array([[w, h] for h, w in sizes], dtype=np.int64).reshape(n, 2),
             "smpl_params": {"global_orient": body_pose[:, :3].copy(), "body_pose": body_pose[:, 3:].copy(),
                             "betas": self.betas[idxs].astype(np.float32)},
             "has_smpl_params": {"global_orient": hbp.copy(), "body_pose": hbp.copy(), "betas": hb.copy()},
             "smpl_params_is_axis_angle": {"global_orient": np.ones(n, dtype=bool), "body_pose": np.ones(n, dtype=bool),
                                           "betas": np.zeros(n, dtype=bool)},
             "personid": self.personid[idxs].astype(np.int64),
             "idx": np.array(idxs, dtype=np.int64),
             "_scale": scale.copy()}
        rel, full = self._names(idxs)
        strings = {"imgname": full, "imgname_rel": rel}
        self._host_extra(idxs, a, strings)
        return a, trans, strings

    # ---- device half -----------------------------------------------------------------------------------------------------------
    @property
    def cropper(self):
        if self._cropper is None:
            self._cropper = PP.Cropper(self.device)
            self.device = self._cropper.device
        return self._cropper

    @property
    def jpeg_decoder(self):
        if self._jpeg is None:
            from .jpeg import JpegDecoder
            self._jpeg = JpegDecoder(self.cropper.device)
        return self._jpeg

    @property
    def png_decoder(self):
        if self._png is None:
            from .png import PNGDecoder
            self._png = PNGDecoder(self.cropper.device)
        return self._png

    def _crops_from_items(self, idxs, items, trans, extra):
        """decode="device": the windows of the entropy-decoded items are finished on the device by ONE thmr_jpeg_decode_batch, the
        windows of the items `imread` decoded are uploaded, and one thmr_cropper_run_frames crops them all — on the current stream.
        decode="device+png": the inflated PNG items are finished by ONE thmr_png_decode_batch beside it, and cropped by the same call."""
        from .png import PlannedPng
        dev = self.cropper.device
        pngs = [k for k, it in enumerate(items) if isinstance(it, PlannedPng)]
        planned = [k for k, it in enumerate(items) if not isinstance(it, (np.ndarray, PlannedPng))]
        wins, sizes, wdev = [None] * len(items), [None] * len(items), [None] * len(items)
        if planned:
            outs = self.jpeg_decoder.decode_planned([items[k] for k in planned], bgr=True)
            for k, o in zip(planned, outs):
                wins[k], sizes[k], wdev[k] = items[k].window, items[k].size, o
            self.decode_stats["coef_bytes"] += self.jpeg_decoder.last_coef_bytes
        if pngs:
            outs = self.png_decoder.decode_planned([items[k] for k in pngs], bgr=True)
            for k, o in zip(pngs, outs):
                wins[k], sizes[k], wdev[k] = items[k].window, items[k].size, o
            self.png_stats["stream_bytes"] += self.png_decoder.last_row_bytes
        self.png_stats["device"] += len(pngs)
        self.png_stats["fallback"] += sum(1 for i in idxs if int(i) in self._png_fallbacks)
        for k, fr in enumerate(items):
            if isinstance(fr, np.ndarray):
                H, W = fr.shape[:2]
                x0, y0, w, h = self._item_window(idxs[k], H, W)
                wins[k], sizes[k] = (x0, y0, w, h), (H, W)
                if w * h:
                    wdev[k] = torch.from_numpy(np.ascontiguousarray(fr[y0:y0 + h, x0:x0 + w])).to(dev)
        self.decode_stats["device"] += len(planned)
        self.decode_stats["fallback"] += len(items) - len(planned) - len(pngs)
        img = self.cropper.warp_device_windows(wdev, sizes, wins, trans, None, truncate=3.0, patch=self.img_size, mean=self.mean_rgb,
                                               std=self.std_rgb, is_bgr=True)
        return img, torch.from_numpy(extra).to(dev)

    def smpl_constants(self, g):
        """The SMPL constants of gender g (0 male, 1 female): those passed as smpl_male= / smpl_female=, else read — host only — from
        SMPL.MODEL_PATH/SMPL_MALE.pkl / SMPL_FEMALE.pkl, the files smplx.SMPL(model_path=..., gender=...) opens.  As in the reference
        (image_dataset.py:153-157), a literal '${SMPL.DATA_DIR}' in a path is replaced by '' — its quirk, mirrored.  The extra-joint
        regressor (SMPL.JOINT_REGRESSOR_EXTRA) is read when the config names it; the meshes do not need it."""
        if self._smpl_const[g] is None:
            from .smpl_assets import load_smpl_pkl
            smpl_cfg = self.cfg.SMPL
            model_dir = str(smpl_cfg.MODEL_PATH).replace("${SMPL.DATA_DIR}", "")
            j19 = _get(smpl_cfg, "JOINT_REGRESSOR_EXTRA", None)
            j19 = str(j19).replace("${SMPL.DATA_DIR}", "") if j19 else None
            self._smpl_const[g] = load_smpl_pkl(os.path.join(model_dir, "SMPL_MALE.pkl" if g == 0 else "SMPL_FEMALE.pkl"), j19)
        return self._smpl_const[g]

    def _smpl_for(self, g, n):
        """The SMPL handle of gender g (0 male, 1 female) for at least n items: created on first use, re-created larger when needed."""
        from .smpl import SMPL
        m = self._smpl.get(g)
        if m is None or m.max_batch < n:
            const = self.smpl_constants(g)
            if m is not None:
                torch.cuda.current_stream(self.device).synchronize()        # launches may still read the old handle's constants
                m.close()
            m = SMPL(const, max_batch=max(n, 64), device=self.device)
            self._smpl[g] = m
            self._J[g] = const["J_regressor"].detach().float().contiguous().to(self.device)
        return m

    def _meshes(self, batch, genders, joints24):
        """Ground-truth vertices of a batch: one forward per gender group (the reference: gender 1 -> female, anything else -> male),
        rows scattered back into item order."""
        n = len(genders)
        verts = torch.empty(n, 6890, 3, device=self.device, dtype=torch.float32)
        kp3d = torch.empty(n, 24, 3, device=self.device, dtype=torch.float32) if joints24 else None
        sp = batch["smpl_params"]
        for g in (0, 1):
            rows = np.nonzero((genders == 1) if g == 1 else (genders != 1))[0]
            if len(rows) == 0:
                continue
            r = batch["_rows_f" if g == 1 else "_rows_m"]
            model = self._smpl_for(g, len(rows))
            v = model(sp["global_orient"].index_select(0, r), sp["body_pose"].index_select(0, r), sp["betas"].index_select(0, r)).vertices
            verts.index_copy_(0, r, v)
            if joints24:
                from .evaluator import regress_joints_gpu
                kp3d.index_copy_(0, r, regress_joints_gpu(self._J[g], v))
        return verts, kp3d

    def batch(self, idxs, frames=None):
        """One collated batch of the given items, on the device, enqueued on the current stream.  `frames`: what `read_item` gives
        for them, where the caller has it already (the iterator's decode threads); read here otherwise."""
        idxs = [int(i) for i in idxs]
        if frames is None:
            frames = [self.read_item(i) for i in idxs]
        a, trans, strings = self.host_batch(idxs, [f.shape[:2] if isinstance(f, np.ndarray) else f.size for f in frames])
        pack = _Pack()
        for k, v in a.items():
            if isinstance(v, dict):
                for kk, vv in v.items():
                    pack.add((k, kk), vv)
            else:
                pack.add(k, v)
        genders = self.gender[idxs] if self._has_meshes else None
        if genders is not None:
            pack.add("_rows_m", np.nonzero(genders != 1)[0].astype(np.int64))
            pack.add("_rows_f", np.nonzero(genders == 1)[0].astype(np.int64))
        if self.decode != "host":
            img, extra = self._crops_from_items(idxs, frames, trans, pack.bytes())
        else:
            img, extra = self.cropper.warp_frames(frames, trans, None, truncate=3.0, patch=self.img_size, mean=self.mean_rgb, std=self.std_rgb,
                                                  is_bgr=True, windows=self.windows, extra=pack.bytes())
        batch = {"img": img}
        for k, v in pack.views(extra).items():
            if isinstance(k, tuple):
                batch.setdefault(k[0], {})[k[1]] = v
            else:
                batch[k] = v
        if genders is not None:
            verts, kp3d = self._meshes(batch, genders, self.kind == "EMDBDataset")
            batch["vertices"] = verts
            if kp3d is not None:
                batch["keypoints_3d"] = kp3d
        batch.pop("_rows_m", None)
        batch.pop("_rows_f", None)
        batch.update(strings)
        return batch

    def __getitem__(self, idx):
        """One item with the reference's keys: arrays as device tensors, names and Python scalars as the reference has them."""
        b = self.batch([idx])
        item = {}
        for k, v in b.items():
            if isinstance(v, dict):
                item[k] = {kk: (bool(vv[0]) if vv.dtype == torch.bool else vv[0]) for kk, vv in v.items()}
            elif torch.is_tensor(v):
                item[k] = int(v[0]) if k in ("personid", "idx") else v[0]
            else:
                item[k] = v[0]
        return item

    def batches(self, batch_size, num_workers=4, prefetch=2, shuffle=False, start=0, stop=None):
        """Iterator of collated batches over items [start, stop) in index order (the last batch may be short): the DataLoader of
        eval.py:124 and its recursive_to.  `num_workers` threads (at most 16) decode the frames of the NEXT batches while the current
        one runs; one more thread packs and enqueues each batch on a side stream the iterator owns, `prefetch` batches ahead, and the
        consumer's stream waits on that batch's event.  Each batch has fresh tensors (only the cropper's staging is recycled), so a
        consumer may hold batch k while batch k+1 is produced.  No process is started.  One iterator at a time per dataset, and no
        `batch()` / `ds[i]` from another thread meanwhile: they share the dataset's cropper."""
        if shuffle:
            raise NotImplementedError("shuffle=True: the device datasets iterate in index order (eval.py's default)")
        stop = len(self) if stop is None else int(stop)
        batch_size, start = int(batch_size), int(start)
        if batch_size < 1 or not (0 <= start <= stop <= len(self)):
            raise ValueError("batches needs batch_size >= 1 and 0 <= start <= stop <= len(dataset)")
        return _BatchIterator(self, [list(range(s, min(s + batch_size, stop))) for s in range(start, stop, batch_size)],
                              max(1, min(int(num_workers), MAX_WORKERS)), max(1, int(prefetch)))


def _put(q, stop, item):
    while not stop.is_set():
        try:
            q.put(item, timeout=0.05)
            return True
        except queue.Full:
            continue
    return False


def _produce(ds, groups, prefetch, pool, q, stop, side):
    """The producer thread's body.  It holds the dataset and the queue, NOT the iterator, so an abandoned iterator is collected and
    its __del__ stops this thread."""
    try:
        ahead = prefetch + 1                      # batches whose frames are being decoded
        futs = {}
        for k in range(len(groups)):
            for j in range(k, min(k + ahead, len(groups))):
                if j not in futs:
                    futs[j] = [pool.submit(ds.read_item, i) for i in groups[j]]
            if stop.is_set():
                return
            frames = [f.result() for f in futs.pop(k)]
            if side is not None:
                with torch.cuda.stream(side):
                    b = ds.batch(groups[k], frames)
                    ev = torch.cuda.Event()
                    ev.record(side)
            else:
                b, ev = ds.batch(groups[k], frames), None
            if not _put(q, stop, (b, ev, None)):
                return
        _put(q, stop, (None, None, None))
    except BaseException as e:                  # handed to the consumer, which re-raises it
        _put(q, stop, (None, None, e))


class _BatchIterator:
    def __init__(self, ds, groups, workers, prefetch):
        self.ds, self.groups = ds, groups
        self.pool = ThreadPoolExecutor(workers, thread_name_prefix="thmr-decode")
        self.q = queue.Queue(maxsize=prefetch)
        self.stop = threading.Event()
        self.side = None
        if ds.device.type == "cuda":
            _ = ds.cropper                      # resolves 'cuda' to an indexed device before the stream is made
            self.side = torch.cuda.Stream(ds.device)
        self.done = False
        self.thread = threading.Thread(target=_produce, args=(ds, groups, prefetch, self.pool, self.q, self.stop, self.side),
                                       name="thmr-batches", daemon=True)
        self.thread.start()

    def __len__(self):
        return len(self.groups)

    def __iter__(self):
        return self

    def __next__(self):
        if self.done:
            raise StopIteration
        b, ev, err = self.q.get()
        if err is not None or b is None:
            self.close()
            if err is not None:
                raise err
            raise StopIteration
        if ev is not None:
            cur = torch.cuda.current_stream(self.ds.device)
            cur.wait_event(ev)
            for t in _tensors(b):
                t.record_stream(cur)            # allocated on the side stream, read on the consumer's
        return b

    def close(self):
        """Stops the producer and the decode threads and waits for them; called at exhaustion, on error, by run_eval when its loop
        ends for any reason, and when an abandoned iterator is collected."""
        if self.done:
            return
        self.done = True
        self.stop.set()
        while self.thread.is_alive():
            try:
                self.q.get_nowait()
            except queue.Empty:
                pass
            self.thread.join(0.05)
        self.pool.shutdown(wait=True, cancel_futures=True)
        if self.side is not None:
            self.side.synchronize()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _tensors(x):
    if torch.is_tensor(x):
        yield x
    elif isinstance(x, dict):
        for v in x.values():
            yield from _tensors(v)


class ImageDataset(_EvalDataset):
    """tokenhmr/lib/datasets/image_dataset.py:54-271 with train=False."""

    kind = "ImageDataset"

    def __init__(self, cfg, dataset_file, img_dir, train=False, prune=None, dataset_name="", device="cuda:0", imread=None, cropper=None,
                 smpl_male=None, smpl_female=None, windows=True, decode="host", **kwargs):
        self._init_common(cfg, dataset_file, img_dir, train, device, imread, cropper, smpl_male, smpl_female, decode)
        self.dataset_name, self.windows = dataset_name, windows
        n = len(self.imgname)
        num_pose = 3 * (int(cfg.SMPL.NUM_BODY_JOINTS) + 1)
        self._load_box(divide=True)
        try:
            self.body_pose = self.data["body_pose"].astype(np.float32)
            self.has_body_pose = self.data["has_body_pose"].astype(np.float32)
        except KeyError:
            self.body_pose = np.zeros((n, num_pose), dtype=np.float32)
            self.has_body_pose = np.zeros(n, dtype=np.float32)
        try:
            self.betas = self.data["betas"].astype(np.float32)
            self.has_betas = self.data["has_betas"].astype(np.float32)
        except KeyError:
            self.betas = np.zeros((n, 10), dtype=np.float32)
            self.has_betas = np.zeros(n, dtype=np.float32)
        try:
            body2d = self.data["body_keypoints_2d"]
        except KeyError:
            body2d = np.zeros((len(self.center), 25, 3))
        try:
            extra2d = self.data["extra_keypoints_2d"]
        except KeyError:
            extra2d = np.zeros((len(self.center), 19, 3))
        self.keypoints_2d = np.concatenate((body2d, extra2d), axis=1).astype(np.float32)
        self._load_keypoints_3d()
        self.has_gender = self._load_gender()
        self._has_meshes = self.has_gender

    def _host_extra(self, idxs, a, strings):
        a["keypoints_3d"] = self.keypoints_3d[idxs].astype(np.float32)        # keypoint_3d_processing with rot = 0: the identity
        strings["dataset"] = [self.dataset_name] * len(idxs)


class EMDBDataset(_EvalDataset):
    """tokenhmr/lib/datasets/emdb_dataset.py:23-200 with train=False."""

    kind = "EMDBDataset"

    def __init__(self, cfg, dataset_file, img_dir, train=False, prune=None, device="cuda:0", imread=None, cropper=None, smpl_male=None,
                 smpl_female=None, windows=True, decode="host", **kwargs):
        self._init_common(cfg, dataset_file, img_dir, train, device, imread, cropper, smpl_male, smpl_female, decode)
        self.windows = windows
        try:
            self.extra_info = self.data["extra_info"]
        except KeyError:
            self.extra_info = [{} for _ in range(len(self.imgname))]
        self._load_box(divide=False)
        self.body_pose = self.data["body_pose"].astype(np.float32)
        self.has_body_pose = self.data["has_body_pose"].astype(np.float32)
        self.betas = self.data["betas"].astype(np.float32)
        self.has_betas = self.data["has_betas"].astype(np.float32)
        self.keypoints_2d = self.data["keypoints_2d"]          # keeps the file's dtype until the final astype(float32)
        self._load_keypoints_3d()                              # as the reference: loaded, then replaced by J_regressor @ vertices
        self._load_gender()
        self._has_meshes = True

    def _host_extra(self, idxs, a, strings):
        import copy
        a["gender"] = self.gender[idxs].astype(np.int32)
        strings["extra_info"] = [copy.deepcopy(self.extra_info[i]) for i in idxs]


_TYPES = {"ImageDataset": ImageDataset, "EMDBDataset": EMDBDataset}


def create_dataset(cfg, dataset_cfg, train=False, device="cuda:0", imread=None, decode="host", **kwargs):
    """lib/datasets/__init__.py:17-26 for the two evaluation types: dispatches on dataset_cfg.TYPE and passes the node's other keys,
    lower-cased, to the constructor (dataset_file, img_dir; keypoint_list, use_hips ride along unused, as in the reference).
    decode="host" (the default): `imread` decodes every frame on the host.  decode="device": baseline JPEG files are only
    entropy-decoded on the host, for the window their crop reads, and finished on the device (tokenhmr_amd.jpeg); other files fall back
    to `imread` one by one; `dataset.decode_stats` counts both and the coefficient bytes uploaded.  decode="device+png": as "device",
    and PNG files are inflated on the host for their window and un-filtered and converted on the device (tokenhmr_amd.png);
    `dataset.png_stats` counts the PNG items finished on the device, those that fell back and the filtered bytes uploaded."""
    if decode not in DECODE_MODES:
        raise ValueError(f"decode={decode!r}: the decoders are {DECODE_MODES}")
    if train:
        raise NotImplementedError("train=True: the device datasets are evaluation-only (augmentation stays with the reference)")
    t = dataset_cfg["TYPE"] if "TYPE" in dataset_cfg else None
    if t not in _TYPES:
        raise NotImplementedError(f"TYPE={t!r}: the device datasets are {sorted(_TYPES)}; other types stay with the reference")
    kw = {k.lower(): v for k, v in dataset_cfg.items()}
    kw.pop("type")
    kw.update(kwargs)
    return _TYPES[t](cfg, train=train, device=device, imread=imread, decode=decode, **kw)
