"""Shared by tests/test_eval_dataset_host.py and tests/test_gpu_eval_dataset.py: tests/golden/eval_dataset.npz
(scripts/gen_golden_eval_dataset.py: the reference's ImageDataset / EMDBDataset executed in place on synthetic inputs) read back,
its input files re-written, and the comparison of a drop-in batch with the reference's items."""
import json
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_dataset.npz")
_cache = {}


def gold():
    if "g" not in _cache:
        z = np.load(GOLD)
        _cache["g"] = {k: z[k] for k in z.files}
        _cache["meta"] = json.loads(str(_cache["g"]["meta"]))
    return _cache["g"], _cache["meta"]


def frames():
    g, _ = gold()
    return {k.split("/", 1)[1]: g[k] for k in g if k.startswith("frame/")}


def imread(path):
    return frames().get(os.path.basename(path))


def model_cfg():
    from tokenhmr_amd.model import ConfigNode
    _, meta = gold()
    return ConfigNode({"MODEL": {"IMAGE_SIZE": 256, "IMAGE_MEAN": [0.485, 0.456, 0.406], "IMAGE_STD": [0.229, 0.224, 0.225],
                                 "BBOX_SHAPE": meta["bbox_shape"]},
                       "SMPL": {"MODEL_PATH": "smpl", "NUM_BODY_JOINTS": 23}, "DATASETS": {"CONFIG": {}}})


def write_input(kind, tmp_path):
    g, _ = gold()
    path = os.path.join(str(tmp_path), f"{kind}.npz")
    np.savez(path, **{k.split("/", 1)[1]: g[k] for k in g if k.startswith(f"in_{kind}/")})
    return path


def smpl_constants():
    """The constants of the generator's stand-in smplx.SMPL, per gender."""
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    _, meta = gold()
    if "smpl" not in _cache:
        _cache["smpl"] = {k: make_synthetic_smpl(HMRConfig(), s) for k, s in meta["smpl_seed"].items()}
    return _cache["smpl"]


def make_dataset(kind, tmp_path, device, **kw):
    from tokenhmr_amd.datasets import create_dataset
    _, meta = gold()
    sm = smpl_constants()
    dcfg = {"TYPE": "EMDBDataset" if kind == "emdb" else "ImageDataset", "DATASET_FILE": write_input(kind, tmp_path),
            "IMG_DIR": meta["img_dir"], "KEYPOINT_LIST": [0]}
    return create_dataset(model_cfg(), dcfg, train=False, device=device, imread=imread, smpl_male=sm["male"], smpl_female=sm["female"], **kw)


def ref_item(kind, i):
    """Reference item i as {flattened key: numpy value} ('smpl_params.betas', ...)."""
    g, _ = gold()
    p = f"{kind}/{i}/"
    return {k[len(p):]: g[k] for k in g if k.startswith(p)}


def flat(batch):
    out = {}
    for k, v in batch.items():
        if isinstance(v, dict) and k != "extra_info":
            for kk, vv in v.items():
                out[f"{k}.{kk}"] = vv
        else:
            out[k] = v
    return out


def rotmat(aa):
    """Rodrigues in float64."""
    aa = np.asarray(aa, dtype=np.float64)
    t = np.linalg.norm(aa)
    if t == 0:
        return np.eye(3)
    k = aa / t
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


DEVICE_KEYS = ("img", "vertices")          # compared by the GPU tests; EMDB's keypoints_3d as well


def check_host_keys(kind, idxs, batch, skip=()):
    """Every non-image key of a collated drop-in batch against the reference's items `idxs`: values, dtype and collated dtype.
    Returns the number of keypoints_2d entries that are not bit-equal (allowed: 2 spacings of float32(|ref| + 0.5), the reference's
    np.dot summation order being BLAS's)."""
    _, meta = gold()
    m = meta["kinds"][kind]
    fb = flat(batch)
    skip = set(skip) | set(DEVICE_KEYS) | ({"keypoints_3d"} if kind == "emdb" else set())
    assert set(fb) == set(m["types"]), (sorted(set(fb) ^ set(m["types"])))
    inexact = 0
    for key, typ in m["types"].items():
        if key in skip:
            continue
        mine = fb[key]
        refs = [ref_item(kind, i).get(key) for i in idxs]
        if key == "extra_info":
            assert mine == [{} for _ in idxs]                 # the list of per-item dicts, not collated (stated departure)
            continue
        if typ == "str" or typ.startswith("scalar:<U"):          # imgname_rel is a numpy str_ in the reference; collated to a list of str
            assert isinstance(mine, list) and mine == [str(r) for r in refs], key
            continue
        assert torch.is_tensor(mine), key
        want = m["collated"][key].split(":")[1]
        assert str(mine.dtype).replace("torch.", "") == want, (key, mine.dtype, want)
        a, ref = mine.cpu().numpy(), np.stack(refs)
        assert a.shape == ref.shape, (key, a.shape, ref.shape)
        if key == "smpl_params.global_orient":
            # departure: passed through unchanged; the reference's rot_aa(aa, 0) is a Rodrigues round trip — the same rotation
            d = max(np.abs(rotmat(x) - rotmat(y)).max() for x, y in zip(a, ref))
            assert d <= 1e-6, d
        elif key == "keypoints_2d":
            assert np.array_equal(a[..., 2], ref[..., 2])
            tol = 2 * np.spacing(np.float32(np.abs(ref[..., :2]) + np.float32(0.5)))
            assert (np.abs(a[..., :2].astype(np.float64) - ref[..., :2]) <= tol).all(), np.abs(a[..., :2] - ref[..., :2]).max()
            inexact += int((a != ref).sum())
        else:
            assert np.array_equal(a, ref.astype(a.dtype)) and (ref.dtype == a.dtype or typ in ("int", "bool")), (key, a.dtype, ref.dtype)
    return inexact
