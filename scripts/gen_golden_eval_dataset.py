"""TEST INFRASTRUCTURE ONLY — golden items of the reference's OWN evaluation datasets: tokenhmr/lib/datasets/dataset.py, utils.py,
image_dataset.py and emdb_dataset.py EXECUTED IN PLACE (nothing of their text is copied), following oracle/gen_golden_crop.py's
load_reference_datasets.  Only what the image lacks is stubbed:
  cv2.getAffineTransform / warpAffine -> oracle/crop_oracle.py restatements (UNPINNED, see its header)
  cv2.imread                          -> a dict of in-memory frames
  cv2.Rodrigues                       -> a scipy Rotation round trip in the input's dtype (UNPINNED: cv2's own rounding and its
                                         representative for angles >= pi are not reproduced; the drop-in states this departure and the
                                         tests compare global_orient as a rotation)
  smplx.SMPL(gender=...)              -> the oracle's fp32 SMPL (oracle/tokenhmr_oracle.py) on make_synthetic_smpl constants, one seed per
                                         gender, with that model's .J_regressor
  yacs / webdataset / braceexpand / skimage -> empty or minimal modules
  numpy 1.23's promotion (requirements.txt:1) of `float32 array - float64 scalar` -> the datasets are handed float32 mean / std after
                                         construction, which is that arithmetic (oracle/crop_oracle.py finish_patch, numpy1=True); the
                                         generator checks the float64 expression of this image's numpy is within 1 float32 ulp of it

Inputs are synthetic: three frames (64x48, 181x260, 200x150 — width x height) and three dataset files, stored in the fixture as arrays
  image   6 items, scale of shape (n,), both genders, one item without has_body_pose
  emdb    4 items, scale of shape (n,2) with unequal sides (not divided by 200), float64 keypoints_2d
  bare    2 items with nothing but imgname / center / scale: the KeyError fallbacks
with boxes inside the frame, over the top-left corner, over the bottom-right corner, entirely outside and an 8x up-sampling one; two
items share one frame; global orientations have angle < pi; some keypoints fall outside the patch.

    python scripts/gen_golden_eval_dataset.py [--reference DIR]   ->   tests/golden/eval_dataset.npz
Stored per item: every key of the reference's item (`img` on the ::4 sub-grid, `vertices` at every 10th vertex), a JSON record of each
value's Python type and dtype and of the dtype default_collate gives it, and d_ref, the max distance of the stand-in's fp32 vertices
from oracle/lbs_independent.py in fp64 on the same inputs."""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden_crop as GC  # noqa: E402
from oracle import crop_oracle as CO  # noqa: E402
from oracle import tokenhmr_oracle as O  # noqa: E402
from oracle.lbs_independent import smpl_forward_independent  # noqa: E402
from tokenhmr_amd.config import HMRConfig  # noqa: E402
from tokenhmr_amd.smpl_assets import make_synthetic_smpl  # noqa: E402

SMPL_SEED = {"male": 1, "female": 2}
FRAME_SIZES = {"f0.jpg": (48, 64), "f1.jpg": (260, 181), "f2.jpg": (150, 200)}        # (H, W)
OUT = os.path.join(ROOT, "tests", "golden", "eval_dataset.npz")


def frames():
    return {name: GC.synthetic_frame(H, W, seed=10 + k) for k, (name, (H, W)) in enumerate(sorted(FRAME_SIZES.items()))}


def smpl_constants(gender):
    return make_synthetic_smpl(HMRConfig(), SMPL_SEED[gender])


def rodrigues(x):
    """cv2.Rodrigues: (3,) / (3,1) / (1,3) rotation vector -> (3,3) matrix, (3,3) matrix -> (3,1) vector; (result, jacobian)."""
    from scipy.spatial.transform import Rotation
    x = np.asarray(x)
    if x.shape == (3, 3):
        return Rotation.from_matrix(x.astype(np.float64)).as_rotvec().reshape(3, 1).astype(x.dtype), None
    return Rotation.from_rotvec(x.astype(np.float64).reshape(3)).as_matrix().astype(x.dtype), None


def load_reference(ref_dir, frame_dict):
    GC.REF = ref_dir
    mods = GC.load_reference_datasets()               # cv2 (affine + warp), skimage, yacs, webdataset, braceexpand; utils.py executed
    cv2 = sys.modules["cv2"]
    cv2.IMREAD_COLOR, cv2.IMREAD_IGNORE_ORIENTATION, cv2.BORDER_REPLICATE = 1, 128, 1
    cv2.imread = lambda path, flags=None: frame_dict.get(os.path.basename(path))
    cv2.Rodrigues = rodrigues
    smplx = types.ModuleType("smplx")

    class SMPL:
        def __init__(self, gender="neutral", **kw):
            self.const = smpl_constants(gender)
            self.J_regressor = self.const["J_regressor"]

        def __call__(self, global_orient, body_pose, betas):
            with torch.no_grad():
                v, _ = O.smpl_forward_axis_angle(global_orient, body_pose, betas, self.const)
            return types.SimpleNamespace(vertices=v)

    smplx.SMPL = SMPL
    sys.modules["smplx"] = smplx
    for name in ("dataset", "smplh_prob_filter", "image_dataset", "emdb_dataset"):
        spec = importlib.util.spec_from_file_location(f"_ref_ds.{name}", os.path.join(ref_dir, f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        mod.__package__ = "_ref_ds"
        sys.modules[f"_ref_ds.{name}"] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


def model_cfg():
    C = GC._Cfg
    return C(MODEL=C(IMAGE_SIZE=256, IMAGE_MEAN=[0.485, 0.456, 0.406], IMAGE_STD=[0.229, 0.224, 0.225], BBOX_SHAPE=[192, 256]),
             SMPL=C(MODEL_PATH="smpl", NUM_BODY_JOINTS=23), DATASETS=C(CONFIG=C()))


def _poses(rng, n):
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    go = axis * rng.uniform(0.2, 2.5, size=(n, 1))              # angle < pi: one representative, no wrap in the Rodrigues round trip
    return np.concatenate([go, 0.3 * rng.normal(size=(n, 69))], axis=1)


def _kp2d(rng, names, k):
    out = np.zeros((len(names), k, 3))
    for i, nm in enumerate(names):
        H, W = FRAME_SIZES[nm]
        out[i, :, 0] = rng.uniform(-0.5 * W, 1.5 * W, size=k)     # some outside the frame, hence outside the patch
        out[i, :, 1] = rng.uniform(-0.5 * H, 1.5 * H, size=k)
        out[i, :, 2] = rng.uniform(0, 1, size=k)
    return out


def make_inputs():
    rng = np.random.default_rng(20240)
    names = ["f2.jpg", "f2.jpg", "f1.jpg", "f0.jpg", "f1.jpg", "f0.jpg"]
    n = len(names)
    image = {"imgname": np.array(names),
             # inside | over the top-left corner (same frame) | over the bottom-right corner | entirely outside | 8x up-sampling | inside
             "center": np.array([[100.3, 75.2], [10.0, 8.5], [170.25, 250.0], [-200.0, -150.0], [90.0, 130.5], [30.0, 20.0]]),
             "scale": np.array([90.0, 60.5, 70.0, 40.0, 24.0, 30.0]),
             "body_pose": _poses(rng, n), "has_body_pose": np.array([1.0, 1, 0, 1, 1, 1]),
             "betas": 0.5 * rng.normal(size=(n, 10)), "has_betas": np.array([1.0, 1, 1, 0, 1, 1]),
             "body_keypoints_2d": _kp2d(rng, names, 25), "extra_keypoints_2d": _kp2d(rng, names, 19),
             "body_keypoints_3d": rng.normal(size=(n, 25, 4)), "extra_keypoints_3d": rng.normal(size=(n, 19, 4)),
             "gender": np.array(["m", "f", "male", "female", "f", "m"])}
    names = ["f1.jpg", "f2.jpg", "f2.jpg", "f0.jpg"]
    n = len(names)
    emdb = {"imgname": np.array(names),
            # inside | over the top-left corner | over the bottom-right corner (same frame) | 8x up-sampling
            "center": np.array([[90.5, 130.0], [12.0, 9.0], [190.0, 141.5], [32.0, 24.0]]),
            "scale": np.array([[0.4, 0.6], [0.5, 0.3], [0.45, 0.35], [0.1, 0.16]]),
            "body_pose": _poses(rng, n), "has_body_pose": np.ones(n), "betas": 0.5 * rng.normal(size=(n, 10)), "has_betas": np.ones(n),
            "keypoints_2d": _kp2d(rng, names, 44), "gender": np.array(["female", "male", "f", "m"])}
    bare = {"imgname": np.array(["f0.jpg", "f1.jpg"]), "center": np.array([[30.0, 22.0], [100.0, 100.0]]), "scale": np.array([[35.0], [150.0]])}
    return {"image": image, "emdb": emdb, "bare": bare}


def describe(v):
    if torch.is_tensor(v):
        return "Tensor:" + str(v.dtype).replace("torch.", "")
    if isinstance(v, np.ndarray):
        return "ndarray:" + str(v.dtype)
    if isinstance(v, np.generic):
        return "scalar:" + str(v.dtype)
    return type(v).__name__


def flatten(item):
    flat = {}
    for k, v in item.items():
        if isinstance(v, dict) and k != "extra_info":
            for kk, vv in v.items():
                flat[f"{k}.{kk}"] = vv
        else:
            flat[k] = v
    return flat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=GC.REF, help="the reference's tokenhmr/lib/datasets directory")
    args = ap.parse_args()
    from torch.utils.data import default_collate
    fr = frames()
    mods = load_reference(args.reference, fr)
    cfg = model_cfg()
    inputs = make_inputs()
    out = {f"frame/{k}": v for k, v in fr.items()}
    meta = {"kinds": {}, "smpl_seed": SMPL_SEED, "bbox_shape": [192, 256], "img_dir": "imgs"}
    d_ref = 0.0
    tmp = tempfile.mkdtemp()
    for kind, arrays in inputs.items():
        for k, v in arrays.items():
            out[f"in_{kind}/{k}"] = v
        path = os.path.join(tmp, f"{kind}.npz")
        np.savez(path, **arrays)
        if kind == "emdb":
            ds = mods["emdb_dataset"].EMDBDataset(cfg, path, "imgs", train=False)
        else:
            ds = mods["image_dataset"].ImageDataset(cfg, path, "imgs", train=False)
        # numpy 1.23 promotion of the normalisation (see the header): float32 mean / std
        items64 = [ds[i] for i in range(len(ds))]
        ds.mean, ds.std = ds.mean.astype(np.float32), ds.std.astype(np.float32)
        items = [ds[i] for i in range(len(ds))]
        for a, b in zip(items, items64):
            assert a["img"].dtype == np.float32 and np.abs(a["img"] - b["img"]).max() < 5e-7
            fa, fb = flatten(a), flatten(b)
            assert all(np.array_equal(np.asarray(fa[k]), np.asarray(fb[k])) for k in fa if k not in ("img", "extra_info"))
        # the restated crop is the reference's, bit for bit, on the full grid
        for i, it in enumerate(items):
            mine = CO.example_item(fr[arrays["imgname"][i]], it["box_center"][0], it["box_center"][1], it["box_size"], it["box_size"])
            assert np.array_equal(mine["img"], it["img"]), (kind, i)
        coll = default_collate([{k: v for k, v in it.items() if k != "extra_info"} for it in items])
        types_, collated = {}, {k: describe(v) for k, v in flatten(coll).items()}
        for i, it in enumerate(items):
            for k, v in flatten(it).items():
                types_[k] = describe(v)
                if k == "extra_info":
                    assert v == {}
                    continue
                v = v.numpy() if torch.is_tensor(v) else np.asarray(v)
                if k == "img":
                    v = v[:, ::4, ::4]
                if k == "vertices":
                    v = v[::10]
                out[f"{kind}/{i}/{k}"] = v
            if "vertices" in it:
                sp = it["smpl_params"]
                aa = np.concatenate([sp["global_orient"], sp["body_pose"]]).astype(np.float64).reshape(24, 3)
                from scipy.spatial.transform import Rotation
                R = Rotation.from_rotvec(aa).as_matrix()[None]
                gender = "female" if ds.gender[i] == 1 else "male"
                v64, _ = smpl_forward_independent(R, sp["betas"][None].astype(np.float64), smpl_constants(gender))
                d_ref = max(d_ref, float(np.linalg.norm(it["vertices"].numpy().astype(np.float64) - v64[0], axis=1).max()))
        meta["kinds"][kind] = {"n": len(items), "types": types_, "collated": collated}
        print(kind, len(items), "items;", sorted(types_))
    out["d_ref"] = np.array(d_ref)
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("d_ref", d_ref, "wrote", OUT, size, "bytes")
    assert size < 1_000_000, size


if __name__ == "__main__":
    main()
