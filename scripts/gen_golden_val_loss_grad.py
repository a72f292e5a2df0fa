"""Writes tests/golden/val_loss_grad.npz: the gradient of the reference's own TokenHMR.compute_loss (tokenhmr/lib/models/tokenhmr.py:190-277)
executed IN PLACE in float64 under torch autograd on seeded inputs (B = 5), in both branches (plain, and LOOSE_SUP with train=True) and with
the ground-truth pose as axis-angle and as matrices.

Nothing of the reference is copied: tokenhmr.py, losses.py and geometry.py are loaded by path (scripts/gen_golden_val_loss.py::load_reference).
Two runs per case:
  direct   the five tensors compute_loss reads are leaves: d loss / d (pred_keypoints_2d, pred_keypoints_3d, global_orient, body_pose, betas)
  chain    the joints and pred_cam are leaves; pred_cam_t is formed as forward_step forms it (:166-168) and pred_keypoints_2d by the
           reference's own perspective_projection with focal_length / IMAGE_SIZE (:183-185): d loss / d (joints, pred_cam)
The reference writes into its batch in the loose branch (:223, :227, :240): every run gets clones.
One adapter: with matrix ground truth compute_loss flattens it to (B, 9 n) (:233, :258), which the loose branch's ParameterLossPCKT cannot
broadcast against (B, n, 3, 3) — the reference never trains on matrix ground truth there.  The parameter-loss module is therefore wrapped
so that the ground truth it receives has the prediction's shape; its arithmetic is the reference's.

    python scripts/gen_golden_val_loss_grad.py [--check]
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import gen_golden_val_loss as GV          # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "val_loss_grad.npz")
SEED, BATCH = 4100, 5
FOCAL_LENGTH, IMAGE_SIZE = 5000.0, 256.0          # tokenhmr_release.yaml: EXTRA.FOCAL_LENGTH, MODEL.IMAGE_SIZE
PLANT = 7                                         # the keypoint of item 0 with pred == gt bit for bit
VALID_3D = ("H36M-TRAIN-WMASK", "BEDLAM")
CASES = [("plain", "aa"), ("plain", "mat"), ("loose", "aa"), ("loose", "mat")]
SLOTS = ("kp2d", "kp3d", "joints", "cam", "rotmat", "betas")


def _away(r, shape, lo, scale):
    """Random numbers of either sign whose magnitude is at least `lo`."""
    return r.choice([-1.0, 1.0], shape) * (lo + np.abs(scale * r.standard_normal(shape)))


def make_inputs(B, seed, pelvis_id=39, thresholds=None):
    """gen_golden_val_loss.make_inputs plus what the gradient's tests need (tests/val_loss_grad_oracle.input_conditions states it):
    'pred_cam' with X_z far above 1; pred_keypoints_2d = the projection of pred_keypoints_3d, rounded to float32; every 2D difference and
    every pelvis-relative 3D residual at least 2e-3 in size; keypoint PLANT of item 0 with pred == gt bit for bit (and item 0's ground-truth
    pelvis equal to the predicted one, so that the residual is an exact 0); item 0 from a trusted 3D dataset, item 1 not;
    'gt_pose_rotmat', the float32 matrices of the ground-truth pose.  thresholds (the LOOSE_SUP tables): 2D differences are then scaled
    so that kp2d_err lands on both sides of its threshold."""
    import val_loss_oracle as VO
    inp = GV.make_inputs(B, seed)
    r = np.random.default_rng(seed + 1)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
    cam = f32(np.stack([r.uniform(0.7, 1.1, B), r.uniform(-0.2, 0.2, B), r.uniform(-0.2, 0.2, B)], 1))
    J = inp["pred_keypoints_3d"].astype(np.float64)
    t = np.stack([cam[:, 1], cam[:, 2], 2.0 * FOCAL_LENGTH / (IMAGE_SIZE * cam[:, 0].astype(np.float64) + 1e-9)], 1)
    X = J + t[:, None]
    kp2 = f32((FOCAL_LENGTH / IMAGE_SIZE) * X[:, :, :2] / X[:, :, 2:])
    # 2D: per keypoint a difference below or above its threshold (kp2d_err = conf (dx^2 + dy^2))
    thr = np.full(44, 0.008) if thresholds is None else np.asarray(thresholds["kp2d"], dtype=np.float64)
    size = np.sqrt(thr)[None, :, None] * np.where(r.uniform(size=(B, 44, 1)) < 0.5, r.uniform(0.15, 0.6, (B, 44, 1)), r.uniform(1.5, 2.5, (B, 44, 1)))
    d2 = r.choice([-1.0, 1.0], (B, 44, 2)) * np.maximum(size * r.uniform(0.5, 1.0, (B, 44, 2)), 2e-3)
    g2 = kp2.astype(np.float64) - d2
    # 3D: g = p - n, the residual is n_k - n_pelvis
    n = _away(r, (B, 44, 3), 2e-3, 0.05)
    n_pel = 0.02 * r.standard_normal((B, 1, 3))
    n_pel[0] = 0.0
    n = n + n_pel
    n[:, pelvis_id] = n_pel[:, 0]
    g3 = J - n
    g2[0, PLANT], g3[0, PLANT] = kp2[0, PLANT], J[0, PLANT]
    inp["pred_keypoints_2d"] = kp2
    inp["gt_keypoints_2d"][:, :, :2] = f32(g2)
    inp["gt_keypoints_3d"][:, :, :3] = f32(g3)
    inp["gt_keypoints_2d"][0, PLANT, 2] = inp["gt_keypoints_3d"][0, PLANT, 3] = 1.0
    inp["pred_cam"] = cam
    inp["dataset"][0] = "BEDLAM"
    if B > 1:
        inp["dataset"][1] = "COCO-TRAIN-2014-PRUNED"
    inp["gt_pose_rotmat"] = f32(VO.aa_to_rotmat64(inp["gt_pose_aa"].reshape(-1, 3)).reshape(B, 24, 3, 3))
    return inp


def valid_3d(inp):
    return np.array([n in VALID_3D for n in inp["dataset"]], dtype=np.float32)


class _LikePrediction(torch.nn.Module):
    """The reference's parameter loss, handed a ground truth of the prediction's shape (see the module's docstring)."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, pred, gt, *rest):
        return self.inner(pred, gt.reshape(pred.shape), *rest)


def run_reference(inp, loose, gt):
    """-> {slot: float64 array}: the gradients of compute_loss's total by the reference's autograd."""
    from tokenhmr_amd.model import ConfigNode
    mod, L = GV.load_reference()
    geometry = sys.modules["_ref_hmr.utils.geometry"]
    cfg = ConfigNode({"MODEL": {"LOOSE_SUP": bool(loose), "LOOSE_WEIGHT": GV.LOOSE_WEIGHT}, "LOSS_WEIGHTS": dict(GV.LOSS_WEIGHTS)})
    ns = types.SimpleNamespace(cfg=cfg)
    if loose:          # tokenhmr.py:67-74
        ns.keypoint_3d_loss, ns.keypoint_2d_loss = L.Keypoint3DLossPCKT(loss_type="l1"), L.Keypoint2DLossPCKT(loss_type="l1")
        ns.smpl_parameter_loss = _LikePrediction(L.ParameterLossPCKT())
    else:
        ns.keypoint_3d_loss, ns.keypoint_2d_loss = L.Keypoint3DLoss(loss_type="l1"), L.Keypoint2DLoss(loss_type="l1")
        ns.smpl_parameter_loss = L.ParameterLoss()
    B = inp["gt_betas"].shape[0]

    def dicts():
        batch, output = GV.to_batch(inp, torch.float64, is_axis_angle=gt == "aa")          # clones
        if gt == "mat":
            Rg = torch.from_numpy(inp["gt_pose_rotmat"]).double()
            batch["smpl_params"]["global_orient"], batch["smpl_params"]["body_pose"] = Rg[:, :1].clone(), Rg[:, 1:].clone()
        return batch, output

    res = {}
    # direct: the five tensors compute_loss reads
    batch, output = dicts()
    leaves = [output["pred_keypoints_2d"], output["pred_keypoints_3d"], output["pred_smpl_params"]["global_orient"],
              output["pred_smpl_params"]["body_pose"], output["pred_smpl_params"]["betas"]]
    for t in leaves:
        t.requires_grad_(True)
    g = torch.autograd.grad(mod.TokenHMR.compute_loss(ns, batch, output, train=True), leaves)
    res["kp2d"], res["kp3d"], res["betas"] = g[0].numpy(), g[1].numpy(), g[4].numpy()
    res["rotmat"] = torch.cat([g[2], g[3]], 1).numpy()
    # chain: joints and pred_cam through forward_step's projection
    batch, output = dicts()
    J = output["pred_keypoints_3d"].requires_grad_(True)
    cam = torch.from_numpy(inp["pred_cam"]).double().requires_grad_(True)
    focal = FOCAL_LENGTH * torch.ones(B, 2, dtype=torch.float64)
    cam_t = torch.stack([cam[:, 1], cam[:, 2], 2 * focal[:, 0] / (IMAGE_SIZE * cam[:, 0] + 1e-9)], dim=-1)
    output["pred_keypoints_2d"] = geometry.perspective_projection(J, translation=cam_t, focal_length=focal / IMAGE_SIZE)
    # the planted keypoint keeps pred == gt in this graph: its ground truth is this float64 projection, not the float32 rounding of it
    batch["keypoints_2d"][0, PLANT, :2] = output["pred_keypoints_2d"].detach()[0, PLANT]
    gj, gc = torch.autograd.grad(mod.TokenHMR.compute_loss(ns, batch, output, train=True), [J, cam])
    res["joints"], res["cam"] = gj.numpy(), gc.numpy()
    return res


def compute(verbose=True):
    th = GV.thresholds()
    inp = make_inputs(BATCH, SEED, thresholds=th)
    out = {"in." + k: v for k, v in inp.items() if k != "dataset"}
    out["in.dataset"] = np.array(inp["dataset"])
    out["in.valid_3d"] = valid_3d(inp)
    out.update({"thresh." + k: v for k, v in th.items()})
    out["loss_weights"] = np.array([GV.LOSS_WEIGHTS[k] for k in ("KEYPOINTS_2D", "KEYPOINTS_3D", "GLOBAL_ORIENT", "BODY_POSE", "BETAS")], dtype=np.float64)
    out["loose_weight"] = np.array(GV.LOOSE_WEIGHT, dtype=np.float64)
    out["focal_length"], out["image_size"] = np.array(FOCAL_LENGTH), np.array(IMAGE_SIZE)
    for mode, gt in CASES:
        r = run_reference(inp, mode == "loose", gt)
        for k, v in r.items():
            out[f"{mode}.{gt}.{k}"] = v
        if verbose:
            print(mode, gt, " ".join(f"{k} {np.abs(v).max():.3e}" for k, v in r.items()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed fixture instead of writing it")
    args = ap.parse_args()
    new = compute()
    if args.check:
        old = np.load(OUT)
        assert set(old.files) == set(new), set(old.files) ^ set(new)
        for k, v in new.items():
            if v.dtype.kind in "US" or k.startswith(("in.", "thresh.")):
                assert np.array_equal(old[k], v), k
            else:
                assert np.allclose(old[k], v, rtol=1e-12, atol=1e-14), k
        print("val_loss_grad.npz: the reference reproduces the committed fixture")
        return
    np.savez_compressed(OUT, **new)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
