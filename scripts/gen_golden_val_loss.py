"""Writes tests/golden/val_loss.npz: the reference's own TokenHMR.compute_loss (tokenhmr/lib/models/tokenhmr.py:190-277) and TokenLoss
(losses.py:230-252) executed IN PLACE on seeded inputs, in both branches (plain, :250-262, and LOOSE_SUP, :214-249), in float32 and float64.

Nothing of the reference is copied.  tokenhmr.py is loaded by path under a made-up package, with empty stand-ins for what its import
lines need and this image may lack (pytorch_lightning, yacs, the two renderers of ..utils, pylogger, misc, backbones, heads,
discriminator, smpl_wrapper): compute_loss touches none of them.  geometry.py, rotation_utils.py and losses.py are the real files.
compute_loss is called unbound on a namespace that carries `cfg` and the three loss modules of TokenHMR.__init__ (:67-74).

What the fixture holds: the inputs (B = 8), the six losses of both modes and both precisions, the batch tensors the loose branch mutates
(:223, :227, :240) after the call, joint_angle_error and kp2D_err, the masks the loss modules were handed, the two threshold tables as
the loaded module holds them, and TokenLoss on a (3 * 160, 2048) softmax whose inputs are regenerated from a seed (`token_inputs`).

The seed is only accepted if every mask decision is far from its threshold: |angle - thresh| and |kp2D_err - thresh| in float64 exceed
4 x the largest float32-vs-float64 distance of that quantity on these inputs, and the reference's float32 masks equal its float64 masks.

    python scripts/gen_golden_val_loss.py [--check]
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "val_loss.npz")

SEED, BATCH = 2024, 8
TOKEN_SEED, TOKEN_ROWS = 77, 3 * 160
LOSS_WEIGHTS = {"KEYPOINTS_3D": 0.05, "KEYPOINTS_2D": 0.01, "GLOBAL_ORIENT": 0.001, "BODY_POSE": 0.001, "BETAS": 0.0005}     # tokenhmr_release.yaml:84-88
LOOSE_WEIGHT = 0.05                                                                                                         # :53
DATASETS = ("H36M-TRAIN-WMASK", "COCO-TRAIN-2014-PRUNED", "BEDLAM", "MPII-TRAIN", "AVA-TRAIN-MIDFRAMES-1FPS-WMASK")
LOSS_KEYS = ("loss", "loss_keypoints_2d", "loss_keypoints_3d", "loss_global_orient", "loss_body_pose", "loss_betas")


def _rodrigues64(aa):
    """(n,3) float64 axis-angle -> (n,3,3), the closed form (input construction only: the perturbed prediction)."""
    ang = np.linalg.norm(aa, axis=1, keepdims=True)
    ax = aa / np.maximum(ang, 1e-300)
    K = np.zeros((aa.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    s, c = np.sin(ang)[:, :, None], np.cos(ang)[:, :, None]
    return np.eye(3)[None] + s * K + (1 - c) * (K @ K)


def make_inputs(B, seed, pose_noise=0.25, kp2d_noise=0.07):
    """The batch and output tensors compute_loss reads, float32, as a flat dict of numpy arrays (+ 'dataset', a list of names).
    GT pose ~ N(0, 0.5) axis-angle; prediction = a rotation ~ N(0, pose_noise) applied on top of the GT pose; confidences Bernoulli(0.7);
    has_* Bernoulli(0.75) with item 0 forced to (1, 0, 1) and, from 2 items, item 1 to (0, 1, 0) so that every flag takes both values."""
    r = np.random.default_rng(seed)
    gt_aa = 0.5 * r.standard_normal((B, 24, 3))
    Rgt = _rodrigues64(gt_aa.reshape(-1, 3).astype(np.float32).astype(np.float64))
    Rp = _rodrigues64(pose_noise * r.standard_normal((B * 24, 3))) @ Rgt
    gt_betas = r.standard_normal((B, 10))
    kp2 = r.uniform(-0.5, 0.5, (B, 44, 2))
    kp3 = 0.3 * r.standard_normal((B, 44, 3))
    has = (r.uniform(size=(3, B)) < 0.75).astype(np.float32)
    has[:, 0] = (1, 0, 1)
    if B > 1:
        has[:, 1] = (0, 1, 0)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
    return {
        "pred_keypoints_2d": f(kp2 + kp2d_noise * r.standard_normal((B, 44, 2))),
        "pred_keypoints_3d": f(kp3 + 0.05 * r.standard_normal((B, 44, 3))),
        "pred_rotmat": f(Rp.reshape(B, 24, 3, 3)),
        "pred_betas": f(gt_betas + 0.3 * r.standard_normal((B, 10))),
        "gt_keypoints_2d": f(np.concatenate([kp2, (r.uniform(size=(B, 44, 1)) < 0.7)], 2)),
        "gt_keypoints_3d": f(np.concatenate([kp3, (r.uniform(size=(B, 44, 1)) < 0.7)], 2)),
        "gt_pose_aa": f(gt_aa.reshape(B, 72)),
        "gt_betas": f(gt_betas),
        "has_global_orient": has[0].copy(), "has_body_pose": has[1].copy(), "has_betas": has[2].copy(),
        "dataset": [DATASETS[i] for i in r.integers(0, len(DATASETS), B)],
    }


def token_inputs(seed=TOKEN_SEED, rows=TOKEN_ROWS):
    """(softmax probabilities (rows, 2048) float32, targets (rows) int64): what TokenLoss is handed (cls_logits_softmax, gt tokens)."""
    g = torch.Generator().manual_seed(int(seed))
    logits = 3.0 * torch.randn(rows, 2048, generator=g, dtype=torch.float32)
    return logits.softmax(-1), torch.randint(0, 2048, (rows,), generator=g)


def to_batch(inp, dtype=torch.float32, is_axis_angle=True):
    """The reference's (batch, output) dicts from make_inputs' arrays."""
    t = lambda k: torch.from_numpy(inp[k]).to(dtype).clone()      # noqa: E731  (a copy: the loose branch writes into the batch)
    B = inp["gt_betas"].shape[0]
    R = t("pred_rotmat")
    aa = t("gt_pose_aa")
    batch = {
        "keypoints_2d": t("gt_keypoints_2d"), "keypoints_3d": t("gt_keypoints_3d"),
        "smpl_params": {"global_orient": aa[:, :3].clone(), "body_pose": aa[:, 3:].clone(), "betas": t("gt_betas")},
        "has_smpl_params": {"global_orient": t("has_global_orient"), "body_pose": t("has_body_pose"), "betas": t("has_betas")},
        "smpl_params_is_axis_angle": {"global_orient": torch.full((B,), is_axis_angle), "body_pose": torch.full((B,), is_axis_angle),
                                      "betas": torch.zeros(B, dtype=torch.bool)},
        "dataset": list(inp["dataset"]),
    }
    output = {"pred_smpl_params": {"global_orient": R[:, :1].clone(), "body_pose": R[:, 1:].clone(), "betas": t("pred_betas")},
              "pred_keypoints_2d": t("pred_keypoints_2d"), "pred_keypoints_3d": t("pred_keypoints_3d")}
    return batch, output


def load_reference():
    """tokenhmr/lib/models/tokenhmr.py as a module of a made-up package -> (tokenhmr module, losses module)."""
    from oracle import ref_import
    if not ref_import.available():
        raise RuntimeError(f"reference tree not found at {ref_import.REF}")
    if "_ref_hmr.models.tokenhmr" in sys.modules:
        return sys.modules["_ref_hmr.models.tokenhmr"], sys.modules["_ref_hmr.models.losses"]
    lib = os.path.join(ref_import.REF, "tokenhmr", "lib")

    def standin(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    def absent(name):
        try:
            __import__(name)
            return False
        except Exception:
            return True

    ident = lambda f: f      # noqa: E731
    if absent("pytorch_lightning"):
        rz = standin("pytorch_lightning.utilities.rank_zero", rank_zero_only=ident)
        ut = standin("pytorch_lightning.utilities", rank_zero=rz)
        standin("pytorch_lightning", LightningModule=torch.nn.Module, utilities=ut)
    if absent("yacs.config"):
        standin("yacs", config=standin("yacs.config", CfgNode=dict))
    for pkg, path in (("_ref_hmr", lib), ("_ref_hmr.utils", os.path.join(lib, "utils")), ("_ref_hmr.models", os.path.join(lib, "models"))):
        standin(pkg, __path__=[path])
    sys.modules["_ref_hmr.utils"].SkeletonRenderer = sys.modules["_ref_hmr.utils"].MeshRenderer = object
    standin("_ref_hmr.utils.pylogger", get_pylogger=lambda name=None: None)
    standin("_ref_hmr.utils.misc", load_pretrained=None)
    standin("_ref_hmr.models.backbones", create_backbone=None)
    standin("_ref_hmr.models.heads", build_smpl_head=None)
    standin("_ref_hmr.models.discriminator", Discriminator=object)
    standin("_ref_hmr.models.smpl_wrapper", SMPL=object)
    ref_import._load("_ref_hmr.utils.geometry", os.path.join(lib, "utils", "geometry.py"), "_ref_hmr.utils")
    ref_import._load("_ref_hmr.utils.rotation_utils", os.path.join(lib, "utils", "rotation_utils.py"), "_ref_hmr.utils")
    losses = ref_import._load("_ref_hmr.models.losses", os.path.join(lib, "models", "losses.py"), "_ref_hmr.models")
    path_before = list(sys.path)
    mod = ref_import._load("_ref_hmr.models.tokenhmr", os.path.join(lib, "models", "tokenhmr.py"), "_ref_hmr.models")
    sys.path[:] = path_before          # tokenhmr.py:11 appends to sys.path
    return mod, losses


class _Tap(torch.nn.Module):
    """A loss module of the reference with the arguments of its last call kept."""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.calls = inner, []

    def forward(self, *a, **k):
        self.calls.append(a)
        return self.inner(*a, **k)


def run_reference(inp, loose, dtype):
    """One compute_loss call -> dict of numpy arrays: the six losses and, in the loose branch, the mutated batch tensors and the masks."""
    from tokenhmr_amd.model import ConfigNode
    mod, L = load_reference()
    cfg = ConfigNode({"MODEL": {"LOOSE_SUP": bool(loose), "LOOSE_WEIGHT": LOOSE_WEIGHT}, "LOSS_WEIGHTS": dict(LOSS_WEIGHTS)})
    ns = types.SimpleNamespace(cfg=cfg)
    if loose:          # tokenhmr.py:67-74
        ns.keypoint_3d_loss, ns.keypoint_2d_loss = L.Keypoint3DLossPCKT(loss_type="l1"), _Tap(L.Keypoint2DLossPCKT(loss_type="l1"))
        ns.smpl_parameter_loss = _Tap(L.ParameterLossPCKT())
    else:
        ns.keypoint_3d_loss, ns.keypoint_2d_loss = L.Keypoint3DLoss(loss_type="l1"), L.Keypoint2DLoss(loss_type="l1")
        ns.smpl_parameter_loss = L.ParameterLoss()
    batch, output = to_batch(inp, dtype)
    angles = []
    real_jae = mod.joint_angle_error
    mod.joint_angle_error = lambda p, g: angles.append(real_jae(p, g)) or angles[-1]
    try:
        with torch.no_grad():
            loss = mod.TokenHMR.compute_loss(ns, batch, output, train=True)
    finally:
        mod.joint_angle_error = real_jae
    assert list(output["losses"]) == list(LOSS_KEYS) and torch.equal(loss, output["losses"]["loss"])
    res = {"losses": np.array([output["losses"][k].item() for k in LOSS_KEYS], dtype=np.float64)}
    if loose:
        res["conf2d_used"] = batch["keypoints_2d"][:, :, -1].numpy()
        res["conf3d_used"] = batch["keypoints_3d"][:, :, -1].numpy()
        res["has_betas_used"] = batch["has_smpl_params"]["betas"].numpy()
        res["weak2d"] = ns.keypoint_2d_loss.calls[0][2].numpy()
        go, bp = ns.smpl_parameter_loss.calls[0], ns.smpl_parameter_loss.calls[1]          # (pred, gt, has, valid, weak, LOOSE_WEIGHT)
        res["valid_rot"] = torch.cat([go[3], bp[3]], 1).numpy()
        res["weak_rot"] = torch.cat([go[4], bp[4]], 1).numpy()
        res["angle_err"] = torch.cat(angles, 1).numpy()
        # kp2D_err is a local of compute_loss (:218-219): the same torch expression on the same inputs
        b0, o0 = to_batch(inp, dtype)
        res["kp2d_err"] = (b0["keypoints_2d"][:, :, -1] * torch.nn.functional.mse_loss(
            o0["pred_keypoints_2d"], b0["keypoints_2d"][:, :, :-1], reduction="none").sum(dim=2)).numpy()
        res["valid2d"] = (torch.from_numpy(res["kp2d_err"]) > L.kp2D_err_valid_thresh[None]).to(dtype).numpy()
    return res


def thresholds():
    _, L = load_reference()
    return {"kp2d": L.kp2D_err_valid_thresh.numpy().astype(np.float32), "body_pose": L.angle_valid_thresh["body_pose"].numpy().astype(np.float32),
            "global_orient": L.angle_valid_thresh["global_orient"].numpy().astype(np.float32)}


def compute(verbose=True):
    _, L = load_reference()
    inp = make_inputs(BATCH, SEED)
    th = thresholds()
    out = {"in." + k: v for k, v in inp.items() if k != "dataset"}
    out["in.dataset"] = np.array(inp["dataset"])
    out["in.valid_3d"] = np.array([n in ("H36M-TRAIN-WMASK", "BEDLAM") for n in inp["dataset"]], dtype=np.float32)
    out.update({"thresh." + k: v for k, v in th.items()})
    out["loss_weights"] = np.array([LOSS_WEIGHTS[k] for k in ("KEYPOINTS_2D", "KEYPOINTS_3D", "GLOBAL_ORIENT", "BODY_POSE", "BETAS")], dtype=np.float64)
    out["loose_weight"] = np.array(LOOSE_WEIGHT, dtype=np.float64)
    runs = {}
    for mode, loose in (("plain", False), ("loose", True)):
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            r = runs[(mode, tag)] = run_reference(inp, loose, dtype)
            for k, v in r.items():
                out[f"{mode}.{tag}.{k}"] = v
    # the acceptance rule of the seed
    a32, a64 = runs[("loose", "f32")], runs[("loose", "f64")]
    ang_thr = np.concatenate([th["global_orient"], th["body_pose"]]).astype(np.float64)
    for name, thr in (("angle_err", ang_thr), ("kp2d_err", th["kp2d"].astype(np.float64))):
        d = np.abs(a32[name].astype(np.float64) - a64[name]).max()
        gap = np.abs(a64[name] - thr[None])
        if name == "kp2d_err":
            gap = gap[inp["gt_keypoints_2d"][:, :, 2] > 0]          # confidence 0: the error is exactly 0 in every precision
        out[f"margin.{name}.d_ref"], out[f"margin.{name}.min_gap"] = np.array(d), np.array(gap.min())
        if verbose:
            print(f"{name}: reference fp32 vs fp64 {d:.2e}, smallest |value - thresh| {gap.min():.2e}")
        assert gap.min() > 4 * d, f"seed {SEED} puts a {name} within 4 x fp32 error of its threshold: choose another"
    for k in ("valid2d", "weak2d", "valid_rot", "weak_rot", "conf2d_used", "conf3d_used", "has_betas_used"):
        assert np.array_equal(a32[k].astype(np.float64), a64[k]), f"the reference's fp32 and fp64 {k} differ: choose another seed"
    if verbose:
        has = np.stack([inp["has_global_orient"]] + [inp["has_body_pose"]] * 23, 1)
        print(f"valid side: {100 * (a64['angle_err'] > ang_thr[None]).mean():.0f} % of the angle entries, "
              f"{100 * a64['valid2d'].mean():.0f} % of the 2D entries; weak_rot set on {int((a64['weak_rot'] * has).sum())} joints")
        for mode in ("plain", "loose"):
            print(mode, "fp64:", " ".join(f"{v:.6f}" for v in runs[(mode, "f64")]["losses"]),
                  "| fp32-fp64 rel:", " ".join(f"{abs(a - b) / max(abs(b), 1e-30):.1e}" for a, b in zip(runs[(mode, "f32")]["losses"], runs[(mode, "f64")]["losses"])))
    probs, tgt = token_inputs()
    tl = L.TokenLoss()
    out["token.seed"], out["token.rows"] = np.array(TOKEN_SEED), np.array(TOKEN_ROWS)
    out["token.f32"] = np.array(tl(probs.view(3, 160, 2048), tgt.view(3, 160)).item(), dtype=np.float64)
    out["token.f64"] = np.array(tl(probs.double().view(3, 160, 2048), tgt.view(3, 160)).item(), dtype=np.float64)
    if verbose:
        print(f"TokenLoss fp32 {out['token.f32']:.8f} fp64 {out['token.f64']:.10f}")
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
            if v.dtype.kind in "US" or k.startswith(("in.", "thresh.", "loss_w", "loose_w", "token.seed", "token.rows")):
                assert np.array_equal(old[k], v), k
            elif ".f64" in k:
                assert np.allclose(old[k], v, rtol=1e-12, atol=1e-14), k
            else:       # float32 arithmetic of another host's torch build: to rounding of the fp32 sums
                assert np.allclose(old[k], v, rtol=2e-6, atol=1e-7), k
        print("val_loss.npz: the reference reproduces the committed fixture")
        return
    np.savez_compressed(OUT, **new)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
