"""Value and gradient of compute_loss down to the head's outputs, next to the same chain in torch ops under torch autograd, on one box, in
one process, interleaved (profiles/loss_grad.jsonl).  Needs a GPU; reads nothing outside the repository.

At 1, 8, 64 and 256 items, plain and loose branch, ms per call between device events around `iters` back-to-back calls; the arms alternate,
`reps` windows each, the order reversed every other repetition, one untimed call after each switch:

  vg_eager      ValidationLoss.value_and_grad with a body model, end to end on a forward's output (prepare, thmr_val_loss,
                thmr_val_loss_grad, thmr_smpl_backward, two adds)
  vg_graph      the same call captured in a torch.cuda.graph and replayed (plain branch only: prepare() uploads valid_3d from the host in
                the loose branch, which a capture refuses)
  torch_chain   the same chain in torch ops on the device under torch autograd: torch LBS (24 joints, the 44 keypoints), pred_cam_t, the
                projection, the five loss terms with the masks of the loose branch as constants, torch.autograd.grad by global_orient,
                body_pose, betas and pred_cam
  value         thmr_val_loss alone (ValidationLoss.__call__): the cost of the value

vg_* exclude the body model's forward (value_and_grad takes a forward's output; thmr_smpl_backward recomputes what it needs);
torch_chain includes it, as autograd must.  Nothing is tuned per arm; no number is a target.

    python scripts/loss_grad_bench.py [--reps 7] [--iters 20] [--out profiles/loss_grad.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def torch_smpl(R, betas, s):
    """smplx lbs for 24 joints + the 44 keypoints of the SMPL wrapper on the device of R: (B,24,3,3), (B,10) -> joints (B,44,3)."""
    import torch
    import torch.nn.functional as F
    B, nj = R.shape[0], 24
    v_shaped = s["v_template"][None] + torch.einsum("bl,vkl->bvk", betas, s["shapedirs"])
    J = torch.einsum("bik,ji->bjk", v_shaped, s["J_regressor"])
    pose_feature = (R[:, 1:] - torch.eye(3, device=R.device)).reshape(B, -1)
    v_posed = v_shaped + torch.matmul(pose_feature, s["posedirs"]).reshape(B, -1, 3)
    parents = s["parents_list"]
    rel = torch.cat([J[:, :1], J[:, 1:] - J[:, parents[1:]]], dim=1)
    T = torch.cat([torch.cat([R, rel.unsqueeze(-1)], dim=3), s["row"].expand(B, nj, 1, 4)], dim=2)
    chain = [T[:, 0]]
    for i in range(1, nj):
        chain.append(torch.matmul(chain[parents[i]], T[:, i]))
    G = torch.stack(chain, dim=1)
    A = G - F.pad(torch.matmul(G, F.pad(J, [0, 1]).unsqueeze(-1)), [3, 0])
    Tv = torch.matmul(s["lbs_weights"][None].expand(B, -1, -1), A.reshape(B, nj, 16)).reshape(B, -1, 4, 4)
    vh = torch.cat([v_posed, torch.ones(B, v_posed.shape[1], 1, device=R.device)], dim=2)
    verts = torch.matmul(Tv, vh.unsqueeze(-1))[:, :, :3, 0]
    j45 = torch.cat([G[:, :, :3, 3], verts[:, s["extra_verts"]]], dim=1)[:, s["joint_map"]]
    return torch.cat([j45, torch.einsum("ji,bik->bjk", s["J19_regressor"], verts)], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 8, 64, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_grad.jsonl"))
    a = ap.parse_args()

    import numpy as np
    import torch
    import gen_golden_val_loss as GV
    import gen_golden_val_loss_grad as GG
    import val_loss_oracle as VO
    from tokenhmr_amd.losses import ValidationLoss
    from tokenhmr_amd.model import ConfigNode
    from tokenhmr_amd.smpl import SMPL
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl

    if not torch.cuda.is_available():
        sys.exit("loss_grad_bench: needs a GPU (no CPU fallback, no CPU timing)")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    g = np.load(os.path.join(ROOT, "tests", "golden", "val_loss_grad.npz"))
    th = {k[7:]: g[k] for k in g.files if k.startswith("thresh.")}
    F_, S_ = GG.FOCAL_LENGTH, GG.IMAGE_SIZE
    smpl = make_synthetic_smpl(seed=0)
    m = SMPL(smpl, max_batch=max(a.sizes), device=dev).enable_grad()
    build = m.lib.thmr_build_info().decode()
    s = {k: v.to(dev) for k, v in smpl.items() if torch.is_tensor(v) and v.is_floating_point()}
    s.update(extra_verts=smpl["extra_verts"].long().to(dev), joint_map=smpl["joint_map"].long().to(dev),
             parents_list=[int(q) for q in smpl["parents"]], row=torch.tensor([0.0, 0.0, 0.0, 1.0], device=dev))
    assert not smpl.get("update_hips", False)
    w2, w3, wgo, wbp, wb = (GV.LOSS_WEIGHTS[k] for k in ("KEYPOINTS_2D", "KEYPOINTS_3D", "GLOBAL_ORIENT", "BODY_POSE", "BETAS"))
    weights = [w2, w3, wgo, wbp, wb]
    lw = GV.LOOSE_WEIGHT

    for B in a.sizes:
        for mode in ("plain", "loose"):
            loose = mode == "loose"
            inp = GG.make_inputs(B, 6000 + B, thresholds=th)
            # a forward's output: the keypoints of the body model on the predicted pose, projected
            R = torch.from_numpy(inp["pred_rotmat"]).to(dev)
            betas = torch.from_numpy(inp["pred_betas"]).to(dev)
            cam = torch.from_numpy(inp["pred_cam"]).to(dev)
            with torch.no_grad():
                joints = m(R[:, :1], R[:, 1:], betas, pose2rot=False).joints
                t = torch.stack([cam[:, 1], cam[:, 2], 2 * F_ / (S_ * cam[:, 0] + 1e-9)], -1)
                X = joints + t[:, None]
                kp2d = (F_ / S_) * X[:, :, :2] / X[:, :, 2:]
            inp["pred_keypoints_3d"], inp["pred_keypoints_2d"] = joints.cpu().numpy(), kp2d.cpu().numpy()
            batch, output = GV.to_batch(inp, torch.float32)
            flags = batch.pop("smpl_params_is_axis_angle")
            mv = lambda d: {k: (mv(v) if isinstance(v, dict) else v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}      # noqa: E731
            batch, output = mv(batch), mv(output)
            batch["smpl_params_is_axis_angle"] = flags
            output["pred_cam"] = cam
            cfg = ConfigNode({"MODEL": {"LOOSE_SUP": loose, "LOOSE_WEIGHT": lw}, "LOSS_WEIGHTS": dict(GV.LOSS_WEIGHTS)})
            vl = ValidationLoss(cfg, thresholds=th)

            def vg_eager():
                return vl.value_and_grad(batch, output, body_model=m, train=loose, focal_length=F_, image_size=S_)

            def value():
                return vl(batch, output, train=loose)

            # the masks of this input, as constants of the torch chain (the device recomputes them in its kernel)
            fwd = VO.val_loss64(inp, weights, loose=loose, loose_weight=lw, thresholds=th, valid_3d=GG.valid_3d(inp))
            d_ = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)      # noqa: E731
            g2, g3, gb = d_(inp["gt_keypoints_2d"]), d_(inp["gt_keypoints_3d"]), d_(inp["gt_betas"])
            Rg = d_(inp["gt_pose_rotmat"])
            has = torch.cat([d_(inp["has_global_orient"])[:, None], d_(inp["has_body_pose"])[:, None].repeat(1, 23)], 1)
            if loose:
                c2, c3 = d_(fwd["conf2d_used"] + lw * fwd["weak2d"]), d_(fwd["conf3d_used"])
                mr, hb = d_(fwd["valid_rot"] + lw * fwd["weak_rot"]), d_(fwd["has_betas_used"])
            else:
                c2, c3, mr, hb = g2[:, :, 2], g3[:, :, 3], has, d_(inp["has_betas"])
            leaves = [R[:, :1].clone().requires_grad_(True), R[:, 1:].clone().requires_grad_(True), betas.clone().requires_grad_(True),
                      cam.clone().requires_grad_(True)]

            def torch_chain():
                go, bp, be, cm = leaves
                Rr = torch.cat([go, bp], 1)
                j = torch_smpl(Rr, be, s)
                tr = torch.stack([cm[:, 1], cm[:, 2], 2 * F_ / (S_ * cm[:, 0] + 1e-9)], -1)
                Xc = j + tr[:, None]
                k2 = (F_ / S_) * Xc[:, :, :2] / Xc[:, :, 2:]
                l2 = (c2[:, :, None] * (k2 - g2[:, :, :2]).abs()).sum()
                l3 = (c3[:, :, None] * ((j - j[:, 39:40]) - (g3[:, :, :3] - g3[:, 39:40, :3])).abs()).sum()
                sq = ((Rr - Rg) ** 2).sum((2, 3))
                total = w3 * l3 + w2 * l2 + wgo * (mr[:, :1] * sq[:, :1]).sum() + wbp * (mr[:, 1:] * sq[:, 1:]).sum() + \
                    wb * (hb[:, None] * (be - gb) ** 2).sum()
                return total, torch.autograd.grad(total, leaves)

            arms = {"vg_eager": vg_eager, "torch_chain": torch_chain, "value": value}
            vg_eager()
            torch.cuda.synchronize()
            graph = None
            if not loose:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    vg_eager()
                arms["vg_graph"] = graph.replay
            # the two chains compute the same thing (a check, not a tolerance test: tests/test_gpu_val_loss_grad.py holds the bound)
            (ld, gd), (tt, tg) = vg_eager(), torch_chain()
            agree = {"loss": float((ld["loss"] - tt.detach()).abs() / tt.detach().abs()),
                     "grad": max(float((gd[k] - x).abs().max() / x.abs().max()) for k, x in zip(("global_orient", "body_pose", "betas", "pred_cam"), tg))}
            ms = {k: [] for k in arms}
            for f in arms.values():
                for _ in range(3):
                    f()
            torch.cuda.synchronize()
            names = list(arms)
            for rep in range(a.reps):
                for name in (names if rep % 2 == 0 else names[::-1]):
                    f = arms[name]
                    f()                                                     # one untimed call after the switch
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        f()
                    e1.record()
                    torch.cuda.synchronize()
                    ms[name].append(e0.elapsed_time(e1) / a.iters)
            med = {k: statistics.median(v) for k, v in ms.items()}
            rec = {"what": "compute_loss value and gradient down to the head's outputs, ms per call between device events, arms interleaved",
                   "build": build, "items": B, "mode": mode, "reps": a.reps, "iters_per_window": a.iters, "gpu": torch.cuda.get_device_name(0),
                   "ms_median": {k: round(v, 4) for k, v in med.items()},
                   "ms_spread": {k: round((max(v) - min(v)) / 2, 4) for k, v in ms.items()},
                   "ms_windows": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                   "torch_over_vg_eager": round(med["torch_chain"] / med["vg_eager"], 2),
                   "torch_over_vg_graph": round(med["torch_chain"] / med["vg_graph"], 2) if graph is not None else None,
                   "chains_max_rel_diff": agree}
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
            print(json.dumps({k: v for k, v in rec.items() if k != "ms_windows"}), flush=True)
            del graph
    m.close()


if __name__ == "__main__":
    main()
