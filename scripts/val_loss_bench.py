"""Times the fused validation loss (thmr_val_loss) against the same arithmetic written as torch ops on device tensors — what the
reference's compute_loss launches — and thmr_op_token_ce against torch.nn.functional.cross_entropy, in one process on one GPU.

    python scripts/val_loss_bench.py [--out profiles/val_loss.jsonl] [--calls 200] [--rounds 7]

Per shape (1, 8, 64 items; plain and loose mode) the two arms alternate `rounds` times; a window is `calls` back-to-back calls between
two device events.  Two figures per arm: "eager" (what a caller gets: host enqueue and device time overlap, the larger one shows) and
"graph" (20 calls captured in one graph, replayed `calls` / 20 times: the device-side time of the launch chain without the host).  Median, minimum and
maximum over the rounds are written, so the spread is on record next to every number.  The torch arm is checked against the fused arm
before it is timed.  token_ce's bytes/s are its algorithmic bytes (the matrix once, targets, row losses) over the graph-replayed call
time, which includes the one-workgroup final reduction: a lower bound of the row kernel's own rate.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import gen_golden_val_loss as GV          # noqa: E402
from tokenhmr_amd import ops          # noqa: E402

WEIGHTS = [GV.LOSS_WEIGHTS[k] for k in ("KEYPOINTS_2D", "KEYPOINTS_3D", "GLOBAL_ORIENT", "BODY_POSE", "BETAS")]
KEYS = ("pred_keypoints_2d", "pred_keypoints_3d", "pred_rotmat", "pred_betas", "gt_keypoints_2d", "gt_keypoints_3d", "gt_pose_aa", "gt_betas",
        "has_global_orient", "has_body_pose", "has_betas")


# ---- the torch arm: compute_loss (tokenhmr.py:190-277) with its helpers, op for op, on device tensors ----
def t_aa_to_rotmat(theta):                                              # geometry.py:5-44
    angle = torch.norm(theta + 1e-8, p=2, dim=1).unsqueeze(-1)
    q = torch.cat([torch.cos(angle * 0.5), torch.sin(angle * 0.5) * (theta / angle)], 1)
    q = q / q.norm(p=2, dim=1, keepdim=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    w2, x2, y2, z2, wx, wy, wz, xy, xz, yz = w * w, x * x, y * y, z * z, w * x, w * y, w * z, x * y, x * z, y * z
    return torch.stack([w2 + x2 - y2 - z2, 2 * xy - 2 * wz, 2 * wy + 2 * xz, 2 * wz + 2 * xy, w2 - x2 + y2 - z2, 2 * yz - 2 * wx,
                        2 * xz - 2 * wy, 2 * wx + 2 * yz, w2 - x2 - y2 + z2], 1).view(-1, 3, 3)


def t_matrix_to_axis_angle(m):                                          # rotation_utils.py:104-163, 478-506
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = torch.unbind(m.reshape(-1, 9), -1)
    q_abs = torch.sqrt(torch.clamp(torch.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], -1), min=0))
    cand = torch.stack([torch.stack([q_abs[:, 0] ** 2, m21 - m12, m02 - m20, m10 - m01], -1),
                        torch.stack([m21 - m12, q_abs[:, 1] ** 2, m10 + m01, m02 + m20], -1),
                        torch.stack([m02 - m20, m10 + m01, q_abs[:, 2] ** 2, m12 + m21], -1),
                        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[:, 3] ** 2], -1)], -2)
    cand = cand / (2.0 * q_abs[:, :, None].clamp(min=0.1))
    # (the reference selects with boolean masks, which synchronise; gather / where keep this arm free of host round trips and capturable)
    q = cand.gather(1, q_abs.argmax(-1)[:, None, None].expand(-1, 1, 4)).squeeze(1)
    norms = torch.norm(q[:, 1:], p=2, dim=-1, keepdim=True)
    half = torch.atan2(norms, q[:, :1])
    angles = 2 * half
    so = torch.where(angles.abs() < 1e-6, 0.5 - (angles * angles) / 48, torch.sin(half) / angles)
    return q[:, 1:] / so.clamp(min=torch.finfo(torch.float32).tiny)


def torch_compute_loss(t, loose, thr2, thr_a, valid_3d):
    p2, p3, R, pb, g2, g3, aa, gb, has_go, has_bp, has_b = [t[k] for k in KEYS]
    B = p2.shape[0]
    l1 = torch.nn.functional.l1_loss
    mse = torch.nn.functional.mse_loss
    Rg = t_aa_to_rotmat(aa.reshape(-1, 3)).view(B, 24, 3, 3)
    conf2, conf3 = g2[:, :, -1], g3[:, :, -1]
    if loose:
        err = conf2 * mse(p2, g2[:, :, :-1], reduction="none").sum(2)
        valid2 = err > thr2[None]
        weak2 = conf2 * (~valid2).float()
        conf2 = conf2 * valid2
        e = l1(p2, g2[:, :, :-1], reduction="none")
        loss2 = (conf2.unsqueeze(-1) * e).sum() + GV.LOOSE_WEIGHT * (weak2.unsqueeze(-1) * e).sum()
        conf3 = conf3 * ((valid_3d.unsqueeze(-1) + conf2) > 0.5)
    else:
        loss2 = (conf2.unsqueeze(-1) * l1(p2, g2[:, :, :-1], reduction="none")).sum()
    pp = p3 - p3[:, 39:40]
    gg = g3[:, :, :-1] - g3[:, 39:40, :-1]
    loss3 = (conf3.unsqueeze(-1) * l1(pp, gg, reduction="none")).sum()
    sq = mse(R, Rg, reduction="none").sum((2, 3))
    has = torch.cat([has_go[:, None], has_bp[:, None].expand(B, 23)], 1)
    if loose:
        r = R.reshape(-1, 3, 3) @ Rg.reshape(-1, 3, 3).permute(0, 2, 1)
        angle = torch.linalg.norm(t_matrix_to_axis_angle(r), dim=-1).reshape(B, 24)
        valid = ((angle > thr_a[None]) * has + valid_3d.unsqueeze(1)).bool()
        weak = (~valid * has).float()
        per = valid.float() * sq
        wk = weak * sq
        lgo, lbp = per[:, 0].sum() + GV.LOOSE_WEIGHT * wk[:, 0].sum(), per[:, 1:].sum() + GV.LOOSE_WEIGHT * wk[:, 1:].sum()
        has_b = has_b * valid_3d
    else:
        per = has * sq
        lgo, lbp = per[:, 0].sum(), per[:, 1:].sum()
    lb = (has_b[:, None] * mse(pb, gb, reduction="none")).sum()
    loss = WEIGHTS[1] * loss3 + WEIGHTS[0] * loss2 + (lgo * WEIGHTS[2] + lbp * WEIGHTS[3] + lb * WEIGHTS[4])
    return torch.stack([loss, loss2, loss3, lgo, lbp, lb])


# ---- timing ----
def count_kernels(fn):
    """Device kernels one call launches, from the profiler; None where the profiler is not available."""
    try:
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return int(sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)) or None
    except Exception:
        return None


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


GRAPH_CALLS = 20      # calls per captured graph: a replay costs the host ~10 us whatever it holds, which must not be read as device time


def graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(GRAPH_CALLS):
            fn()
    return g.replay


def time_arms(arms, calls, rounds):
    """arms: name -> callable.  Alternating windows; -> name -> {'eager_us': [median, min, max], 'graph_us': [...]}."""
    replay = {n: graph_of(f) for n, f in arms.items()}
    for f in list(arms.values()) + list(replay.values()):
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    raw = {n: {"eager_us": [], "graph_us": []} for n in arms}
    for _ in range(rounds):
        for n in arms:
            raw[n]["eager_us"].append(1e3 * window_ms(arms[n], calls))
        for n in arms:
            raw[n]["graph_us"].append(1e3 * window_ms(replay[n], max(1, calls // GRAPH_CALLS)) / GRAPH_CALLS)
    return {n: {k: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)] for k, v in d.items()} for n, d in raw.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "val_loss.jsonl"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("val_loss_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(ROOT, "tests", "golden", "val_loss.npz"))
    thr2 = torch.from_numpy(g["thresh.kp2d"]).to(dev)
    thr_a = torch.from_numpy(np.concatenate([g["thresh.global_orient"], g["thresh.body_pose"]])).to(dev)
    recs = []
    for B in (1, 8, 64):
        inp = GV.make_inputs(B, 9000 + B)
        t = {k: torch.from_numpy(inp[k]).to(dev) for k in KEYS}
        v3 = torch.tensor([float(n in ("H36M-TRAIN-WMASK", "BEDLAM")) for n in inp["dataset"]], device=dev)
        ws = torch.empty(5 * B, device=dev)
        for loose in (False, True):
            kw = dict(loose=loose, loose_weight=GV.LOOSE_WEIGHT, workspace=ws, taps=False)
            if loose:
                kw.update(valid_3d=v3, kp2d_thresh=thr2, angle_thresh=thr_a)
            fused = lambda: ops.val_loss(*[t[k] for k in KEYS], WEIGHTS, **kw)["losses"]      # noqa: E731
            composed = lambda: torch_compute_loss(t, loose, thr2, thr_a, v3)      # noqa: E731
            a, b = fused().double(), composed().double()
            rel = ((a - b).abs() / b.abs().clamp(min=1e-30)).max().item()
            assert rel < 1e-5, f"the torch arm disagrees with the fused arm at {B} items: {rel:.2e}"
            n_kernels = count_kernels(composed)
            r = time_arms({"fused": fused, "torch": composed}, args.calls, args.rounds)
            rec = {"what": "val_loss", "items": B, "mode": "loose" if loose else "plain", "calls_per_window": args.calls, "rounds": args.rounds,
                   "fused_launches": 2, "torch_kernels": n_kernels, "fused_vs_torch_max_rel": rel,
                   "columns": "[median, min, max] microseconds per call", **{f"{n}_{k}": v for n, d in r.items() for k, v in d.items()},
                   "torch_arm_note": "the reference's arithmetic op for op, except that matrix_to_quaternion's boolean-mask selection "
                                     "(which synchronises) is written as argmax + gather so that the arm is capturable: a favourable "
                                     "reading of what the reference launches"}
            print(json.dumps(rec))
            recs.append(rec)
    rows = 64 * 160
    gen = torch.Generator().manual_seed(3)
    probs = (3.0 * torch.randn(rows, 2048, generator=gen)).softmax(-1).to(dev)
    tgt = torch.randint(0, 2048, (rows,), generator=gen).to(dev)
    t32 = tgt.to(torch.int32)
    out, ws = torch.empty((), device=dev), torch.empty(rows, device=dev)
    fused = lambda: ops.token_ce(probs, t32, out=out, workspace=ws)      # noqa: E731
    composed = lambda: torch.nn.functional.cross_entropy(probs, tgt)      # noqa: E731
    rel = abs(float(fused()) - float(composed())) / float(composed())
    assert rel < 1e-5, rel
    r = time_arms({"fused": fused, "torch": composed}, args.calls, args.rounds)
    nbytes = rows * 2048 * 4 + rows * 4 + rows * 4 * 2
    rec = {"what": "token_ce", "rows": rows, "calls_per_window": args.calls, "rounds": args.rounds, "algorithmic_bytes": nbytes,
           "fused_vs_torch_rel": rel, "columns": "[median, min, max] microseconds per call",
           **{f"{n}_{k}": v for n, d in r.items() for k, v in d.items()}}
    rec["GBps_note"] = ("algorithmic bytes over the whole graph-replayed call (row kernel + the one-workgroup final reduction), not over "
                        "the row kernel alone: a lower bound of the row kernel's rate")
    rec["fused_GBps_over_graph_call_time"] = [round(nbytes / (us * 1e-6) / 1e9, 1) for us in rec["fused_graph_us"]]
    rec["torch_GBps_over_graph_call_time"] = [round(nbytes / (us * 1e-6) / 1e9, 1) for us in rec["torch_graph_us"]]
    print(json.dumps(rec))
    recs.append(rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for rec in recs:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
