"""SMPL-H next to SMPL, and the tokenizer's three metrics, on one box, in one process, the arms alternating (profiles/smplh.jsonl).

Arms, at 1, 8 and 64 poses, each window `iters` back-to-back C ABI calls between device events, the arms taking turns over `reps`
windows (order reversed every other round):

  smplh_full     thmr_smplh_forward(body_only=0): 52-joint chain, K = 480 blend product, 52-joint skinning
  smplh_folded   thmr_smplh_forward(body_only=1): 22-joint chain, K = 224 blend product, 22-joint skinning  (the tokenizer's call)
  smpl_24        thmr_smpl_forward: the existing 24-joint SMPL path (prep, K = 224 blend product, skin + regressed joints)

and, at 64 poses, the three-metric evaluation (pose, mesh, joints: six launches of thmr_op_mean_row_dist).  Rotation matrices in, so no
Rodrigues launch is in any window; the same body pose feeds every arm (identity hands for the full SMPL-H arm, so that it computes what
the folded arm computes and the two are compared before they are timed).  No threshold: the parent has no SMPL-H path to compare with.

    python scripts/smplh_bench.py [--reps 7] [--iters 200] [--out profiles/smplh.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smplh.jsonl"))
    a = ap.parse_args()

    import torch
    from oracle import tokenhmr_oracle as O
    from tokenhmr_amd import _cabi
    from tokenhmr_amd.smpl import SMPL
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl, make_synthetic_smplh
    from tokenhmr_amd.smplh import SMPLHLayer

    if not torch.cuda.is_available():
        sys.exit("smplh_bench: needs a GPU (no CPU fallback, no CPU timing)")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    lib = _cabi.load()
    build = lib.thmr_build_info().decode()
    p = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731

    def emit(rec):
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)

    def time_arms(fns):
        ms = {k: [] for k in fns}
        for f in fns.values():
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        names = list(fns)
        for rep in range(a.reps):
            for name in (names if rep % 2 == 0 else names[::-1]):
                f = fns[name]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                f()                                                       # one untimed call after the switch
                e0.record()
                for _ in range(a.iters):
                    f()
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1) / a.iters)
        return ms

    BMAX = 64
    layer = SMPLHLayer(make_synthetic_smplh(0), max_batch=BMAX, device=dev)
    smpl = SMPL(make_synthetic_smpl(seed=0), max_batch=BMAX, device=dev)
    h, st = layer._handle(), None
    g = torch.Generator().manual_seed(6200)
    rot22 = O.rot6d_to_rotmat(torch.randn(BMAX * 22, 6, generator=g)).view(BMAX, 22, 3, 3)
    eye = torch.eye(3).expand(BMAX, 30, 3, 3)
    pose52 = torch.cat([rot22, eye], 1).contiguous().to(dev)
    pose22 = rot22.contiguous().to(dev)
    pose24 = torch.cat([rot22, eye[:, :2]], 1).contiguous().to(dev)
    betas = torch.randn(BMAX, 10, generator=g).to(dev)
    verts, joints = torch.empty(BMAX, 6890, 3, device=dev), torch.empty(BMAX, 73, 3, device=dev)
    verts2, joints2 = torch.empty_like(verts), torch.empty_like(joints)
    joints44 = torch.empty(BMAX, 44, 3, device=dev)

    def smplh(pose, body_only, B, v, j):
        _cabi.check(lib.thmr_smplh_forward(h, p(pose), 0, p(betas), None, body_only, B, p(v), p(j), st), lib=lib)

    for B in (1, 8, 64):
        fns = {"smplh_full": lambda: smplh(pose52, 0, B, verts, joints), "smplh_folded": lambda: smplh(pose22, 1, B, verts2, joints2),
               "smpl_24": lambda: _cabi.check(lib.thmr_smpl_forward(smpl.h, p(pose24), 0, p(betas), B, p(verts), p(joints44), st), lib=lib)}
        fns["smplh_folded"]()
        fns["smplh_full"]()
        torch.cuda.synchronize()
        d = max((verts[:B] - verts2[:B]).abs().max().item(), (joints[:B] - joints2[:B]).abs().max().item())
        if d > 1e-5:
            sys.exit(f"smplh_bench: the full and the folded path disagree at {B} poses: max|diff| {d:.3e} m")
        ms = time_arms(fns)
        rec = {"what": "ms per call, rotation matrices in: thmr_smplh_forward full (52 joints) / folded (22 joints, body_only) / thmr_smpl_forward "
                       "(24 joints), arms interleaved", "build": build, "poses": B, "reps": a.reps, "iters_per_window": a.iters,
               "gpu": torch.cuda.get_device_name(0), "full_vs_folded_max_abs_m": d}
        for name, w in ms.items():
            rec[f"{name}_ms_windows"] = [round(v, 4) for v in w]
            rec[f"{name}_ms_median"] = round(statistics.median(w), 4)
            rec[f"{name}_spread_ms"] = round((max(w) - min(w)) / 2, 4)
        rec["folded_over_full"] = round(statistics.median(ms["smplh_folded"]) / statistics.median(ms["smplh_full"]), 4)
        rec["folded_over_smpl_24"] = round(statistics.median(ms["smplh_folded"]) / statistics.median(ms["smpl_24"]), 4)
        emit(rec)

    # the three metrics of one evaluation batch at 64 poses
    B = 64
    smplh(pose22, 1, B, verts2, joints2)
    smplh(pose52, 0, B, verts, joints)
    gt_rot = pose22[:, 1:].contiguous()
    pr_rot = pose22.roll(1, 0)[:, 1:].contiguous()
    res, ws = torch.zeros(3, device=dev), torch.empty(_cabi.MEAN_ROW_DIST_WS, device=dev)
    verts_b, joints_b = verts.roll(1, 0).contiguous(), joints.roll(1, 0).contiguous()

    def metrics():
        _cabi.check(lib.thmr_op_mean_row_dist(p(gt_rot), p(pr_rot), 63, 0, 63, B, p(res[0]), p(ws), st), lib=lib)
        _cabi.check(lib.thmr_op_mean_row_dist(p(verts_b), p(verts2), 6890, 0, 6890, B, p(res[1]), p(ws), st), lib=lib)
        _cabi.check(lib.thmr_op_mean_row_dist(p(joints_b), p(joints2), 73, 1, 22, B, p(res[2]), p(ws), st), lib=lib)

    ms = time_arms({"metrics": metrics})["metrics"]
    emit({"what": "ms per evaluation batch: pose + mesh + joints errors (3 x thmr_op_mean_row_dist, results left on the device)", "build": build,
          "poses": B, "reps": a.reps, "iters_per_window": a.iters, "gpu": torch.cuda.get_device_name(0),
          "metrics_ms_windows": [round(v, 4) for v in ms], "metrics_ms_median": round(statistics.median(ms), 4),
          "metrics_spread_ms": round((max(ms) - min(ms)) / 2, 4), "values": [round(v, 6) for v in res.cpu().tolist()]})


if __name__ == "__main__":
    main()
