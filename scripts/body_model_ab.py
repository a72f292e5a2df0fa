"""The body-model kernels (csrc/body_model.hip) of two builds of the library, in one process on one box.

    python scripts/build_ab_lib.py <git-ref> parent                      # no GPU needed
    python scripts/body_model_ab.py bits [--a build_ab/parent/libtokenhmr_hip.so] [--out profiles/body_model_bit_equal.json]
    python scripts/body_model_ab.py time [--a ...] [--parent-tree build_ab/parent_tree] [--out profiles/body_model_ab_same_box.json]

bits: the same inputs and synthetic constants through library A and the in-tree library, every output compared byte for byte (output
      buffers pre-filled with one pattern, so what a call leaves unwritten compares equal too).  SMPL through thmr_smpl_forward (every
      crops-per-pass regime of launch_lbs and its ragged last group; each case twice, so the arrival counter is re-zeroed), the engine
      path (thmr_lbs_forward with a camera, thmr_forward) on a depth-1 engine, SMPL-H through thmr_smplh_forward.  The backward through
      thmr_smpl_backward (matrices and axis-angle) and thmr_smplh_backward (folded and full, both paths reserved on one handle), each at
      the smallest batch of every crops-per-workgroup value and at one batch with a ragged last group.  Exit status 1 if any byte differs.
time: thmr_smpl_forward at 1, 64, 512 crops (scripts/lbs_bench.py's call), thmr_smplh_forward full / folded at 1, 8, 64 poses
      (scripts/smplh_bench.py's calls) and the three backward calls at 64, three arms taking turns window by window: A, the in-tree library, and A AGAIN on a second handle,
      whose distance from the first is the parent's own run-to-run spread; then bench.py's default line from a built checkout of the
      parent, from this tree and from the parent's again.  Exit status 1 unless in every row the in-tree figure lies within that spread
      of the parent's.  The recorded run (profiles/body_model_ab_same_box.json) ended with status 1: 4 of 10 rows outside, three of them
      with the in-tree build the faster one, the fourth thmr_smpl_forward at 64 crops, 48.08 us against 47.56 with a spread of 0.51; the
      parent's own two handles differ by that much, their windows apart (profiles/README.md).
"""
import argparse
import ctypes as C
import itertools
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from tokenhmr_amd import _cabi  # noqa: E402
from tokenhmr_amd import weights as W  # noqa: E402
from tokenhmr_amd.config import HMRConfig  # noqa: E402
from tokenhmr_amd.engine import Engine  # noqa: E402
from tokenhmr_amd.smpl_assets import make_synthetic_smpl, make_synthetic_smplh  # noqa: E402

DEV = torch.device("cuda:0")
FKEYS = ["v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights"]


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def create(lib, consts, max_batch, smplh):
    fk = FKEYS + ([] if smplh else ["J19_regressor"])
    ik = ["parents", "extra_verts"] + ([] if smplh else ["joint_map"])
    ts = {k: consts[k].detach().float().contiguous().cpu() for k in fk}
    ts.update({k: consts[k].detach().to(torch.int32).contiguous().cpu() for k in ik})
    ptrs = {k: t.data_ptr() for k, t in ts.items()}
    d = _cabi.SmplhDesc(**ptrs, on_device=0) if smplh else _cabi.SmplDesc(**ptrs, on_device=0, update_hips=1 if consts.get("update_hips") else 0)
    h = C.c_void_p(0)
    _cabi.check((lib.thmr_smplh_create if smplh else lib.thmr_smpl_create)(C.byref(d), max_batch, 0, C.byref(h)), lib=lib)
    return h


def smpl_fwd(lib, h, pose, pose2rot, betas, B, verts, joints):
    _cabi.check(lib.thmr_smpl_forward(h, p(pose), pose2rot, p(betas), B, p(verts), p(joints), None), lib=lib)


def smplh_fwd(lib, h, pose, pose2rot, betas, transl, body_only, B, verts, joints):
    _cabi.check(lib.thmr_smplh_forward(h, p(pose), pose2rot, p(betas), p(transl), body_only, B, p(verts), p(joints), None), lib=lib)


def smpl_bwd(lib, h, pose, pose2rot, betas, B, gV, gJ, gp, gb):
    _cabi.check(lib.thmr_smpl_backward(h, p(pose), pose2rot, p(betas), B, p(gV), p(gJ), p(gp), p(gb), None), lib=lib)


def smplh_bwd(lib, h, pose, pose2rot, betas, transl, body_only, B, gV, gJ, gp, gb, gt):
    _cabi.check(lib.thmr_smplh_backward(h, p(pose), pose2rot, p(betas), p(transl), body_only, B, p(gV), p(gJ), p(gp), p(gb), p(gt), None), lib=lib)


def rotmats(n, g):
    R = torch.linalg.qr(torch.randn(n, 3, 3, generator=g))[0]
    return R * torch.linalg.det(R).sign()[:, None, None]


def differing_bytes(a, b):
    return int((a.contiguous().view(torch.uint8) != b.contiguous().view(torch.uint8)).sum().item())


def bits(libs, out):
    g = torch.Generator().manual_seed(7100)
    cases, worst = [], 0

    def record(name, outs):          # outs: {output name: (tensor of A, tensor of the in-tree library)}
        nonlocal worst
        torch.cuda.synchronize()
        diff = {k: differing_bytes(a, b) for k, (a, b) in outs.items()}
        worst = max(worst, *diff.values())
        cases.append({"case": name, "bytes": sum(a.numel() * a.element_size() for a, _ in outs.values()), "differing_bytes": diff})

    # ---- SMPL, stand-alone handle ----
    BMAX = 300
    base = make_synthetic_smpl(seed=0)
    dup = dict(base)
    dup["extra_verts"] = base["extra_verts"].clone()
    dup["extra_verts"][5] = dup["extra_verts"][2]
    dup["extra_verts"][20] = dup["extra_verts"][2]
    models = [("hips0", dict(base, update_hips=False)), ("hips1", dict(base, update_hips=True)), ("hips1_dup_extra", dict(dup, update_hips=True))]
    R = rotmats(BMAX * 24, g).reshape(BMAX, 24, 3, 3).to(DEV)
    aa = (torch.randn(BMAX, 72, generator=g) * 0.7).to(DEV)
    betas = torch.randn(BMAX, 10, generator=g).to(DEV)
    gV = torch.randn(BMAX, 6890, 3, generator=g).to(DEV)          # the backward rows' output gradients, SMPL's and (the first 256) SMPL-H's
    gJ = torch.randn(BMAX, 73, 3, generator=g).to(DEV)
    for mname, consts in models:
        hs = [create(lib, consts, BMAX, False) for lib in libs]
        for B, pose2rot in itertools.product([64] if "dup" in mname else [1, 3, 31, 32, 63, 64, 65, 100, 255, 256, 300], (0, 1)):
            for call in (1, 2):
                outs = []
                for lib, h in zip(libs, hs):
                    v, j = torch.full((B, 6890, 3), -7.5, device=DEV), torch.full((B, 44, 3), -7.5, device=DEV)
                    smpl_fwd(lib, h, (aa if pose2rot else R)[:B].contiguous(), pose2rot, betas[:B].contiguous(), B, v, j)
                    outs.append((v, j))
                record(f"smpl {mname} B={B} pose2rot={pose2rot} call={call}", {"verts": (outs[0][0], outs[1][0]), "joints": (outs[0][1], outs[1][1])})
        # thmr_smpl_backward: the smallest batch of every crops-per-pass value (1 ... 8), and 300 = 37 groups of 8 and a ragged one of 4
        for lib, h in zip(libs, hs):
            _cabi.check(lib.thmr_smpl_grad_reserve(h), lib=lib)
        for B, pose2rot in itertools.product([64] if "dup" in mname else [1, 64, 96, 128, 160, 192, 224, 256, 300], (0, 1)):
            pose = (aa if pose2rot else R)[:B].contiguous()
            outs = []
            for lib, h in zip(libs, hs):
                gp, gb = torch.full_like(pose, -7.5), torch.full((B, 10), -7.5, device=DEV)
                smpl_bwd(lib, h, pose, pose2rot, betas[:B].contiguous(), B, gV[:B].contiguous(), gJ[:B, :44].contiguous(), gp, gb)
                outs.append((gp, gb))
            record(f"smpl backward {mname} B={B} pose2rot={pose2rot}", {"grad_pose": (outs[0][0], outs[1][0]), "grad_betas": (outs[0][1], outs[1][1])})
        for lib, h in zip(libs, hs):
            lib.thmr_smpl_destroy(h)

    # ---- the engine path, depth 1 ----
    cfg = HMRConfig(vit_depth=1, dec_depth=1)
    sd, tok, smpl = W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0), make_synthetic_smpl(cfg, 0)
    engs = []
    for spec in (libs[0]._name, None):
        e = Engine(cfg, max_batch=64, device=DEV, experiments=spec)
        e.load_state(sd, tok)
        e.load_smpl(smpl)
        e.finalize()
        engs.append(e)
    cam = (torch.randn(64, 3, generator=g) * 0.1 + torch.tensor([0.9, 0.0, 0.0])).to(DEV)
    for B in (3, 64):
        res = [e.lbs_forward(R[:B].contiguous(), betas[:B].contiguous(), cam[:B].contiguous()) for e in engs]
        record(f"engine thmr_lbs_forward kp2d B={B}", {k: (res[0][i], res[1][i]) for i, k in enumerate(("verts", "joints", "cam_t", "kp2d"))})
    img = torch.randn(4, 3, 256, 256, generator=g).to(DEV)
    res = []
    for e in engs:
        res.append({k: v.clone() for k, v in e.forward(img).items() if torch.is_tensor(v)})
        e.status()
    record("engine thmr_forward B=4", {k: (res[0][k], res[1][k]) for k in res[0]})
    del engs

    # ---- SMPL-H ----
    HMAX = 256
    consts = make_synthetic_smplh(0)
    hs = [create(lib, consts, HMAX, True) for lib in libs]
    Rh = rotmats(HMAX * 52, g).reshape(HMAX, 52, 3, 3).to(DEV)
    aah = (torch.randn(HMAX, 52 * 3, generator=g) * 0.5).to(DEV)
    transl = torch.randn(HMAX, 3, generator=g).to(DEV)
    hb = torch.randn(HMAX, 10, generator=g).to(DEV)
    for body_only, B, wt, wb, wj, pose2rot in itertools.product((0, 1), [1, 5, 63, 64, 66, 127, 128, 255, 256], (0, 1), (0, 1), (0, 1), (0, 1)):
        nj = 22 if body_only else 52
        pose = (aah[:B, :nj * 3] if pose2rot else Rh[:B, :nj]).contiguous()
        outs = []
        for lib, h in zip(libs, hs):
            v, j = torch.full((B, 6890, 3), -7.5, device=DEV), torch.full((B, 73, 3), -7.5, device=DEV)
            smplh_fwd(lib, h, pose, pose2rot, hb[:B].contiguous() if wb else None, transl[:B].contiguous() if wt else None, body_only, B, v,
                      j if wj else None)
            outs.append((v, j))
        record(f"smplh {'folded' if body_only else 'full'} B={B} transl={wt} betas={wb} joints={wj} pose2rot={pose2rot}",
               {"verts": (outs[0][0], outs[1][0]), "joints": (outs[0][1], outs[1][1])})
    # thmr_smplh_backward, both paths reserved on one handle: the smallest batch of every poses-per-workgroup value (1, 2, 4, 8), and 255 =
    # 63 groups of 4 and a ragged one of 3
    for lib, h in zip(libs, hs):
        _cabi.check(lib.thmr_smplh_grad_reserve(h, 3), lib=lib)
    for body_only, B, pose2rot in itertools.product((1, 0), [1, 64, 128, 255, 256], (0, 1)):
        nj = 22 if body_only else 52
        pose = (aah[:B, :nj * 3] if pose2rot else Rh[:B, :nj]).contiguous()
        outs = []
        for lib, h in zip(libs, hs):
            grads = [torch.full_like(pose, -7.5), torch.full((B, 10), -7.5, device=DEV), torch.full((B, 3), -7.5, device=DEV)]
            smplh_bwd(lib, h, pose, pose2rot, hb[:B].contiguous(), transl[:B].contiguous(), body_only, B, gV[:B].contiguous(), gJ[:B].contiguous(),
                      *grads)
            outs.append(grads)
        record(f"smplh backward {'folded' if body_only else 'full'} B={B} pose2rot={pose2rot}",
               {k: (outs[0][i], outs[1][i]) for i, k in enumerate(("grad_pose", "grad_betas", "grad_transl"))})
    for lib, h in zip(libs, hs):
        lib.thmr_smplh_destroy(h)

    res = {"what": "body-model outputs of two builds, same inputs, one process: differing bytes per output (scripts/body_model_ab.py bits)",
           "A": libs[0].thmr_build_info().decode(), "B": libs[1].thmr_build_info().decode(), "gpu": torch.cuda.get_device_name(0),
           "cases": len(cases), "max_differing_bytes": worst, "case_list": cases}
    write(out, res, "case_list")
    print(json.dumps({k: v for k, v in res.items() if k != "case_list"}), flush=True)
    return 0 if worst == 0 else 1


def timing(libs, out, reps, iters, parent_tree, steps, warmup):
    """Exit status 1 unless, in every row, the in-tree build's figure lies within the parent's run-to-run spread of the parent's figure."""
    g = torch.Generator().manual_seed(9)
    arms = {"parent": libs[0], "new": libs[1], "parent_again": libs[0]}
    rows = []

    def windows(fns):
        ms = {k: [] for k in fns}
        for f in fns.values():
            for _ in range(30):          # a window right after an idle gap runs at ramping clocks
                f()
        torch.cuda.synchronize()
        names = list(fns)
        for rep in range(reps):
            for name in names[rep % 3:] + names[:rep % 3]:          # every arm takes every place in the turn equally often
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                fns[name]()
                e0.record()
                for _ in range(iters):
                    fns[name]()
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1) / iters * 1e3)
        return ms

    def row(what, n, unit, runs):
        # the parent's figure: the median of all its runs; its spread: how far its two timings (their medians) lie apart
        med = {k: statistics.median(v) for k, v in runs.items()}
        parent, spread = statistics.median(runs["parent"] + runs["parent_again"]), abs(med["parent"] - med["parent_again"])
        r = {"call": what, "items": n, "unit": unit, "runs": {k: [round(x, 2) for x in v] for k, v in runs.items()},
             "median": {k: round(v, 2) for k, v in med.items()}, "parent_median": round(parent, 2), "parent_spread": round(spread, 2),
             "new_minus_parent": round(med["new"] - parent, 2), "within_parent_spread": bool(abs(med["new"] - parent) <= spread)}
        rows.append(r)
        print(json.dumps({k: v for k, v in r.items() if k != "runs"}), flush=True)

    smpl = make_synthetic_smpl()
    for B in (1, 64, 512):
        hs = {k: create(lib, smpl, B, False) for k, lib in arms.items()}
        R = rotmats(B * 24, g).reshape(B, 24, 3, 3).to(DEV)
        betas = torch.randn(B, 10, generator=g).to(DEV)
        v, j = torch.empty(B, 6890, 3, device=DEV), torch.empty(B, 44, 3, device=DEV)
        row("thmr_smpl_forward", B, "us per call", windows({k: (lambda k=k: smpl_fwd(arms[k], hs[k], R, 0, betas, B, v, j)) for k in arms}))
        if B == 64:
            for k, lib in arms.items():
                _cabi.check(lib.thmr_smpl_grad_reserve(hs[k]), lib=lib)
            gp, gb = torch.empty_like(R), torch.empty_like(betas)
            row("thmr_smpl_backward", B, "us per call", windows({k: (lambda k=k: smpl_bwd(arms[k], hs[k], R, 0, betas, B, v, j, gp, gb)) for k in arms}))
        for k, lib in arms.items():
            lib.thmr_smpl_destroy(hs[k])
    consts = make_synthetic_smplh(0)
    hs = {k: create(lib, consts, 64, True) for k, lib in arms.items()}
    Rh = rotmats(64 * 52, g).reshape(64, 52, 3, 3)
    Rh[:, 22:] = torch.eye(3)
    Rh = Rh.to(DEV)
    R22 = Rh[:, :22].contiguous()
    hb = torch.randn(64, 10, generator=g).to(DEV)
    v, j = torch.empty(64, 6890, 3, device=DEV), torch.empty(64, 73, 3, device=DEV)
    for B in (1, 8, 64):
        row("thmr_smplh_forward full", B, "us per call", windows({k: (lambda k=k: smplh_fwd(arms[k], hs[k], Rh, 0, hb, None, 0, B, v, j)) for k in arms}))
        row("thmr_smplh_forward folded", B, "us per call", windows({k: (lambda k=k: smplh_fwd(arms[k], hs[k], R22, 0, hb, None, 1, B, v, j)) for k in arms}))
    # the backward at 64 poses, the forward's last outputs as its output gradients
    for k, lib in arms.items():
        _cabi.check(lib.thmr_smplh_grad_reserve(hs[k], 3), lib=lib)
    gb, gt = torch.empty_like(hb), torch.empty(64, 3, device=DEV)
    for name, pose, body_only in (("full", Rh, 0), ("folded", R22, 1)):
        gp = torch.empty_like(pose)
        row(f"thmr_smplh_backward {name}", 64, "us per call",
            windows({k: (lambda k=k: smplh_bwd(arms[k], hs[k], pose, 0, hb, None, body_only, 64, v, j, gp, gb, gt)) for k in arms}))
    for k, lib in arms.items():
        lib.thmr_smplh_destroy(hs[k])

    # the 64-crop line of bench.py: the parent's built checkout, this tree, the parent's again, each a child process of its own
    lines = {}
    for arm, tree in (("parent", parent_tree), ("new", ROOT), ("parent_again", parent_tree)):
        cp = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                            stdout=subprocess.PIPE, text=True, timeout=420)
        if cp.returncode != 0:
            sys.exit(f"body_model_ab: bench.py in {tree} ended with status {cp.returncode}; nothing more is started")
        lines[arm] = json.loads([ln for ln in cp.stdout.splitlines() if ln.startswith("{") and '"value"' in ln][-1])
    row("bench.py", 64, "crops/s", {k: [ln["value"]] for k, ln in lines.items()})
    rows[-1]["builds"] = {k: ln.get("build") for k, ln in lines.items()}

    ok = all(r["within_parent_spread"] for r in rows)
    write(out, {"what": "three arms taking turns in one session on one box: the parent build, the in-tree build, the parent again (a second "
                        "handle / a second process); condition per row: |median(new) - median(all parent runs)| <= |median(parent) - "
                        "median(parent_again)| (scripts/body_model_ab.py time)",
                "parent": libs[0].thmr_build_info().decode(), "new": libs[1].thmr_build_info().decode(), "gpu": torch.cuda.get_device_name(0),
                "windows_per_arm": reps, "calls_per_window": iters, "bench_steps": steps, "bench_warmup": warmup,
                "every_row_within_parent_spread": ok, "rows": rows}, "rows")
    print(json.dumps({"every_row_within_parent_spread": ok}), flush=True)
    return 0 if ok else 1


def write(path, res, listkey):
    """Pretty-printed, except the list under `listkey`: one line per entry."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    head = json.dumps({k: v for k, v in res.items() if k != listkey}, indent=1)
    body = ",\n".join("  " + json.dumps(c) for c in res[listkey])
    with open(path, "w") as f:
        f.write(head[:-2] + f',\n "{listkey}": [\n{body}\n ]\n}}\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["bits", "time"])
    ap.add_argument("--a", default=os.path.join(ROOT, "build_ab", "parent", "libtokenhmr_hip.so"))
    ap.add_argument("--reps", type=int, default=9, help="time: windows per arm")
    ap.add_argument("--iters", type=int, default=200, help="time: calls per window")
    ap.add_argument("--parent-tree", default=os.path.join(ROOT, "build_ab", "parent_tree"), help="time: a BUILT checkout of the other commit, for its bench.py line")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("body_model_ab: needs a GPU")
    if not os.path.exists(a.a):
        sys.exit(f"body_model_ab: {a.a} does not exist (python scripts/build_ab_lib.py <git-ref> parent)")
    libs = [_cabi.load(os.path.abspath(a.a)), _cabi.load()]
    if a.mode == "bits":
        return bits(libs, a.out or os.path.join(ROOT, "profiles", "body_model_bit_equal.json"))
    if not os.path.exists(os.path.join(a.parent_tree, "bench.py")):
        sys.exit(f"body_model_ab: {a.parent_tree} is no checkout (git archive <git-ref> | tar -x -C it, then python __graft_entry__.py in it)")
    return timing(libs, a.out or os.path.join(ROOT, "profiles", "body_model_ab_same_box.json"), a.reps, a.iters, a.parent_tree, a.steps, a.warmup)


if __name__ == "__main__":
    sys.exit(main())
