"""SMPL-H's backward and the tokenizer's reconstruction objective next to torch autograd on one box, in one process, interleaved
(profiles/smplh_grad.jsonl).  Needs a GPU; reads nothing outside the repository.

At 1, 8, 64 and 256 poses, rotation-matrix input, ms per call between device events around `iters` back-to-back calls; the arms alternate,
`reps` windows each, the order reversed every other repetition, one untimed call after each switch:

  fwd_folded / fwd_full          thmr_smplh_forward alone (the C call), body_only = 1 / 0
  fwdbwd_folded / fwdbwd_full    the same + thmr_smplh_backward, both gradients in, pose / betas / transl gradients out (the C calls)
  vg_eager                       PoseReConsLoss.value_and_grad end to end (release weights, l2 / l1 / l2, valid joints) on a forward output
  vg_graph                       the same call captured in a torch.cuda.graph and replayed
  torch_chain                    the same chain in torch ops on the device under torch autograd: 6D -> rotation matrices -> the 52-joint
                                 model with identity hands -> the three terms -> torch.autograd.grad by the 6D pose
  with --parent-lib PATH (another build of this library, scripts/build_ab_lib.py), a second group of arms interleaved among themselves in
  the same session, each pair on two handles created the same way:
  pair_fwd_folded / parent_fwd_folded, pair_fwd_full / parent_fwd_full   thmr_smplh_forward of this build and of that one (untouched)
  smpl_fwdbwd / parent_smpl_fwdbwd   thmr_smpl_forward + thmr_smpl_backward of this build and of that one (SMPL's instantiation)

fwdbwd - fwd is the backward alone.  vg_* exclude the forward (value_and_grad takes its output); torch_chain includes forward and backward,
so the comparison line is vg_eager + fwd_folded against torch_chain.  Nothing is tuned per arm; no number is a target.

    python scripts/smplh_grad_bench.py [--reps 7] [--iters 20] [--parent-lib build_ab/parent/libtokenhmr_hip.so] [--out profiles/smplh_grad.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_smplh(R, s):
    """smplx lbs + VertexJointSelector for 52 joints on the device of R, betas zero: (B,52,3,3) -> verts, joints."""
    import torch
    import torch.nn.functional as F
    B, nj = R.shape[0], 52
    v_shaped = s["v_template"][None].expand(B, -1, -1)
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
    return verts, torch.cat([G[:, :, :3, 3], verts[:, s["extra_verts"]]], dim=1)


def torch_rot6d(x):
    import torch
    import torch.nn.functional as F
    a1, a2 = x[..., :3], x[..., 3:]
    b1 = F.normalize(a1, dim=-1)
    b2 = F.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 8, 64, 256])
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smplh_grad.jsonl"))
    a = ap.parse_args()

    import numpy as np
    import torch
    from oracle.lbs_independent import random_rotations
    from tokenhmr_amd import _cabi, ops
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl, make_synthetic_smplh
    from tokenhmr_amd.smplh import SMPLHLayer
    from tokenhmr_amd.tokenizer_loss import PoseReConsLoss

    if not torch.cuda.is_available():
        sys.exit("smplh_grad_bench: needs a GPU (no CPU fallback, no CPU timing)")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    MB = max(a.sizes)
    c = make_synthetic_smplh(seed=0)
    m = SMPLHLayer(c, max_batch=MB, device=dev).enable_grad()
    lib = m.lib
    build = lib.thmr_build_info().decode()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)      # noqa: E731
    s = {k: v.to(dev) for k, v in c.items() if torch.is_tensor(v) and v.is_floating_point()}
    s.update(extra_verts=c["extra_verts"].long().to(dev), parents_list=[int(q) for q in c["parents"]],
             row=torch.tensor([0.0, 0.0, 0.0, 1.0], device=dev))
    params = dict(POSE_LOSS="l2", MESH_LOSS="l1", JNT_LOSS="l2", ONLY_VALID_JNT=True, POSE_LOSS_WT=20.0, JNT_LOSS_WT=100.0,
                  MESH_LOSS_WT=100.0, COMMIT_LOSS_WT=1.0, LOSS_WT=1.0)
    loss = PoseReConsLoss(params, 21, "rotmat", "smplh", body_model=m, device=dev)
    w = loss.weights

    # handles on the parent's build, and SMPL on both builds
    smpl = make_synthetic_smpl(seed=0)
    smpl["update_hips"] = True

    def raw_handles(L):
        keep = []

        def desc(cls, consts, keys, ikeys, **kw):
            ts = {k: consts[k].detach().float().contiguous().cpu() for k in keys}
            ts.update({k: consts[k].detach().to(torch.int32).contiguous().cpu() for k in ikeys})
            keep.append(ts)
            return cls(**{k: ts[k].data_ptr() for k in keys + ikeys}, on_device=0, **kw)

        hh, hs = C.c_void_p(), C.c_void_p()
        dh = desc(_cabi.SmplhDesc, c, ["v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights"], ["parents", "extra_verts"])
        ds = desc(_cabi.SmplDesc, smpl, ["v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights", "J19_regressor"],
                  ["parents", "extra_verts", "joint_map"], update_hips=1)
        assert L.thmr_smplh_create(C.byref(dh), MB, 0, C.byref(hh)) == 0 and L.thmr_smpl_create(C.byref(ds), MB, 0, C.byref(hs)) == 0
        assert L.thmr_smpl_grad_reserve(hs) == 0
        return hh, hs

    own = raw_handles(lib)
    parent, parent_build = None, None
    if a.parent_lib:
        PL = _cabi.load(exp=a.parent_lib)
        parent, parent_build = (PL,) + raw_handles(PL), PL.thmr_build_info().decode()

    for B in a.sizes:
        rng = np.random.default_rng(B)
        R52 = torch.from_numpy(random_rotations(B * 52, seed=B).reshape(B, 52, 3, 3)).float().to(dev)
        R22 = R52[:, :22].contiguous()
        R24 = torch.from_numpy(random_rotations(B * 24, seed=B + 1).reshape(B, 24, 3, 3)).float().to(dev)
        betas = torch.from_numpy(rng.standard_normal((B, 10))).float().to(dev)
        transl = torch.from_numpy(rng.standard_normal((B, 3))).float().to(dev)
        gV = torch.from_numpy(rng.standard_normal((B, 6890, 3))).float().to(dev)
        gJ = torch.from_numpy(rng.standard_normal((B, 73, 3))).float().to(dev)
        gJ44 = gJ[:, :44].contiguous()
        verts, joints, joints44 = torch.empty(B, 6890, 3, device=dev), torch.empty(B, 73, 3, device=dev), torch.empty(B, 44, 3, device=dev)
        g52, g22, g24, gb, gt = torch.empty_like(R52), torch.empty_like(R22), torch.empty_like(R24), torch.empty_like(betas), torch.empty_like(transl)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def fwd(L, h, R, body_only):
            assert L.thmr_smplh_forward(h, p(R), 0, p(betas), p(transl), body_only, B, p(verts), p(joints), st) == 0

        def fwdbwd(R, g, body_only):
            fwd(lib, m.h, R, body_only)
            assert lib.thmr_smplh_backward(m.h, p(R), 0, p(betas), p(transl), body_only, B, p(gV), p(gJ), p(g), p(gb), p(gt), st) == 0

        def smpl_fwdbwd(L, h):
            assert L.thmr_smpl_forward(h, p(R24), 0, p(betas), B, p(verts), p(joints44), st) == 0
            assert L.thmr_smpl_backward(h, p(R24), 0, p(betas), B, p(gV), p(gJ44), p(g24), p(gb), st) == 0

        x6d = torch.from_numpy(rng.standard_normal((B, 21, 6))).float().to(dev)
        with torch.no_grad():
            gt_rot = ops.rot6d_to_rotmat(x6d + 0.2).view(B, 21, 3, 3)
            gtm = m(body_pose=gt_rot)
            rot = ops.rot6d_to_rotmat(x6d).view(B, 21, 3, 3)
            pm = m(body_pose=rot)
        batch = {"gt_pose_body": gt_rot, "body_vertices": gtm.vertices, "body_joints": gtm.joints}
        out = {"pred_pose_body_6d": x6d, "pred_pose_body_rotmat": rot, "pred_body_vertices": pm.vertices, "pred_body_joints": pm.joints}
        commit = torch.tensor(0.1, device=dev)

        def vg_eager():
            return loss.value_and_grad(batch, out, commit)

        vg_eager()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            vg_eager()
        xg = x6d.clone().requires_grad_(True)
        eye = torch.eye(3, device=dev)

        def torch_chain():
            r = torch_rot6d(xg)
            full = torch.cat([eye.expand(B, 1, 3, 3), r, eye.expand(B, 30, 3, 3)], dim=1)
            v, j = torch_smplh(full, s)
            total = (w[0] * torch.nn.functional.mse_loss(r, gt_rot) + w[1] * torch.nn.functional.l1_loss(v, gtm.vertices) +
                     w[2] * torch.nn.functional.mse_loss(j[:, 1:22], gtm.joints[:, 1:22]) + w[3] * commit) * w[4]
            return total, torch.autograd.grad(total, xg)[0]

        # two groups, each interleaved on its own: the windows that follow torch_chain's (hundreds of MB of traffic) run 3 % slower, which
        # must not land on one build of a pair
        feature = {"fwd_folded": lambda: fwd(lib, m.h, R22, 1), "fwdbwd_folded": lambda: fwdbwd(R22, g22, 1),
                   "fwd_full": lambda: fwd(lib, m.h, R52, 0), "fwdbwd_full": lambda: fwdbwd(R52, g52, 0),
                   "vg_eager": vg_eager, "vg_graph": graph.replay, "torch_chain": torch_chain}
        pairs = {}
        if parent:
            pairs = {"smpl_fwdbwd": lambda: smpl_fwdbwd(lib, own[1]), "parent_smpl_fwdbwd": lambda: smpl_fwdbwd(parent[0], parent[2]),
                     "pair_fwd_folded": lambda: fwd(lib, own[0], R22, 1), "parent_fwd_folded": lambda: fwd(parent[0], parent[1], R22, 1),
                     "pair_fwd_full": lambda: fwd(lib, own[0], R52, 0), "parent_fwd_full": lambda: fwd(parent[0], parent[1], R52, 0)}
        # the two chains compute the same thing (a check, not a tolerance test: tests/test_gpu_tokenizer_loss.py holds the bound)
        (ld, gd), (tt, tg) = vg_eager(), torch_chain()
        agree = float((gd - tg).abs().max() / tg.abs().max())
        ms = {}
        for arms in (pairs, feature):
            ms.update({k: [] for k in arms})
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
        rec = {"what": "SMPL-H forward / forward + backward and the tokenizer's value_and_grad, ms per call between device events, arms interleaved",
               "build": build, "parent_build": parent_build, "poses": B, "reps": a.reps, "iters_per_window": a.iters,
               "gpu": torch.cuda.get_device_name(0), "value_and_grad_launches": loss.LAUNCHES,
               "ms_median": {k: round(v, 4) for k, v in med.items()},
               "ms_spread": {k: round((max(v) - min(v)) / 2, 4) for k, v in ms.items()},
               "ms_windows": {k: [round(x, 4) for x in v] for k, v in ms.items()},
               "backward_only_ms_folded": round(med["fwdbwd_folded"] - med["fwd_folded"], 4),
               "backward_only_ms_full": round(med["fwdbwd_full"] - med["fwd_full"], 4),
               "device_chain_ms_fwd_folded_plus_vg_eager": round(med["fwd_folded"] + med["vg_eager"], 4),
               "device_chain_ms_fwd_folded_plus_vg_graph": round(med["fwd_folded"] + med["vg_graph"], 4),
               "torch_over_device_chain_eager": round(med["torch_chain"] / (med["fwd_folded"] + med["vg_eager"]), 2),
               "torch_over_device_chain_graph": round(med["torch_chain"] / (med["fwd_folded"] + med["vg_graph"]), 2),
               "chains_max_rel_diff": agree}
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps({k: v for k, v in rec.items() if k != "ms_windows"}), flush=True)
        del graph
    m.close()


if __name__ == "__main__":
    main()
