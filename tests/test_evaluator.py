"""Evaluator: oracle pinned to the reference's own Evaluator (CPU), HIP kernels vs both (GPU)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from oracle import eval_oracle as E
from oracle.gen_golden_eval import make_case

KP = [25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 43]


def test_eval_oracle_matches_reference_golden():
    g = np.load(os.path.join(GOLDEN_DIR, "eval_small.npz"))
    pred_k, pred_v, gt_k, gt_v, J24 = make_case()
    mp, re, pve = E.evaluate_batch(pred_k, pred_v, gt_k, gt_v, KP, 39)
    assert np.abs(mp.numpy() - g["mpjpe"]).max() < 1e-3 and np.abs(re.numpy() - g["re"]).max() < 1e-3
    assert np.abs(pve.numpy() - g["pve"]).max() < 1e-3
    mp, re, pve = E.evaluate_batch_emdb(pred_v, gt_v, J24, list(range(24)))
    assert np.abs(mp.numpy() - g["emdb_mpjpe"]).max() < 1e-3 and np.abs(re.numpy() - g["emdb_re"]).max() < 1e-3


def test_procrustes_is_invariant_to_similarity():
    g = torch.Generator().manual_seed(3)
    from oracle.tokenhmr_oracle import rot6d_to_rotmat
    x = torch.randn(4, 14, 3, generator=g)
    R = rot6d_to_rotmat(torch.randn(4, 6, generator=g))
    y = 0.7 * torch.einsum("bij,bkj->bki", R, x) + torch.randn(4, 1, 3, generator=g)
    _, re = E.eval_pose(y, x)
    assert re.abs().max() < 1e-2     # mm


@pytest.mark.gpu
def test_gpu_evaluator_matches_reference(built_lib, cuda_dev):
    """Tolerance 0.01 mm (north_star asks +-0.1 mm): fp64 Jacobi SVD on the GPU vs LAPACK fp32 gesdd in the reference."""
    from tokenhmr_amd.evaluator import Evaluator, eval_pose_gpu
    g = np.load(os.path.join(GOLDEN_DIR, "eval_small.npz"))
    pred_k, pred_v, gt_k, gt_v, J24 = make_case()
    d = cuda_dev
    ev = Evaluator(100, KP, 39, metrics=["mode_re", "mode_mpjpe", "mode_pve"], dataset="3DPW-TEST")
    r = ev({"pred_keypoints_3d": pred_k.to(d), "pred_vertices": pred_v.to(d)},
           {"imgname": ["x"] * 6, "keypoints_3d": gt_k.to(d), "vertices": gt_v.to(d)})
    assert np.abs(r["mode_mpjpe"] - g["mpjpe"]).max() < 1e-2
    assert np.abs(r["mode_re"] - g["re"]).max() < 1e-2            # includes the mirrored crop (det < 0 branch)
    assert np.abs(r["mode_pve"] - g["pve"]).max() < 1e-2
    assert ev.counter == 6 and abs(ev.get_metrics_dict()["mode_mpjpe"] - g["mpjpe"].mean()) < 1e-2
    ev2 = Evaluator(100, list(range(24)), 39, metrics=["mode_re", "mode_mpjpe", "mode_pve"], J_regressor_24_SMPL=J24.to(d), dataset="EMDB")
    r2 = ev2({"pred_vertices": pred_v.to(d)}, {"imgname": ["x"] * 6, "vertices": gt_v.to(d)})
    assert np.abs(r2["mode_mpjpe"] - g["emdb_mpjpe"]).max() < 1e-2
    assert np.abs(r2["mode_re"] - g["emdb_re"]).max() < 1e-2
    assert np.abs(r2["mode_pve"] - g["emdb_pve"]).max() < 1e-2
    # size-independent property at B=512: a similarity-transformed copy has zero PA error and the right MPJPE
    gg = torch.Generator().manual_seed(11)
    from oracle.tokenhmr_oracle import rot6d_to_rotmat
    x = torch.cat([torch.randn(512, 44, 3, generator=gg), torch.ones(512, 44, 1)], -1)
    R = rot6d_to_rotmat(torch.randn(512, 6, generator=gg))
    y = 1.3 * torch.einsum("bij,bkj->bki", R, x[:, :, :3]) + 0.2
    mp, re, _ = eval_pose_gpu(y.to(d), x.to(d), KP, 39)
    assert re.abs().max().item() < 1e-2
    ref_mp, _, _ = E.evaluate_batch(y, torch.zeros(512, 4, 3), x, torch.zeros(512, 4, 3), KP, 39)
    assert (mp.cpu() - ref_mp).abs().max() < 1e-1 * 1e-1


def test_evaluator_fills_its_host_arrays_lazily(monkeypatch):
    """The drop-in evaluator keeps a batch's (B,) results where the kernels left them and copies them into the reference's host arrays
    only when somebody looks — so eval.py's loop (evaluator(out, batch) per batch, :149) never synchronises per batch.  Host logic only:
    the kernels are replaced by a stand-in that returns known per-sample values."""
    from tokenhmr_amd import evaluator as EV
    calls = []

    def fake_eval(pred_j, gt_j, kpl, pelvis, mode=0, pv=None, gv=None):
        B = pred_j.shape[0]
        base = float(len(calls)) * 100
        calls.append(B)
        mk = lambda off: torch.arange(B, dtype=torch.float32) + base + off      # noqa: E731
        return mk(0.0), mk(0.25), (mk(0.5) if pv is not None else None)

    monkeypatch.setattr(EV, "eval_pose_gpu", fake_eval)
    ev = EV.Evaluator(dataset_length=100, keypoint_list=[0, 1], pelvis_ind=0, metrics=["mode_re", "mode_mpjpe", "mode_pve"], max_pending=3)
    out = {"pred_keypoints_3d": torch.zeros(4, 44, 3), "pred_vertices": torch.zeros(4, 10, 3)}
    batch = {"keypoints_3d": torch.zeros(4, 44, 4), "vertices": torch.zeros(4, 10, 3), "imgname": ["a", "b", "c", "d"]}
    r0 = ev(out, batch)
    r1 = ev(out, batch)
    assert ev.counter == 8 and len(ev._pending) == 2 and ev.imgnames == ["a", "b", "c", "d"] * 2
    assert not ev._arrays["mode_mpjpe"][:8].any()                       # nothing copied yet
    assert list(r1["mode_mpjpe"]) == [100.0, 101.0, 102.0, 103.0]       # a returned batch result materialises ITS OWN values ...
    assert len(ev._pending) == 2 and list(r0["mode_re"]) == [0.25, 1.25, 2.25, 3.25]      # ... without touching the evaluator's arrays
    assert not ev._arrays["mode_mpjpe"][:8].any()
    assert set(r0.keys()) == {"mode_mpjpe", "mode_re", "mode_pve"} and r0.get("nope") is None and len(r0.get("mode_pve")) == 4
    assert type(r0.to_dict()) is dict and list(r0.to_dict()["mode_pve"]) == [0.5, 1.5, 2.5, 3.5]
    ev(out, batch)                                                      # max_pending (3) batches: flushed without being asked
    assert len(ev._pending) == 0 and ev._arrays["mode_mpjpe"][4] == 100.0
    ev(out, batch)
    ev(out, batch)
    assert len(ev._pending) == 2
    assert hasattr(ev, "mode_pve") and not hasattr(ev, "mode_nope")
    assert ev.mode_pve[16] == 400.5 and len(ev._pending) == 0            # reading a metric array is "looking": it fills the host arrays
    ev(out, batch)
    assert ev.mode_mpjpe[20] == 500.0 and len(ev._pending) == 0
    r5 = ev(out, batch)
    ev.mode_mpjpe = np.full((100,), -1.0)                                # merge_evaluator replaces the arrays: a batch result read AFTERWARDS is still its own
    assert list(r5["mode_mpjpe"]) == [600.0, 601.0, 602.0, 603.0]
    ev.mode_mpjpe = np.concatenate([np.array([b * 100.0 + i for b in range(6) for i in range(4)]), np.zeros(76)])
    ev.counter = 24
    eager = EV.Evaluator(dataset_length=10, keypoint_list=[0, 1], pelvis_ind=0, metrics=["mode_re", "mode_mpjpe"], eager_results=True)
    re = eager({"pred_keypoints_3d": torch.zeros(2, 44, 3)}, {"keypoints_3d": torch.zeros(2, 44, 4), "imgname": []})
    assert type(re) is dict and set(re) == {"mode_mpjpe", "mode_re"} and re["mode_re"].shape == (2,)
    d = ev.get_metrics_dict()
    assert abs(d["mode_mpjpe"] - np.mean([b * 100 + i for b in range(6) for i in range(4)])) < 1e-9
    ev.mode_re = np.full((100,), 7.0)                                    # merge_evaluator (dist.py) replaces arrays wholesale
    assert ev.get_metrics_dict()["mode_re"] == 7.0
    # the reference's default metric list spells 'model_pve' (pose_utils.py): that array exists and stays zero, and no PVE is computed
    ev2 = EV.Evaluator(dataset_length=10, keypoint_list=[0], pelvis_ind=0)
    ev2({"pred_keypoints_3d": torch.zeros(2, 44, 3), "pred_vertices": torch.zeros(2, 10, 3)},
        {"keypoints_3d": torch.zeros(2, 44, 4), "vertices": torch.zeros(2, 10, 3), "imgname": []})
    assert ev2.get_metrics_dict()["model_pve"] == 0.0 and "mode_pve" not in ev2._arrays


def test_eval_pose_gpu_refuses_bad_arguments_on_the_host():
    """Every shape and argument rule of eval_pose_gpu is checked before the device is, so it is testable on CPU tensors: a well-formed
    call gets as far as the device check (RuntimeError), a malformed one never does.  eval_pve_kernel indexes both vertex tensors by
    pred_vertices.shape[1]: a shorter gt_vertices used to be read past its end, where the reference raises a broadcast error."""
    from tokenhmr_amd.evaluator import eval_pose_gpu
    pj, gj, v = torch.zeros(2, 44, 3), torch.zeros(2, 44, 4), torch.zeros(2, 10, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eval_pose_gpu(pj, gj, KP, 39, 0, v, v)
    for pv, gv in ((v, torch.zeros(2, 9, 3)), (torch.zeros(2, 9, 3), v), (v, torch.zeros(1, 10, 3)), (torch.zeros(3, 10, 3), torch.zeros(3, 10, 3)),
                   (torch.zeros(2, 10, 4), torch.zeros(2, 10, 4)), (v, torch.zeros(2, 10, 4)), (torch.zeros(2, 0, 3), torch.zeros(2, 0, 3)),
                   (torch.zeros(2, 30), torch.zeros(2, 30)), (torch.zeros(20, 3), torch.zeros(20, 3))):
        with pytest.raises(ValueError, match="vertex shapes"):
            eval_pose_gpu(pj, gj, KP, 39, 0, pv, gv)
    for bad_pj, bad_gj in ((torch.zeros(2, 44, 2), gj), (pj, torch.zeros(2, 43, 4)), (pj, torch.zeros(3, 44, 4)), (pj, torch.zeros(2, 44, 5)),
                           (torch.zeros(44, 3), torch.zeros(44, 4)), (torch.zeros(0, 44, 3), torch.zeros(0, 44, 4))):
        with pytest.raises(ValueError, match="joint shapes"):
            eval_pose_gpu(bad_pj, bad_gj, KP, 39)
    big_p, big_g = torch.zeros(2, 70, 3), torch.zeros(2, 70, 4)
    with pytest.raises(ValueError, match="the kernel holds 64"):
        eval_pose_gpu(big_p, big_g, list(range(65)), 39)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # 64 is the kernel's size: accepted
        eval_pose_gpu(big_p, big_g, list(range(64)), 39)
    for mode in (2, -1, 3, 0.5, None):
        with pytest.raises(ValueError, match="pelvis_mode"):
            eval_pose_gpu(pj, gj, KP, 39, mode)
    with pytest.raises(ValueError, match="joints 1 and 2"):
        eval_pose_gpu(torch.zeros(2, 2, 3), torch.zeros(2, 2, 3), [0, 1], 0, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # three joints are enough for mode 1
        eval_pose_gpu(torch.zeros(2, 3, 3), torch.zeros(2, 3, 3), [0, 1], 0, 1)
    for kpl in ([], [44], [-1, 3]):
        with pytest.raises(IndexError):
            eval_pose_gpu(pj, gj, kpl, 39)
    with pytest.raises(IndexError, match="pelvis_ind"):
        eval_pose_gpu(pj, gj, KP, 44)
    meta = lambda *s: torch.zeros(*s, device="meta")          # noqa: E731  a second device that needs no GPU
    for args in ((pj, meta(2, 44, 4), KP, 39), (meta(2, 44, 3), gj, KP, 39), (pj, gj, KP, 39, 0, meta(2, 10, 3), v), (pj, gj, KP, 39, 0, v, meta(2, 10, 3))):
        with pytest.raises(ValueError, match="different devices"):
            eval_pose_gpu(*args)
    with pytest.raises(ValueError, match="vertex shapes"):          # shapes before devices
        eval_pose_gpu(pj, gj, KP, 39, 0, meta(2, 9, 3), v)


def test_regress_joints_gpu_refuses_bad_arguments_on_the_host():
    """regress_joints_kernel reads J as (nj, verts.shape[1]): a J with another second dimension used to be read past its end (or mis-strided),
    where torch.matmul raises.  Shapes are checked first, devices after, the GPU last."""
    from tokenhmr_amd.evaluator import regress_joints_gpu
    J, v = torch.zeros(24, 10), torch.zeros(2, 10, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        regress_joints_gpu(J, v)
    for bad in (torch.zeros(10), torch.zeros(1, 24, 10), torch.zeros(0, 10)):
        with pytest.raises(ValueError, match="J must be"):
            regress_joints_gpu(bad, v)
    for bad in (torch.zeros(24, 9), torch.zeros(24, 11), torch.zeros(24, 30)):
        with pytest.raises(ValueError, match="regresses from"):
            regress_joints_gpu(bad, v)
    for bad in (torch.zeros(10, 3), torch.zeros(2, 10, 4), torch.zeros(2, 10), torch.zeros(0, 10, 3), torch.zeros(2, 0, 3), torch.zeros(1, 2, 10, 3)):
        with pytest.raises(ValueError, match="verts must be"):
            regress_joints_gpu(J, bad)
    with pytest.raises(ValueError, match="different devices"):
        regress_joints_gpu(torch.zeros(24, 10, device="meta"), v)
    with pytest.raises(ValueError, match="different devices"):
        regress_joints_gpu(J, torch.zeros(2, 10, 3, device="meta"))
    with pytest.raises(ValueError, match="regresses from"):          # shapes before devices
        regress_joints_gpu(torch.zeros(24, 9, device="meta"), v)


@pytest.mark.parametrize("exp", [False, True])
def test_eval_entry_points_reject_bad_arguments_without_a_gpu(built_lib, exp):
    """thmr_eval_pose / thmr_regress_joints validate before any HIP call, in both libraries: with dummy pointers and no GPU every refusal
    below is a negative status and a message, never a launch.  New here: n_verts < 1 when PVE is asked for (all three vertex pointers
    given) divided by zero, and a pelvis_mode other than 0 or 1 was silently treated as 1."""
    import ctypes as C
    from tokenhmr_amd import _cabi
    L = _cabi.load(exp=exp)
    null, one = C.c_void_p(0), C.c_void_p(16)      # 16: any non-null address, validation fails before it is dereferenced

    def refused(*args, fn="thmr_eval_pose", says=None):
        rc = getattr(L, fn)(*args)
        msg = L.thmr_last_error(None)
        assert rc < 0 and msg and (says is None or says in msg), (args, rc, msg)

    #        pred gt nj stride kp nkp pelvis mode pv gv nv B mp re pve pelv stream
    for nv in (0, -1):
        refused(one, one, 44, 4, one, 14, 39, 0, one, one, nv, 2, one, one, one, one, null, says=b"n_verts")
    for mode in (2, -1, 7):
        refused(one, one, 44, 4, one, 14, 39, mode, null, null, 0, 2, one, one, null, one, null, says=b"pelvis_mode")
        refused(one, one, 44, 4, one, 14, 39, mode, one, one, 10, 2, one, one, one, one, null, says=b"pelvis_mode")
    for nkp in (0, 65):
        refused(one, one, 44, 4, one, nkp, 39, 0, null, null, 0, 2, one, one, null, one, null, says=b"n_kp")
    refused(one, one, 44, 2, one, 14, 39, 0, null, null, 0, 2, one, one, null, one, null)          # gt_stride < 3
    refused(one, one, 44, 4, one, 14, 44, 0, null, null, 0, 2, one, one, null, one, null)          # pelvis_ind == n_joints
    refused(one, one, 44, 4, one, 14, -1, 0, null, null, 0, 2, one, one, null, one, null)
    refused(one, one, 2, 4, one, 2, 0, 0, null, null, 0, 2, one, one, null, one, null)             # n_joints < 3
    refused(one, one, 44, 4, one, 14, 39, 0, null, null, 0, 0, one, one, null, one, null)          # B < 1
    for hole in (0, 1, 4, 12, 13, 15):                                                             # each required buffer null in turn
        args = [one, one, 44, 4, one, 14, 39, 0, null, null, 0, 2, one, one, null, one, null]
        args[hole] = null
        refused(*args, says=b"null")
    #        J verts nj nv B out stream
    for args in ((null, one, 24, 10, 2, one, null), (one, null, 24, 10, 2, one, null), (one, one, 24, 10, 2, null, null),
                 (one, one, 0, 10, 2, one, null), (one, one, 24, 0, 2, one, null), (one, one, 24, 10, 0, one, null)):
        refused(*args, fn="thmr_regress_joints")
