"""thmr_val_loss / thmr_op_token_ce on the device (csrc/loss.hip, tokenhmr_amd/losses.py) against the reference's own record
(tests/golden/val_loss.npz: TokenHMR.compute_loss executed in place, float32 and float64) and the fp64 oracle tests/val_loss_oracle.py.

Bounds.
  losses      max(1e-5 relative, 2 x |reference fp32 - reference fp64|) against the float64 value.  The 1e-5 floor is the bound
              thmr_op_mean_row_dist carries; the reference distance comes from the fixture.  Away from the fixture (shapes, edges) the
              floor alone: a term is a sum of at most 64 fp32 terms per item added in fp64 across items.
  angle_err   max(1e-6 rad, 2 x d_ref), kp2d_err max(1e-7, 2 x d_ref).  d_ref is the reference's fp32-to-fp64 distance on the fixture's
              inputs (recorded in the fixture); for the edge cases, whose angles reach pi, it is the distance of the SAME formula run in
              numpy float32 from its float64 run on the same inputs, computed in the test.
  masks       compared on every entry of the fixture (its generator guarantees the margin); elsewhere wherever the fp64 value is farther
              from its threshold than the fixture's margin (4 x d_ref) — at least 98 % of the entries, or the test fails — and 0 may differ.
Every test prints the distances it measures before it asserts; DESIGN.md 8 N7 records them.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

import val_loss_oracle as VO
from tokenhmr_amd import _cabi, ops
from tokenhmr_amd.losses import LOSS_KEYS, ValidationLoss, token_loss
from tokenhmr_amd.model import ConfigNode

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_golden_val_loss as GV          # noqa: E402

pytestmark = pytest.mark.gpu
REL_FLOOR, ANGLE_FLOOR, KP2D_FLOOR = 1e-5, 1e-6, 1e-7
MASKS = ("valid2d", "weak2d", "valid_rot", "weak_rot", "conf2d_used", "conf3d_used")
WEIGHTS = [GV.LOSS_WEIGHTS[k] for k in ("KEYPOINTS_2D", "KEYPOINTS_3D", "GLOBAL_ORIENT", "BODY_POSE", "BETAS")]
IN_KEYS = ("pred_keypoints_2d", "pred_keypoints_3d", "pred_rotmat", "pred_betas", "gt_keypoints_2d", "gt_keypoints_3d", "gt_pose_aa",
           "gt_betas", "has_global_orient", "has_body_pose", "has_betas")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN_DIR, "val_loss.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def thresholds(golden):
    return {k[7:]: v for k, v in golden.items() if k.startswith("thresh.")}


def _valid_3d(inp):
    return np.array([n in ("H36M-TRAIN-WMASK", "BEDLAM") for n in inp["dataset"]], dtype=np.float32)


def _device_call(inp, dev, thresholds, loose, gt="aa", **kw):
    """ops.val_loss on make_inputs-style arrays; gt 'aa' hands the axis-angle pose, 'mat' inp['gt_pose_rotmat']."""
    t = {k: torch.from_numpy(np.ascontiguousarray(inp[k], dtype=np.float32)).to(dev) for k in IN_KEYS if k != "gt_pose_aa"}
    pose = torch.from_numpy(np.ascontiguousarray(inp["gt_pose_aa" if gt == "aa" else "gt_pose_rotmat"], dtype=np.float32)).to(dev)
    extra = {}
    if loose:
        extra = dict(valid_3d=torch.from_numpy(_valid_3d(inp)).to(dev), kp2d_thresh=torch.from_numpy(thresholds["kp2d"]).to(dev),
                     angle_thresh=torch.from_numpy(np.concatenate([thresholds["global_orient"], thresholds["body_pose"]])).to(dev))
    return ops.val_loss(t["pred_keypoints_2d"], t["pred_keypoints_3d"], t["pred_rotmat"], t["pred_betas"], t["gt_keypoints_2d"],
                        t["gt_keypoints_3d"], pose, t["gt_betas"], t["has_global_orient"], t["has_body_pose"], t["has_betas"], WEIGHTS,
                        loose=loose, loose_weight=GV.LOOSE_WEIGHT, **extra, **kw)


def _np(res):
    return {k: v.cpu().double().numpy() for k, v in res.items()}


def _check_against_oracle(name, dev_res, inp, thresholds, golden, loose, gt_is_axis_angle=True, d_angle=None):
    """Losses at the relative floor; errors at max(floor, 2 x d_ref); masks wherever the fp64 value clears the fixture's margin."""
    want = VO.val_loss64(inp, WEIGHTS, loose=loose, loose_weight=GV.LOOSE_WEIGHT, thresholds=thresholds, valid_3d=_valid_3d(inp),
                         gt_is_axis_angle=gt_is_axis_angle)
    got = _np(dev_res)
    d = np.abs(got["losses"] - want["losses"])
    print(f"{name} [{'loose' if loose else 'plain'}]: losses relative to fp64 " + " ".join(f"{x / max(abs(w), 1e-300):.1e}" for x, w in zip(d, want["losses"])))
    assert (d <= REL_FLOOR * np.abs(want["losses"])).all(), (got["losses"], want["losses"])
    dp = np.abs(got["per_item"] - want["per_item"])
    assert (dp <= REL_FLOOR * np.abs(want["per_item"])).all()
    if not loose:
        return want, got
    tol_a = max(ANGLE_FLOOR, 2 * (float(golden["margin.angle_err.d_ref"]) if d_angle is None else d_angle))
    tol_k = max(KP2D_FLOOR, 2 * float(golden["margin.kp2d_err.d_ref"]))
    da, dk = np.abs(got["angle_err"] - want["angle_err"]).max(), np.abs(got["kp2d_err"] - want["kp2d_err"]).max()
    print(f"{name}: angle_err {da:.2e} rad (bound {tol_a:.2e}), kp2d_err {dk:.2e} (bound {tol_k:.2e})")
    assert da <= tol_a and dk <= tol_k
    # the margin is the fixture's (4 x d_ref), narrower than the 1e-6 rad floor angle_err is granted: a mask that differs inside that gap
    # fails this test, which then asks more of the kernel than the angle bound does (measured device error on these shapes: 1.1e-7 to 2.5e-7 rad)
    thr_a = np.concatenate([thresholds["global_orient"], thresholds["body_pose"]]).astype(np.float64)
    clear_a = np.abs(want["angle_err"] - thr_a[None]) > 4 * float(golden["margin.angle_err.d_ref"])
    clear_k = np.abs(want["kp2d_err"] - thresholds["kp2d"].astype(np.float64)[None]) > 4 * float(golden["margin.kp2d_err.d_ref"])
    frac = (clear_a.sum() + clear_k.sum()) / (clear_a.size + clear_k.size)
    assert frac >= 0.98, f"only {100 * frac:.1f} % of the mask entries clear the margin"
    # conf3d_used depends on the 2D decision of the same keypoint, the rest on its own row
    for k in MASKS:
        clear = clear_a if "rot" in k else clear_k
        bad = int((got[k][clear] != want[k][clear]).sum())
        assert bad == 0, f"{name}: {bad} entries of {k} differ from the oracle"
    assert np.array_equal(got["has_betas_used"], want["has_betas_used"])
    return want, got


# ------------------------------------------------------------------------------------------------ the reference's record
@pytest.mark.parametrize("mode", ["plain", "loose"])
def test_fixture_against_the_reference_record(built_lib, cuda_dev, golden, thresholds, mode):
    """Through the public path: ValidationLoss on the reference's batch / output dicts."""
    inp = {k[3:]: v for k, v in golden.items() if k.startswith("in.")}
    inp["dataset"] = [str(s) for s in inp["dataset"]]
    batch, output = GV.to_batch(inp, torch.float32)
    mv = lambda d: {k: (mv(v) if isinstance(v, dict) else v.to(cuda_dev) if torch.is_tensor(v) else v) for k, v in d.items()}      # noqa: E731
    batch, output = mv(batch), mv(output)
    before = {"kp2": batch["keypoints_2d"].clone(), "kp3": batch["keypoints_3d"].clone(), "hb": batch["has_smpl_params"]["betas"].clone()}
    cfg = ConfigNode({"MODEL": {"LOOSE_SUP": mode == "loose", "LOOSE_WEIGHT": GV.LOOSE_WEIGHT}, "LOSS_WEIGHTS": dict(GV.LOSS_WEIGHTS)})
    vl = ValidationLoss(cfg, thresholds=thresholds)
    loss = vl(batch, output, train=True)
    assert loss.dim() == 0 and loss.is_cuda and list(output["losses"]) == list(LOSS_KEYS) and loss.data_ptr() == output["losses"]["loss"].data_ptr()
    got = np.array([float(output["losses"][k]) for k in LOSS_KEYS])
    r32, r64 = golden[f"{mode}.f32.losses"], golden[f"{mode}.f64.losses"]
    tol = np.maximum(REL_FLOOR * np.abs(r64), 2 * np.abs(r32 - r64))
    for k, g_, a, b, t in zip(LOSS_KEYS, got, r32, r64, tol):
        print(f"{mode} {k}: device {g_:.8f}  reference fp64 {b:.10f}  |device - fp64| {abs(g_ - b):.2e}  |reference fp32 - fp64| {abs(a - b):.2e}  bound {t:.2e}")
    assert (np.abs(got - r64) <= tol).all()
    # nothing was written into the batch (the one deliberate departure)
    assert torch.equal(batch["keypoints_2d"], before["kp2"]) and torch.equal(batch["keypoints_3d"], before["kp3"])
    assert torch.equal(batch["has_smpl_params"]["betas"], before["hb"])
    assert torch.allclose(output["loss_per_item"].double().sum(0), torch.from_numpy(r64[1:]).to(cuda_dev), rtol=1e-5, atol=0)
    if mode == "plain":
        assert "loss_masks" not in output
        return
    m = _np(output["loss_masks"])
    for k in MASKS + ("has_betas_used",):
        ref = golden[f"loose.f32.{k}"].astype(np.float64)
        assert m[k].shape == ref.shape and np.array_equal(m[k], ref), f"{k}: {(m[k] != ref).sum()} entries differ from the reference"
    tol_a = max(ANGLE_FLOOR, 2 * float(golden["margin.angle_err.d_ref"]))
    tol_k = max(KP2D_FLOOR, 2 * float(golden["margin.kp2d_err.d_ref"]))
    da = np.abs(m["angle_err"] - golden["loose.f64.angle_err"]).max()
    dk = np.abs(m["kp2d_err"] - golden["loose.f64.kp2d_err"]).max()
    print(f"angle_err: device vs reference fp64 {da:.2e} rad (reference fp32 {float(golden['margin.angle_err.d_ref']):.2e}, bound {tol_a:.2e}); "
          f"kp2d_err {dk:.2e} (reference fp32 {float(golden['margin.kp2d_err.d_ref']):.2e}, bound {tol_k:.2e})")
    assert da <= tol_a and dk <= tol_k


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("B", [1, 3, 5, 64, 257])
def test_shapes_against_the_fp64_oracle(built_lib, cuda_dev, golden, thresholds, B):
    """1: a single item; 3: a partial workgroup; 5: across the four-items-per-workgroup boundary; 64: the evaluation batch; 257: thread 0
    of the reduce stage adds two items."""
    inp = GV.make_inputs(B, 1000 + B)
    for loose in (False, True):
        _check_against_oracle(f"B = {B}", _device_call(inp, cuda_dev, thresholds, loose), inp, thresholds, golden, loose)


# ------------------------------------------------------------------------------------------------ edges
def _edge(name, golden):
    B = 5
    inp = GV.make_inputs(B, 77)
    kw = {}
    if name == "all confidences zero":
        inp["gt_keypoints_2d"][:, :, 2] = 0
        inp["gt_keypoints_3d"][:, :, 3] = 0
    elif name == "all has zero":
        for k in ("has_global_orient", "has_body_pose", "has_betas"):
            inp[k][:] = 0
    elif name == "prediction equals ground truth":
        inp["gt_pose_rotmat"] = inp["pred_rotmat"].copy()
        inp["gt_betas"] = inp["pred_betas"].copy()
        kw["gt"] = "mat"
    elif name == "relative rotation pi - 1e-3":
        Rg = VO.aa_to_rotmat64(inp["gt_pose_aa"].reshape(-1, 3))
        ax = np.random.default_rng(5).standard_normal((B * 24, 3))
        ax /= np.linalg.norm(ax, axis=1, keepdims=True)
        inp["pred_rotmat"] = (GV._rodrigues64(ax * (np.pi - 1e-3)) @ Rg).reshape(B, 24, 3, 3).astype(np.float32)
    elif name == "zero axis-angle ground truth":
        inp["gt_pose_aa"][:] = 0
    elif name == "pelvis confidence zero":
        inp["gt_keypoints_2d"][:, 39, 2] = 0
        inp["gt_keypoints_3d"][:, 39, 3] = 0
    else:
        raise KeyError(name)
    return inp, kw


EDGES = ["all confidences zero", "all has zero", "prediction equals ground truth", "relative rotation pi - 1e-3", "zero axis-angle ground truth",
         "pelvis confidence zero"]


@pytest.mark.parametrize("name", EDGES)
def test_edges_against_the_fp64_oracle(built_lib, cuda_dev, golden, thresholds, name):
    inp, kw = _edge(name, golden)
    is_aa = kw.get("gt", "aa") == "aa"
    # the formula's own float32 rounding on THESE inputs (numpy float32 vs float64), for the angle bound
    Rg64 = VO.aa_to_rotmat64(inp["gt_pose_aa"].reshape(-1, 3)).reshape(-1, 24, 3, 3) if is_aa else inp["gt_pose_rotmat"]
    Rg32 = VO.aa_to_rotmat64(inp["gt_pose_aa"].reshape(-1, 3), np.float32).reshape(-1, 24, 3, 3) if is_aa else inp["gt_pose_rotmat"]
    d_angle = np.abs(VO.joint_angle_error64(inp["pred_rotmat"], Rg32, np.float32) - VO.joint_angle_error64(inp["pred_rotmat"], Rg64)).max()
    for loose in (False, True):
        res = _device_call(inp, cuda_dev, thresholds, loose, **kw)
        want, got = _check_against_oracle(name, res, inp, thresholds, golden, loose, gt_is_axis_angle=is_aa, d_angle=d_angle)
        if name == "all confidences zero":
            assert got["losses"][1] == 0.0 and got["losses"][2] == 0.0 and (got["per_item"][:, :2] == 0.0).all()
        if name == "all has zero" and not loose:
            assert (got["losses"][3:] == 0.0).all()
        if name == "prediction equals ground truth":
            assert (got["losses"][3:] == 0.0).all()
            if loose:          # R R^T is symmetric in every precision: a zero vector part, the small-angle branch, angle 0
                assert got["angle_err"].max() <= ANGLE_FLOOR and got["valid_rot"].sum() == (np.repeat(_valid_3d(inp)[:, None], 24, 1)).sum()
        if name == "relative rotation pi - 1e-3" and loose:
            # matrix_to_quaternion takes the x, y or z candidate here and does not standardise the sign of w, so the reference's
            # angle 2 atan2(|xyz|, w) is pi - 1e-3 where w > 0 and 2 pi - (pi - 1e-3) = pi + 1e-3 where w < 0: both sides of pi
            off = want["angle_err"] - np.pi
            assert abs(abs(off) - 1e-3).max() < 1e-5 and (off < 0).any() and (off > 0).any()
        if name == "zero axis-angle ground truth":
            # aa_to_rotmat(0): angle = |1e-8 (1,1,1)|, axis 0 / angle = 0 -> the identity, exactly
            eye = torch.zeros(24 * 5, 3, device=cuda_dev)
            R = torch.empty(24 * 5, 3, 3, device=cuda_dev)
            _cabi.check(built_lib.thmr_op_aa_to_rotmat(_p(eye), _p(R), 120, None), lib=built_lib)
            assert torch.equal(R, torch.eye(3, device=cuda_dev).expand(120, 3, 3))


def test_matrix_and_axis_angle_ground_truth_agree(built_lib, cuda_dev, golden, thresholds):
    """The same ground truth as (B,72) axis-angle and as the (B,24,3,3) matrices thmr_op_aa_to_rotmat makes of it."""
    B = 7
    inp = GV.make_inputs(B, 31)
    aa = torch.from_numpy(inp["gt_pose_aa"]).to(cuda_dev).reshape(-1, 3).contiguous()
    R = torch.empty(B * 24, 3, 3, device=cuda_dev)
    _cabi.check(built_lib.thmr_op_aa_to_rotmat(_p(aa), _p(R), B * 24, None), lib=built_lib)
    inp["gt_pose_rotmat"] = R.view(B, 24, 3, 3).cpu().numpy()
    for loose in (False, True):
        a, b = _np(_device_call(inp, cuda_dev, thresholds, loose)), _np(_device_call(inp, cuda_dev, thresholds, loose, gt="mat"))
        rel = np.abs(a["losses"] - b["losses"]) / np.abs(a["losses"])
        print(f"axis-angle vs matrix ground truth [{'loose' if loose else 'plain'}]: relative difference " + " ".join(f"{x:.1e}" for x in rel),
              "(bit-equal)" if np.array_equal(a["losses"], b["losses"]) else "")
        assert (rel <= REL_FLOOR).all()
        # the twins held together: rotation_device.h's aa_to_rotmat_dev restates thmr_op_aa_to_rotmat's kernel (head.hip) operation for
        # operation, so both calls hand the same matrices to the same deterministic sums; a copy that drifts shows here
        assert np.array_equal(a["per_item"][:, 2:4], b["per_item"][:, 2:4]), "aa_to_rotmat_dev and aa_to_rotmat_kernel no longer agree bit for bit"
        if loose:
            assert np.abs(a["angle_err"] - b["angle_err"]).max() <= ANGLE_FLOOR
            for k in ("valid_rot", "weak_rot", "valid2d", "conf3d_used"):
                assert np.array_equal(a[k], b[k])


def test_matrix_and_axis_angle_ground_truth_agree_on_the_edge_sets(built_lib, cuda_dev, thresholds):
    """The same twins on the rows where the formula is singular: 24 joints x 5 items take ten rows of each axis-angle group of
    tests/rotation_cases.py (zero, |aa| = 1e-9 ... 1e-2, near pi, 2 pi and 4 pi, single-axis), the NaN row excluded."""
    import rotation_cases as RC
    B = 5
    x, spans = RC.aa_set()
    rows = torch.cat([x[lo + 3:lo + 13] for lo, hi in spans.values()])
    assert rows.shape == (B * 24, 3) and torch.isfinite(rows).all()
    inp = GV.make_inputs(B, 33)
    inp["gt_pose_aa"] = rows.reshape(B, 72).numpy().copy()
    for k in ("has_global_orient", "has_body_pose"):           # every row counts
        inp[k] = np.ones(B, dtype=np.float32)
    aa = rows.to(cuda_dev).contiguous()
    R = torch.empty(B * 24, 3, 3, device=cuda_dev)
    _cabi.check(built_lib.thmr_op_aa_to_rotmat(_p(aa), _p(R), B * 24, None), lib=built_lib)
    inp["gt_pose_rotmat"] = R.view(B, 24, 3, 3).cpu().numpy()
    for loose in (False, True):
        a, b = _np(_device_call(inp, cuda_dev, thresholds, loose)), _np(_device_call(inp, cuda_dev, thresholds, loose, gt="mat"))
        assert np.isfinite(a["per_item"]).all() and (a["per_item"][:, 2:4] > 0).all()
        assert np.array_equal(a["per_item"][:, 2:4], b["per_item"][:, 2:4]), "aa_to_rotmat_dev and aa_to_rotmat_kernel no longer agree bit for bit"
        assert np.array_equal(a["losses"], b["losses"])
        if loose:
            d = np.abs(a["angle_err"] - b["angle_err"]).max()
            print(f"edge sets: angle_err between the two ground truths differs by {d:.2e} rad")
            assert d <= ANGLE_FLOOR
            for k in ("valid_rot", "weak_rot", "valid2d", "conf3d_used"):
                assert np.array_equal(a[k], b[k])


# ------------------------------------------------------------------------------------------------ determinism, graph replay
def test_two_runs_and_a_graph_replay_are_bit_equal(built_lib, cuda_dev, golden, thresholds):
    lib = built_lib
    B = 8
    inp = {k[3:]: v for k, v in golden.items() if k.startswith("in.")}
    inp["dataset"] = [str(s) for s in inp["dataset"]]
    a, b = _device_call(inp, cuda_dev, thresholds, True), _device_call(inp, cuda_dev, thresholds, True)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # the C ABI with every buffer preallocated, captured on one stream
    t = {k: torch.from_numpy(inp[k]).to(cuda_dev) for k in IN_KEYS}
    t["valid_3d"] = torch.from_numpy(_valid_3d(inp)).to(cuda_dev)
    t["kp2d_thresh"] = torch.from_numpy(thresholds["kp2d"]).to(cuda_dev)
    t["angle_thresh"] = torch.from_numpy(np.concatenate([thresholds["global_orient"], thresholds["body_pose"]])).to(cuda_dev)
    order = [k if k != "gt_pose" else "gt_pose_aa" for k in _cabi.VAL_LOSS_IN_FIELDS]
    cin = _cabi.ValLossIn(*[t[k].data_ptr() for k in order])
    outs = {k: torch.zeros_like(a[k]) for k in a}
    running = torch.zeros(7, device=cuda_dev, dtype=torch.float64)
    cout = _cabi.ValLossOut(**{k: outs[k].data_ptr() for k in outs}, running=running.data_ptr())
    desc = _cabi.ValLossDesc(*WEIGHTS, GV.LOOSE_WEIGHT, 39, _cabi.VAL_LOSS_LOOSE, 0, 0)
    ws = torch.zeros(_cabi.VAL_LOSS_WS_PER_ITEM * B, device=cuda_dev)

    def run(stream):
        _cabi.check(lib.thmr_val_loss(C.byref(desc), C.byref(cin), B, C.byref(cout), _p(ws), C.c_void_p(stream.cuda_stream)), lib=lib)

    run(torch.cuda.current_stream(cuda_dev))
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(outs[k], a[k]), k
    assert running[6].item() == 1.0 and torch.equal(running[:6], a["losses"].double())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(torch.cuda.current_stream(cuda_dev))
    for i in range(2):
        for v in outs.values():
            v.fill_(-3.0)
        ws.fill_(123.0)
        graph.replay()
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(outs[k], a[k]), k
        assert running[6].item() == 2.0 + i                       # one batch per replay
        assert torch.equal(running[:6], sum([a["losses"].double()] * (2 + i)))


# ------------------------------------------------------------------------------------------------ token_ce
@pytest.fixture(scope="module")
def token_cases(golden):
    """rows -> (softmax float32, logits x 30 float32, target int64, the fp64 row losses of the two matrices); computed once."""
    out = {}
    for rows in (160, 480, 64 * 160):
        if rows == 480:
            probs, tgt = GV.token_inputs(int(golden["token.seed"]), rows)
            logits = probs.log()
        else:
            g = torch.Generator().manual_seed(rows)
            logits = 3.0 * torch.randn(rows, 2048, generator=g)
            probs, tgt = logits.softmax(-1), torch.randint(0, 2048, (rows,), generator=g)
        raw = 30.0 * logits
        ce = lambda x: torch.logsumexp(x.double(), 1) - x.double().gather(1, tgt[:, None])[:, 0]      # noqa: E731
        out[rows] = (probs, raw, tgt, ce(probs), ce(raw))
    return out


@pytest.mark.parametrize("rows", [160, 480, 64 * 160])
def test_token_ce_against_fp64(built_lib, cuda_dev, golden, token_cases, rows):
    probs, raw, tgt, rows_p, rows_r = token_cases[rows]
    ce_p = float(rows_p.mean())
    t32 = tgt.to(torch.int32).to(cuda_dev)
    for name, x, row64 in (("softmax", probs, rows_p), ("logits x 30", raw, rows_r)):
        want = float(row64.mean())
        xd = x.to(cuda_dev)
        ws = torch.empty(rows, device=cuda_dev)
        r1, r2 = ops.token_ce(xd, t32, workspace=ws), ops.token_ce(xd, t32)
        rel = abs(float(r1) - want) / abs(want)
        print(f"token_ce [{rows} rows, {name}]: device {float(r1):.8f}, fp64 {want:.10f}, relative error {rel:.1e}")
        assert r1.dim() == 0 and r1.is_cuda and rel <= REL_FLOOR and torch.equal(r1, r2)
        assert (ws.cpu().double() - row64).abs().max() <= REL_FLOOR * row64.abs().max()
    if rows == 480:
        assert abs(ce_p - float(golden["token.f64"])) <= 1e-12 * abs(ce_p)
        got = float(token_loss(probs.view(3, 160, 2048).to(cuda_dev), tgt.view(3, 160).to(cuda_dev)))
        rec = float(golden["token.f32"])
        print(f"TokenLoss fixture: device {got:.8f}, the reference's float32 {rec:.8f}, float64 {ce_p:.10f}")
        assert abs(got - ce_p) <= REL_FLOOR * ce_p and abs(rec - ce_p) <= REL_FLOOR * ce_p


def test_token_ce_out_of_range_target_is_nan_and_touches_nothing_else(built_lib, cuda_dev, token_cases):
    probs, _, tgt, _, _ = token_cases[160]
    rows = 160
    pad = torch.full(((rows + 2) * 2048,), float("nan"), device=cuda_dev)          # a NaN row in front of and behind the matrix
    x = pad[2048:-2048].view(rows, 2048)
    x.copy_(probs)
    ws_pad = torch.full((rows + 8,), -7.0, device=cuda_dev)
    ws = ws_pad[4:-4]
    good = tgt.to(torch.int32).to(cuda_dev)
    clean = ops.token_ce(x, good, workspace=ws)
    clean_rows = ws.clone()
    assert torch.isfinite(clean) and torch.isfinite(clean_rows).all() and (ws_pad[:4] == -7.0).all() and (ws_pad[-4:] == -7.0).all()
    bad = good.clone()
    bad_rows = {0: -1, 17: 2048, 100: 2 ** 31 - 1, 159: 2048}
    for r, v in bad_rows.items():
        bad[r] = v
    ws.fill_(5.0)
    res = ops.token_ce(x, bad, workspace=ws)
    assert torch.isnan(res)
    keep = torch.ones(rows, dtype=torch.bool, device=cuda_dev)
    keep[list(bad_rows)] = False
    assert torch.isnan(ws[~keep]).all() and torch.equal(ws[keep], clean_rows[keep])
    assert (ws_pad[:4] == -7.0).all() and (ws_pad[-4:] == -7.0).all()
    assert torch.isnan(pad[:2048]).all() and torch.isnan(pad[-2048:]).all() and torch.equal(x, probs.to(cuda_dev))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_of_both_entry_points(built_lib, cuda_dev, golden, thresholds):
    lib = built_lib
    B = 8
    inp = {k[3:]: v for k, v in golden.items() if k.startswith("in.")}
    t = {k: torch.from_numpy(inp[k]).to(cuda_dev) for k in IN_KEYS}
    t["valid_3d"] = torch.from_numpy(inp["valid_3d"]).to(cuda_dev)
    t["kp2d_thresh"] = torch.from_numpy(thresholds["kp2d"]).to(cuda_dev)
    t["angle_thresh"] = torch.from_numpy(np.concatenate([thresholds["global_orient"], thresholds["body_pose"]])).to(cuda_dev)
    order = [k if k != "gt_pose" else "gt_pose_aa" for k in _cabi.VAL_LOSS_IN_FIELDS]
    losses = torch.full((6,), -3.0, device=cuda_dev)
    ws = torch.full((5 * B,), -3.0, device=cuda_dev)

    running = torch.full((8,), -3.0, device=cuda_dev, dtype=torch.float64)

    def call(desc_kw=None, in_kw=None, B_=B, ws_=ws, desc_null=False, in_null=False, out_null=False, running_=None):
        d = dict(pelvis_id=39, mode=_cabi.VAL_LOSS_LOOSE, gt_pose_is_rotmat=0)
        d.update(desc_kw or {})
        desc = _cabi.ValLossDesc(*WEIGHTS, GV.LOOSE_WEIGHT, d["pelvis_id"], d["mode"], d["gt_pose_is_rotmat"], 0)
        ptrs = {f: t[k].data_ptr() for f, k in zip(_cabi.VAL_LOSS_IN_FIELDS, order)}
        ptrs.update(in_kw or {})
        cin, cout = _cabi.ValLossIn(**ptrs), _cabi.ValLossOut(losses=losses.data_ptr(), running=running_)
        rc = lib.thmr_val_loss(None if desc_null else C.byref(desc), None if in_null else C.byref(cin), B_,
                               None if out_null else C.byref(cout), _p(ws_) if ws_ is not None else None, None)
        return rc, lib.thmr_last_error(None).decode()

    cases = [dict(desc_null=True), dict(in_null=True), dict(out_null=True), dict(B_=0), dict(B_=-1), dict(B_=2 ** 24 + 1), dict(B_=2 ** 31 - 1),
             dict(running_=running.data_ptr() + 4), dict(desc_kw={"mode": 2}),
             dict(desc_kw={"mode": -1}), dict(desc_kw={"pelvis_id": 44}), dict(desc_kw={"pelvis_id": -1}), dict(desc_kw={"gt_pose_is_rotmat": 2}),
             dict(ws_=None), dict(in_kw={"valid_3d": None}), dict(in_kw={"kp2d_thresh": None}), dict(in_kw={"angle_thresh": None}),
             dict(in_kw={"gt_keypoints_3d": t["gt_keypoints_3d"].data_ptr() + 4}), dict(in_kw={"pred_keypoints_2d": t["pred_keypoints_2d"].data_ptr() + 4})]
    cases += [dict(in_kw={f: None}) for f in _cabi.VAL_LOSS_IN_FIELDS[:11]]
    for kw in cases:
        rc, msg = call(**kw)
        assert rc == -1 and "val_loss" in msg, (kw, rc, msg)
    # the plain mode needs neither thresholds nor valid_3d
    torch.cuda.synchronize()
    assert (losses == -3.0).all() and (ws == -3.0).all() and (running == -3.0).all()      # no refused call launched anything
    rc, msg = call(desc_kw={"mode": _cabi.VAL_LOSS_PLAIN}, in_kw={"valid_3d": None, "kp2d_thresh": None, "angle_thresh": None})
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert abs(float(losses[0]) - float(golden["plain.f64.losses"][0])) <= 1e-5 * float(golden["plain.f64.losses"][0])
    # token_ce
    x = torch.zeros(4, 2048, device=cuda_dev)
    tg = torch.zeros(4, dtype=torch.int32, device=cuda_dev)
    out, tws = torch.full((1,), -3.0, device=cuda_dev), torch.full((4,), -3.0, device=cuda_dev)
    for bad in ((None, _p(tg), 4, _p(out), _p(tws)), (_p(x), None, 4, _p(out), _p(tws)), (_p(x), _p(tg), 4, None, _p(tws)),
                (_p(x), _p(tg), 4, _p(out), None), (_p(x), _p(tg), 0, _p(out), _p(tws)), (_p(x), _p(tg), -5, _p(out), _p(tws)),
                (C.c_void_p(x.data_ptr() + 4), _p(tg), 3, _p(out), _p(tws))):
        assert lib.thmr_op_token_ce(*bad, None) == -1
        assert "token_ce" in lib.thmr_last_error(None).decode()
    torch.cuda.synchronize()
    assert float(out) == -3.0 and (tws == -3.0).all()
    assert lib.thmr_op_token_ce(_p(x), _p(tg), 4, _p(out), _p(tws), None) == 0
    torch.cuda.synchronize()
    assert abs(float(out) - np.log(2048.0)) <= 1e-5 * np.log(2048.0)
    with pytest.raises(ValueError):
        ops.token_ce(x, tg.long())
    with pytest.raises(ValueError, match="loose"):
        ops.val_loss(*[t[k] for k in order[:11]], WEIGHTS, loose=True)


# ------------------------------------------------------------------------------------------------ the facade
def test_validation_step_on_a_synthetic_engine(built_lib, cuda_dev):
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd.model import TokenHMR
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    cfg = HMRConfig(vit_depth=2, dec_depth=2)
    mcfg = ConfigNode({"MODEL": {"LOOSE_SUP": True, "LOOSE_WEIGHT": GV.LOOSE_WEIGHT}, "LOSS_WEIGHTS": dict(GV.LOSS_WEIGHTS)})
    model = TokenHMR.from_state(cfg, W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0), make_synthetic_smpl(cfg, 0),
                                max_batch=4, device=cuda_dev, model_cfg=mcfg)
    with pytest.raises(NotImplementedError):
        model.forward_step({}, train=True)
    bare = TokenHMR.from_engine(model.engine)                     # no model_cfg: no LOSS_WEIGHTS to read, and the error says what to pass
    assert bare.validation_loss is None and model.validation_loss is None
    with pytest.raises(KeyError, match="model_cfg"):
        bare.compute_loss({}, {})
    per_batch = []
    for i, B in enumerate((4, 2, 3)):
        inp = GV.make_inputs(B, 500 + i)
        batch, _ = GV.to_batch(inp, torch.float32)
        batch = {k: ({kk: vv.to(cuda_dev) for kk, vv in v.items()} if isinstance(v, dict) else v.to(cuda_dev) if torch.is_tensor(v) else v)
                 for k, v in batch.items()}
        batch["img"] = torch.randn(B, 3, 256, 256, generator=torch.Generator().manual_seed(i)).to(cuda_dev)
        out = model.validation_step(batch, i)
        assert list(out["losses"]) == list(LOSS_KEYS) and out["loss"].data_ptr() == out["losses"]["loss"].data_ptr() and "loss_masks" not in out
        # the same tensors through a ValidationLoss of its own: bit for bit
        mine = ValidationLoss(mcfg)
        out2 = {k: out[k] for k in ("pred_smpl_params", "pred_keypoints_2d", "pred_keypoints_3d")}
        mine(batch, out2)
        for k in LOSS_KEYS:
            assert torch.equal(out["losses"][k], out2["losses"][k]), k
        assert torch.isfinite(out["loss"]) and float(out["loss"]) > 0
        per_batch.append([float(out["losses"][k]) for k in LOSS_KEYS])
    m = model.validation_loss.get_metrics_dict()
    want = (np.array(per_batch[0]) + np.array(per_batch[1]) + np.array(per_batch[2])) / 3.0
    assert [m[k] for k in LOSS_KEYS] == want.tolist()
    model.validation_loss.reset()
    with pytest.raises(ValueError):
        model.validation_loss.get_metrics_dict()
    model.engine.status()
    model.engine.close()
