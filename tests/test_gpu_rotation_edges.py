"""The rotation kernels where their formulas are singular: zero, |aa| down to 1e-9, near pi / 2 pi / 4 pi, single-axis rows, 6D vectors
scaled by 1e+-10, near-collinear, zero and under F.normalize's eps (tests/rotation_cases.py holds the sets, the rule and the reasons).

The rule is tests/stage_bounds.py's, applied PER GROUP of 64 rows: the device may be MULT = 2 times as far from float64 as the oracle in
fp32 is on the same rows, with a floor of 4 ulp of that group's largest element.  Every check prints its ratio; DESIGN.md 5.1 records the
measured table.  tests/test_rotation_cases_host.py asserts on the CPU what this file rests on: finite and meaningful references for these
seeds, the property-only groups, the agreement of the two float64 truths of the axis-angle backward."""
import ctypes as C

import numpy as np
import pytest
import torch

import lbs_backward_numpy as L
import rotation_cases as RC
import stage_bounds as SB
import tokenizer_rt_oracle as TO
from oracle import tokenhmr_oracle as O

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -24


@pytest.fixture(scope="module")
def aa():
    x, spans = RC.aa_set()
    gR = RC.grad_out(x.shape[0])
    t = {"x": x, "spans": spans, "gR": gR}
    t["fwd32"], t["fwd64"] = RC.fwd(O.aa_to_rotmat, x, torch.float32), RC.fwd(O.aa_to_rotmat, x, torch.float64)
    t["bwd64"] = RC.vjp(O.aa_to_rotmat, x, gR, torch.float64)          # the truth: float64 autograd of the forward the operator computes
    t["quat32"], t["rod32"] = RC.vjp(O.aa_to_rotmat, x, gR, torch.float32), RC.vjp(O.batch_rodrigues, x, gR, torch.float32)
    return t


@pytest.fixture(scope="module")
def r6():
    x, spans = RC.rot6d_set()
    gR = RC.grad_out(x.shape[0], RC.SEED_GRAD + 1)
    t = {"x": x, "spans": spans, "gR": gR}
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        t[f"fwd{tag}"], t[f"bwd{tag}"] = RC.fwd(O.rot6d_to_rotmat, x, dt), RC.vjp(O.rot6d_to_rotmat, x, gR, dt)
    return t


def _table(title, table):
    print(f"\n{title}\n  group            device        reference's own   ratio   bound")
    for g, d, own, r, b in table:
        print(f"  {g:<16} {d:.3e}     {own:.3e}         {r:5.2f}   {b:.3e}")


# ------------------------------------------------------------------------------------------------ thmr_op_aa_to_rotmat
def test_aa_to_rotmat_per_group(built_lib, cuda_dev, aa):
    from tokenhmr_amd import ops
    x, spans = aa["x"], aa["spans"]
    R = ops.aa_to_rotmat(x.to(cuda_dev)).cpu()
    table = []
    fails = RC.check_groups("aa_to_rotmat", R, aa["fwd32"], aa["fwd64"], spans, table=table)
    _table("thmr_op_aa_to_rotmat", table)
    lo, hi = spans["zero"]
    assert torch.equal(R[lo:hi], torch.eye(3).expand(RC.GROUP, 3, 3)), "aa = 0 is not the identity exactly"
    assert torch.allclose(R @ R.transpose(-1, -2), torch.eye(3).expand_as(R), atol=1e-5, rtol=0)
    assert torch.allclose(torch.linalg.det(R), torch.ones(R.shape[0]), atol=1e-5, rtol=0)
    for g, (lo, hi) in spans.items():                    # one edge row of each group alone, n = 1: the bits of the batched call
        i = lo + 17
        assert torch.equal(ops.aa_to_rotmat(x[i:i + 1].to(cuda_dev)).cpu()[0], R[i]), g
    assert not fails, "\n".join(fails)


def test_aa_to_rotmat_backward_per_group(built_lib, cuda_dev, aa):
    """Through ops.aa_to_rotmat under autograd.  The fp32 reference of a group is the tighter of the two forms (the quaternion form the
    operator computes, the Rodrigues form its adjoint is written from); the ratio against the Rodrigues form is printed beside it."""
    from tokenhmr_amd import ops
    x, spans = aa["x"], aa["spans"]
    xd = x.to(cuda_dev).requires_grad_(True)
    g, = torch.autograd.grad((ops.aa_to_rotmat(xd) * aa["gR"].to(cuda_dev)).sum(), xd)
    g = g.cpu()
    cands = {"quat": aa["quat32"], "rod": aa["rod32"]}
    ref32 = {k: RC.tighter(cands, aa["bwd64"], lo, hi)[1] for k, (lo, hi) in spans.items()}
    table = []
    fails = RC.check_groups("aa_to_rotmat_backward", g, ref32, aa["bwd64"], spans, table=table)
    _table("thmr_op_aa_to_rotmat_backward, against the tighter fp32 form", table)
    print("  ratio against the Rodrigues form in fp32: " +
          ", ".join(f"{k} {RC.ratio(g[lo:hi], aa['rod32'][lo:hi], aa['bwd64'][lo:hi]):.3g}" for k, (lo, hi) in spans.items()))
    assert torch.isfinite(g).all()
    assert not fails, "\n".join(fails)


def test_the_nan_row_is_nan_as_in_the_reference(built_lib, cuda_dev):
    """aa = (-1e-8, -1e-8, -1e-8) in fp32: theta + 1e-8 is exactly zero, the reference returns NaN in all nine elements and all three of
    the gradient, and so does the device.  Recorded as the reference's behaviour, not as something to fix.  The rows beside it keep the
    bits they have without it."""
    from tokenhmr_amd import ops
    rows = RC.nan_rows()
    gR = RC.grad_out(3, RC.SEED_GRAD + 2)
    assert torch.isnan(RC.fwd(O.aa_to_rotmat, rows, torch.float32)[1]).all()

    def run(t, gr):
        xd = t.to(cuda_dev).requires_grad_(True)
        R = ops.aa_to_rotmat(xd)
        g, = torch.autograd.grad((R * gr.to(cuda_dev)).sum(), xd)
        return R.detach().cpu(), g.cpu()

    R, g = run(rows, gR)
    print(f"NaN row: device forward {int(torch.isnan(R[1]).sum())} of 9 NaN, backward {int(torch.isnan(g[1]).sum())} of 3 NaN")
    assert torch.isnan(R[1]).all() and torch.isnan(g[1]).all()
    R2, g2 = run(rows[[0, 2]], gR[[0, 2]])
    assert torch.isfinite(R2).all() and torch.isfinite(g2).all()
    assert torch.equal(R[[0, 2]], R2) and torch.equal(g[[0, 2]], g2)


# ------------------------------------------------------------------------------------------------ thmr_op_rot6d, thmr_op_rot6d_backward
def test_rot6d_per_group(built_lib, cuda_dev, r6):
    from tokenhmr_amd import ops
    x, spans = r6["x"], r6["spans"]
    R = ops.rot6d_to_rotmat(x.to(cuda_dev)).cpu()
    table = []
    fails = RC.check_groups("rot6d", R, r6["fwd32"], r6["fwd64"], spans, table=table)
    _table("thmr_op_rot6d", table)
    assert torch.isfinite(R).all()
    for g in RC.CLAMP_GROUPS:                          # the clamp: zero rows where the reference has zero rows
        lo, hi = spans[g]
        ref_zero = (r6["fwd32"][lo:hi] == 0).all(dim=-1)
        assert torch.equal((R[lo:hi] == 0).all(dim=-1), ref_zero), g
        assert ref_zero.any() or g == "a1_1e-13"
    lo, hi = spans["a1_1e-13"]                         # b1 = a1 / 1e-12: length 0.1, not 1
    assert torch.allclose(R[lo:hi, 0].norm(dim=-1), torch.full((RC.GROUP,), 0.1), rtol=1e-5, atol=0)
    lo, hi = spans["a2_eq_2a1"]                        # property-only: b2's direction is rounding; b1 to the rule, no row longer than 1 + 4 ulp
    ok, line = SB.check("rot6d [a2_eq_2a1, b1 only]", R[lo:hi, 0], r6["fwd32"][lo:hi, 0], r6["fwd64"][lo:hi, 0], RC.MULT)
    fails += [] if ok else [line]
    assert (R[lo:hi].double().norm(dim=-1) <= 1 + 4 * ULP).all(), R[lo:hi].double().norm(dim=-1).max().item() - 1
    assert not fails, "\n".join(fails)


def test_rot6d_backward_per_group(built_lib, cuda_dev, r6):
    """The clamp groups' gradients are O(1e12); the rule is relative to the reference's own distance there as everywhere."""
    from tokenhmr_amd import ops
    x, spans = r6["x"], r6["spans"]
    g = ops.rot6d_backward(x.to(cuda_dev), r6["gR"].to(cuda_dev)).cpu()
    table = []
    fails = RC.check_groups("rot6d_backward", g, r6["bwd32"], r6["bwd64"], spans, table=table)
    _table("thmr_op_rot6d_backward", table)
    lo, hi = spans["a1_zero"]
    assert g[lo:hi].abs().max() > 1e11                 # the clamp groups do reach the division by eps
    assert torch.isfinite(g).all()                     # a2 = 2 a1 included: finite only
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ thmr_op_head_finish
HEADS = {"token": 32, "hmr2": 160}


@pytest.mark.parametrize("kind", ["token", "hmr2"])
def test_head_finish_joints_across_the_6d_groups(built_lib, cuda_dev, r6, kind):
    """B = 2: the 48 joints take four rows of each compared 6D group (init_pose = 0, so pose6d is the input bits)."""
    from tokenhmr_amd import ops
    groups = RC.compared(r6["spans"])
    idx = torch.tensor([r6["spans"][groups[j % len(groups)]][0] + 5 + j // len(groups) for j in range(48)])
    p6 = r6["x"][idx].reshape(2, 144).contiguous()
    ro = torch.zeros(2, HEADS[kind])
    bpose = None
    if kind == "token":
        ro[:, :6], bpose, ro[:, 19:31] = p6[:, :6], p6[:, 6:132].contiguous(), p6[:, 132:]
    else:
        ro[:, :144] = p6
    dev = lambda t: None if t is None else t.to(cuda_dev)      # noqa: E731
    o = ops.head_finish(kind, dev(ro), dev(torch.zeros(144)), dev(torch.zeros(10)), dev(torch.tensor([2.0, 0.0, 0.0])), bpose=dev(bpose))
    assert torch.equal(o["pose6d"].cpu(), p6)
    R = o["rotmat"].cpu().reshape(48, 3, 3)
    sub = {g: [4 * i, 4 * i + 4] for i, g in enumerate(groups)}
    order = torch.tensor([j for i in range(len(groups)) for j in range(48) if j % len(groups) == i])     # joints sorted by group
    table = []
    fails = RC.check_groups(f"head_finish/{kind}", R[order], r6["fwd32"][idx][order], r6["fwd64"][idx][order], sub, table=table)
    _table(f"thmr_op_head_finish ({kind}) rotmat, 4 joints per group", table)
    alone = ops.rot6d_to_rotmat(r6["x"][idx].to(cuda_dev)).cpu()
    print(f"head_finish ({kind}): the rows of its 6D step equal thmr_op_rot6d's bit for bit: {torch.equal(alone, R)}")
    assert torch.isfinite(R).all()
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ thmr_op_rotmat_to_aa o thmr_op_aa_to_rotmat
def test_round_trip_below_pi(built_lib, cuda_dev, aa):
    from tokenhmr_amd import ops
    x, spans = aa["x"], aa["spans"]
    keep = x.double().norm(dim=1) <= np.pi - 1e-2
    groups = [g for g, (lo, hi) in spans.items() if keep[lo:hi].any()]
    assert groups == ["zero", "n1e-9", "n1e-8", "n1e-7", "n1e-6", "n1e-4", "n1e-2", "randn0.8", "one_axis"]
    back = ops.rotmat_to_aa(ops.aa_to_rotmat(x.to(cuda_dev))).cpu()
    with torch.no_grad():
        r32, r64 = TO.matrix_to_axis_angle(O.aa_to_rotmat(x)), TO.matrix_to_axis_angle(O.aa_to_rotmat(x.double()))
    assert torch.isfinite(r32[keep]).all() and torch.isfinite(r64[keep]).all()
    table = []
    fails = RC.check_groups("rotmat_to_aa o aa_to_rotmat", back, r32, r64, spans, groups=groups, table=table, keep=keep)
    _table("thmr_op_rotmat_to_aa o thmr_op_aa_to_rotmat, |aa| <= pi - 1e-2", table)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ SMPL with pose2rot = 1
def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _smpl_inputs():
    rng = np.random.default_rng(RC.SEED_AA + 11)
    pose = np.zeros((3, 24, 3))                                          # item 0: the zero pose
    u = rng.standard_normal((24, 3))
    pose[1] = 1e-7 * u / np.linalg.norm(u, axis=1, keepdims=True)        # item 1: every joint at |aa| = 1e-7
    pose[2] = 0.6 * rng.standard_normal((24, 3))                         # item 2: generic, the padded hands (22, 23) zero
    pose[2, 22:] = 0.0
    f = lambda a: torch.from_numpy(a).float()                            # noqa: E731
    return f(pose).reshape(3, 72), f(rng.standard_normal((3, 10))), f(rng.standard_normal((3, 44, 3)))


def test_smpl_axis_angle_at_zero_and_tiny_poses(built_lib, cuda_dev):
    """Forward: the zero pose through rodrigues_kernel is the identity exactly, so item 0 equals the pose2rot = 0 call on identity matrices bit
    for bit.  Backward: grad_pose per item to the rule; the truth is tests/lbs_backward_numpy.py in float64 chained through float64 autograd
    of batch_rodrigues, the fp32 reference the oracle's own autograd in fp32, both of sum(joints * gJ) as
    tests/test_gpu_val_loss_grad.py::_smpl_truth32 takes it (what the validation loss feeds the body model).  A dense vertex gradient is NOT
    added: measured on eight generic poses, gV ~ N(0, 1) puts grad_R of the pose2rot = 0 call, which no rotation kernel touches, at 1.0 ...
    5.4 times the reference's own distance per item (the skin-backward's fp32 sums over 6890 vertices), and that would decide this test.  SMPL-H is left out: both models reach the same two kernels
    (launch_rodrigues, launch_rodrigues_backward through resolve_pose / finish_pose_grad in csrc/body_model_abi.hip), and its float64 chain would be a second copy of this test."""
    from tokenhmr_amd.smpl import SMPL
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    smpl = make_synthetic_smpl(seed=0)
    smpl["update_hips"] = True
    pose, betas, gJ = _smpl_inputs()
    m = SMPL(smpl, max_batch=3, device=cuda_dev).enable_grad()
    pd, bd, gJd = (t.to(cuda_dev).contiguous() for t in (pose, betas, gJ))
    out = m(pd[:, :3], pd[:, 3:], bd, pose2rot=True)
    eye = torch.eye(3, device=cuda_dev).expand(3, 24, 3, 3).contiguous()
    ident = m(eye[:, :1], eye[:, 1:], bd, pose2rot=False)
    same_v, same_j = torch.equal(out.vertices[0], ident.vertices[0]), torch.equal(out.joints[0], ident.joints[0])
    print(f"SMPL forward, zero pose, pose2rot = 1 against identity matrices: vertices bit-equal {same_v}, joints bit-equal {same_j}")
    out = m(pd[:, :3], pd[:, 3:], bd, pose2rot=True)           # the backward follows its own forward
    gp = torch.empty_like(pd)
    with torch.cuda.device(cuda_dev):
        st = C.c_void_p(torch.cuda.current_stream(cuda_dev).cuda_stream)
        m._check(m.lib.thmr_smpl_backward(m.h, _p(pd), 1, _p(bd), 3, C.c_void_p(0), _p(gJd), _p(gp), C.c_void_p(0), st), "thmr_smpl_backward")
    torch.cuda.synchronize()
    gp = gp.cpu()
    m.close()
    # truth
    R64 = O.batch_rodrigues(pose.double().reshape(-1, 3)).reshape(3, 24, 3, 3)
    gR64, _ = L.smpl_backward(R64.numpy(), betas.double().numpy(), None, gJ.double().numpy(), smpl)
    r64 = RC.vjp(O.batch_rodrigues, pose.reshape(-1, 3), torch.from_numpy(gR64).reshape(-1, 3, 3), torch.float64).reshape(3, 72)
    p32, b32 = pose.clone().requires_grad_(True), betas.clone()
    v, j = O.smpl_forward_axis_angle(p32[:, :3], p32[:, 3:], b32, smpl)
    r32, = torch.autograd.grad((j * gJ).sum(), p32)
    assert torch.isfinite(r32).all() and torch.isfinite(r64).all() and torch.isfinite(gp).all()
    fails = []
    for b, tag in enumerate(("zero pose", "|aa| = 1e-7", "generic, joints 22 and 23 zero")):
        ok, line = SB.check(f"SMPL backward grad_pose, item {b} ({tag}):", gp[b], r32[b], r64[b], RC.MULT)
        fails += [] if ok else [line]
    assert same_v and same_j, "rodrigues_kernel at the zero pose does not hand the body model the identity's bits"
    assert not fails, "\n".join(fails)
