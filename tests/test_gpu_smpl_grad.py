"""The body model's backward on the device (thmr_smpl_backward) against float64 autograd of the oracle's forward, under the
project's rule (tests/stage_bounds.py): the device may be MULT x as far from float64 as the same autograd in fp32 on the CPU is on the same
inputs, and never needs to be closer than 4 ulp of the tensor's largest element.  Every check prints the measured ratio."""
import ctypes as C

import numpy as np
import pytest
import torch

import rotation_cases as RC
import stage_bounds as SB
from tests import guarded as G

pytestmark = pytest.mark.gpu

MULT = 2.0            # the project's rule; no tensor of this file carries more
POOL = 11             # coprime to every crops-per-pass value and to 32: row b holds pool item b % 11


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _smpl(hips=False, dup=False, seed=0):
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    smpl = make_synthetic_smpl(seed=seed)
    smpl["update_hips"] = hips
    if dup:                   # as test_gpu_lbs_duplicate_extra_vertex_ids_and_repeated_calls: slots 0 and 1, 4 and 9 name one vertex each
        ev = smpl["extra_verts"].clone()
        ev[1], ev[9] = ev[0], ev[4]
        smpl["extra_verts"] = ev
    return smpl


def _inputs(B, seed, pose2rot):
    from oracle.lbs_independent import random_rotations
    rng = np.random.default_rng(seed)
    if pose2rot:
        pose = torch.from_numpy(0.6 * rng.standard_normal((B, 24, 3))).float()
        pose[0, 5] = 0.0                                               # an all-zero joint
        pose[min(1, B - 1), 7] = torch.tensor([6e-5, -7e-5, 4e-5])     # one of norm 1e-4
        pose = pose.reshape(B, 72)
    else:
        pose = torch.from_numpy(random_rotations(B * 24, seed=seed).reshape(B, 24, 3, 3)).float()
    betas = torch.from_numpy(rng.standard_normal((B, 10))).float()
    gV = torch.from_numpy(rng.standard_normal((B, 6890, 3))).float()
    gJ = torch.from_numpy(rng.standard_normal((B, 44, 3))).float()
    return pose, betas, gV, gJ


def _truth(smpl, pose, betas, gV, gJ, pose2rot, dtype):
    """torch autograd through the oracle on the CPU in `dtype`: (grad_pose, grad_betas)."""
    from oracle import tokenhmr_oracle as O
    s = SB.to64(smpl) if dtype == torch.float64 else smpl
    pose, betas = pose.to(dtype).clone().requires_grad_(True), betas.to(dtype).clone().requires_grad_(True)
    if pose2rot:
        v, j = O.smpl_forward_axis_angle(pose[:, :3], pose[:, 3:], betas, s)
    else:
        v, j = O.smpl_forward(pose[:, :1], pose[:, 1:], betas, s)
    loss = (0 if gV is None else (v * gV.to(dtype)).sum()) + (0 if gJ is None else (j * gJ.to(dtype)).sum())
    return torch.autograd.grad(loss, (pose, betas))


def _backward(m, pose, betas, gV, gJ, pose2rot, want_pose=True, want_betas=True):
    """thmr_smpl_backward through the C call: device tensors in, (grad_pose, grad_betas) out."""
    m.enable_grad()
    B = betas.shape[0]
    gp = torch.empty_like(pose) if want_pose else None
    gb = torch.empty_like(betas) if want_betas else None
    with torch.cuda.device(m.device):
        st = C.c_void_p(torch.cuda.current_stream(m.device).cuda_stream)
        m._check(m.lib.thmr_smpl_backward(m.h, _p(pose), 1 if pose2rot else 0, _p(betas), B, _p(gV), _p(gJ), _p(gp), _p(gb), st),
                 "thmr_smpl_backward")
    return gp, gb


def _dev(dev, *ts):
    return [None if t is None else t.to(dev).contiguous() for t in ts]


def _hold(tag, got, ref32, ref64, fails):
    for name, g, r32, r64 in (("grad_pose", got[0], ref32[0], ref64[0]), ("grad_betas", got[1], ref32[1], ref64[1])):
        ok, line = SB.check(f"{tag} {name}", g.cpu(), r32, r64, MULT)
        if not ok:
            fails.append(line)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("arm", ["both", "gV", "gJ"])
@pytest.mark.parametrize("pose2rot", [False, True], ids=["rotmat", "axis_angle"])
@pytest.mark.parametrize("hips", [False, True], ids=["plain", "update_hips"])
def test_gpu_smpl_backward_parity(built_lib, cuda_dev, hips, pose2rot, arm):
    from tokenhmr_amd.smpl import SMPL
    smpl = _smpl(hips)
    pose, betas, gV, gJ = _inputs(5, 51, pose2rot)
    gV, gJ = (gV if arm != "gJ" else None), (gJ if arm != "gV" else None)
    r64, r32 = _truth(smpl, pose, betas, gV, gJ, pose2rot, torch.float64), _truth(smpl, pose, betas, gV, gJ, pose2rot, torch.float32)
    m = SMPL(smpl, max_batch=8, device=cuda_dev)
    got = _backward(m, *_dev(cuda_dev, pose, betas, gV, gJ), pose2rot)
    torch.cuda.synchronize()
    m.close()
    fails = []
    _hold(f"5 crops, update_hips={hips}, pose2rot={pose2rot}, {arm}:", got, r32, r64, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ 2. every joint path, one call
@pytest.mark.parametrize("dup", [False, True], ids=["plain_ids", "duplicate_ids"])
def test_gpu_smpl_backward_every_joint_path(built_lib, cuda_dev, dup):
    """Row b's gJ is one-hot on joint b (all three coordinates), gV is absent: the joint_map adjoint, each picked vertex, both hips and
    each J19 row, each held to the bound on its own row."""
    from tokenhmr_amd.smpl import SMPL
    smpl = _smpl(True, dup, seed=4 if dup else 0)
    pose, betas, _, _ = _inputs(44, 61, False)
    gJ = torch.zeros(44, 44, 3)
    gJ[torch.arange(44), torch.arange(44)] = torch.tensor([1.0, -0.75, 0.5])
    r64, r32 = _truth(smpl, pose, betas, None, gJ, False, torch.float64), _truth(smpl, pose, betas, None, gJ, False, torch.float32)
    m = SMPL(smpl, max_batch=44, device=cuda_dev)
    got = _backward(m, *_dev(cuda_dev, pose, betas, None, gJ), False)
    torch.cuda.synchronize()
    m.close()
    fails = []
    for b in range(44):
        _hold(f"joint {b} (duplicate ids={dup}):", (got[0][b], got[1][b]), (r32[0][b], r32[1][b]), (r64[0][b], r64[1][b]), fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ 3. batch-shape edges
# launch_lbs_backward (tokenhmr_amd/csrc/body_model.hip) walks the forward's crops per workgroup pass, cg = B / 32 capped at 8, with the bone
# matrices double-buffered on c & 1; the blend GEMM's reverse is ONE tile shape (64 rows x 128) and ONE ksplit (38) at every size, so its
# only edges are whole and ragged 64-row tiles
EDGE_BATCHES = (31, 32, 63,       # cg 1; 63: a ragged 64-row GEMM tile
                64, 65, 95,       # cg 2: whole, last pass of one (and the second GEMM row tile, one row), last pass of one at 47 whole passes
                96, 100,          # cg 3 (an odd pass): whole, last pass of one
                128, 129,         # cg 4: whole GEMM row tiles, a third of one row
                161,              # cg 5: last pass of one
                255,              # cg 7: last pass of three
                256, 257)         # cg 8: whole, last pass of one
STATE_BATCHES = (257, 65)


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "update_hips"])
def edge_case(request, cuda_dev):
    smpl = _smpl(request.param)
    pose, betas, gV, gJ = _inputs(POOL, 71, False)
    case = dict(smpl=smpl, host=(pose, betas, gV, gJ), r64=_truth(smpl, pose, betas, gV, gJ, False, torch.float64),
                r32=_truth(smpl, pose, betas, gV, gJ, False, torch.float32), model=None, fresh={})
    yield case
    if case["model"] is not None:
        case["model"].close()


def _edge_model(case, dev):
    from tokenhmr_amd.smpl import SMPL
    if case["model"] is None:
        case["model"] = SMPL(case["smpl"], max_batch=257, device=dev)
    return case["model"]


def _edge_run(m, case, B, dev):
    sel = torch.arange(B) % POOL
    return _backward(m, *_dev(dev, *(t[sel] for t in case["host"])), False)


@pytest.mark.parametrize("B", EDGE_BATCHES)
def test_gpu_smpl_backward_batch_edges(built_lib, cuda_dev, edge_case, B):
    m = _edge_model(edge_case, cuda_dev)
    gp, gb = _edge_run(m, edge_case, B, cuda_dev)
    torch.cuda.synchronize()
    assert torch.equal(gp[POOL:], gp[:B - POOL]) and torch.equal(gb[POOL:], gb[:B - POOL]), \
        "rows b and b + 11 hold the same pose, shape and incoming gradients but differ"
    fails = []
    _hold(f"{B} crops (update_hips={edge_case['smpl']['update_hips']}), first {POOL} rows:", (gp[:POOL], gb[:POOL]), edge_case["r32"],
          edge_case["r64"], fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ 4. state
def test_gpu_smpl_backward_state(built_lib, cuda_dev, edge_case):
    """257 -> 65 -> 257 crops on ONE handle give the bits a fresh handle gives at each size; two identical calls are bit-equal; a
    backward issued after an unrelated forward on the same handle equals the one issued straight after its own forward."""
    from tokenhmr_amd.smpl import SMPL
    case = edge_case
    want = {}
    for B in STATE_BATCHES:
        f = SMPL(case["smpl"], max_batch=257, device=cuda_dev)
        want[B] = [t.clone() for t in _edge_run(f, case, B, cuda_dev)]
        torch.cuda.synchronize()
        f.close()
    m = SMPL(case["smpl"], max_batch=257, device=cuda_dev)
    for B in (257, 65, 257, 257):
        gp, gb = _edge_run(m, case, B, cuda_dev)
        assert torch.equal(gp, want[B][0]) and torch.equal(gb, want[B][1]), B
    # an unrelated forward in between: other poses, another batch size
    pose, betas, gV, gJ = _dev(cuda_dev, *(t[torch.arange(65) % POOL] for t in case["host"]))
    m(pose[:, :1], pose[:, 1:], betas, pose2rot=False)
    other = _dev(cuda_dev, *_inputs(40, 99, True)[:2])
    m(other[0][:, :3], other[0][:, 3:], other[1], pose2rot=True)
    gp, gb = _backward(m, pose, betas, gV, gJ, False)
    assert torch.equal(gp, want[65][0]) and torch.equal(gb, want[65][1])
    torch.cuda.synchronize()
    m.close()


# ------------------------------------------------------------------------------------------------ 5. the forward is untouched
@pytest.mark.parametrize("pose2rot", [False, True], ids=["rotmat", "axis_angle"])
def test_gpu_smpl_differentiable_forward_is_the_plain_forward(built_lib, cuda_dev, pose2rot):
    from tokenhmr_amd.smpl import SMPL
    smpl = _smpl(True)
    pose, betas = _dev(cuda_dev, *_inputs(37, 81, pose2rot)[:2])
    n = 3 if pose2rot else 1
    plain_handle = SMPL(smpl, max_batch=37, device=cuda_dev)
    never = plain_handle(pose[:, :n], pose[:, n:], betas, pose2rot=pose2rot)
    m = SMPL(smpl, max_batch=37, device=cuda_dev)
    p = pose.clone().requires_grad_(True)
    diff = m(p[:, :n], p[:, n:], betas, pose2rot=pose2rot)
    plain = m(pose[:, :n], pose[:, n:], betas, pose2rot=pose2rot)
    assert diff.vertices.grad_fn is not None and diff.joints.grad_fn is not None
    assert plain.vertices.grad_fn is None and never.vertices.grad_fn is None
    for a in ("vertices", "joints"):
        assert torch.equal(getattr(diff, a).detach(), getattr(plain, a)), a
        assert torch.equal(getattr(diff, a).detach(), getattr(never, a)), a
    assert not plain_handle._grad_ready and m._grad_ready
    torch.cuda.synchronize()
    plain_handle.close()
    m.close()


# ------------------------------------------------------------------------------------------------ 6. autograd plumbing
def test_gpu_smpl_autograd_plumbing(built_lib, cuda_dev):
    from oracle import tokenhmr_oracle as O
    from tokenhmr_amd.smpl import SMPL
    smpl = _smpl(True)
    B = 4
    pose, betas, _, _ = _inputs(B, 91, True)
    rng = np.random.default_rng(5)
    target = torch.from_numpy(rng.standard_normal((B, 44, 2))).float()
    cam_t = torch.tensor([[0.1, -0.2, 30.0]]).repeat(B, 1)
    focal = torch.full((B, 2), 5000.0 / 256.0)

    def loss_of(joints, dtype, dev):
        return (O.perspective_projection(joints, cam_t.to(dev, dtype), focal.to(dev, dtype)) - target.to(dev, dtype)).pow(2).sum()

    def truth(dtype):
        s = SB.to64(smpl) if dtype == torch.float64 else smpl
        go, bp, bt = (t.to(dtype).clone().requires_grad_(True) for t in (pose[:, :3], pose[:, 3:], betas))
        _, j = O.smpl_forward_axis_angle(go, bp, bt, s)
        return torch.autograd.grad(loss_of(j, dtype, "cpu"), (go, bp, bt))

    r64, r32 = truth(torch.float64), truth(torch.float32)
    m = SMPL(smpl, max_batch=B, device=cuda_dev)
    go = pose[:, :3].to(cuda_dev).requires_grad_(True)
    bp = pose[:, 3:].to(cuda_dev).requires_grad_(True)
    bt = betas.to(cuda_dev).requires_grad_(True)
    out = m(go, bp, bt, pose2rot=True)
    loss = loss_of(out.joints, torch.float32, cuda_dev)
    got = torch.autograd.grad(loss, (go, bp, bt), retain_graph=False)
    assert got[0].shape == (B, 3) and got[1].shape == (B, 69) and got[2].shape == (B, 10)
    fails = []
    for name, g, a, b in zip(("global_orient", "body_pose", "betas"), got, r32, r64):
        ok, line = SB.check(f"autograd, reprojection loss, grad {name}:", g.cpu(), a, b, MULT)
        if not ok:
            fails.append(line)
    # a second backward through the same graph: torch's own error, not a fault
    with pytest.raises(RuntimeError, match="second time|already been freed"):
        torch.autograd.grad(loss, (go, bp, bt))
    # under no_grad: no graph
    with torch.no_grad():
        o2 = m(go, bp, bt, pose2rot=True)
    assert o2.vertices.grad_fn is None and o2.joints.grad_fn is None and not o2.vertices.requires_grad
    # an input without requires_grad gets None; rotation matrices come back in the shapes passed; a non-contiguous incoming gradient
    R = O.batch_rodrigues(pose.reshape(-1, 3)).view(B, 24, 3, 3).to(cuda_dev)
    gor, bpr = R[:, :1].clone().requires_grad_(True), R[:, 1:].clone()
    o3 = m(gor, bpr, bt.detach(), pose2rot=False)
    w = torch.randn(B, 3, 6890, device=cuda_dev).transpose(1, 2)               # (B,6890,3), not contiguous
    (o3.vertices * w).sum().backward()
    assert gor.grad.shape == (B, 1, 3, 3) and bpr.grad is None and bt.grad is None
    assert torch.isfinite(gor.grad).all() and gor.grad.abs().max() > 0
    torch.cuda.synchronize()
    m.close()
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ 7. capture
def test_gpu_smpl_forward_backward_captured(built_lib, cuda_dev):
    """After enable_grad(): forward + backward captured in one graph on one stream; replayed on new input values it equals eager."""
    from tokenhmr_amd.smpl import SMPL
    B = 9
    m = SMPL(_smpl(True), max_batch=B, device=cuda_dev).enable_grad()
    ins = [_dev(cuda_dev, *_inputs(B, 100 + k, True)) for k in range(3)]
    pose, betas, gV, gJ = (t.clone() for t in ins[0])
    verts, joints = torch.empty(B, 6890, 3, device=cuda_dev), torch.empty(B, 44, 3, device=cuda_dev)
    gp, gb = torch.empty_like(pose), torch.empty_like(betas)

    def run(stream):
        st = C.c_void_p(stream.cuda_stream)
        m._check(m.lib.thmr_smpl_forward(m.h, _p(pose), 1, _p(betas), B, _p(verts), _p(joints), st), "thmr_smpl_forward")
        m._check(m.lib.thmr_smpl_backward(m.h, _p(pose), 1, _p(betas), B, _p(gV), _p(gJ), _p(gp), _p(gb), st), "thmr_smpl_backward")

    eager = []
    for k in range(3):
        for dst, src in zip((pose, betas, gV, gJ), ins[k]):
            dst.copy_(src)
        run(torch.cuda.current_stream(cuda_dev))
        torch.cuda.synchronize()
        eager.append([t.clone() for t in (verts, joints, gp, gb)])
    assert not torch.equal(eager[1][2], eager[2][2])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(torch.cuda.current_stream(cuda_dev))
    for k in (1, 2):
        for dst, src in zip((pose, betas, gV, gJ), ins[k]):
            dst.copy_(src)
        for t in (verts, joints, gp, gb):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for t, e in zip((verts, joints, gp, gb), eager[k]):
            assert torch.equal(t, e), k
    del graph
    m.close()


# ------------------------------------------------------------------------------------------------ 8. guard bands and refusals
@pytest.mark.parametrize("pose2rot", [False, True], ids=["rotmat", "axis_angle"])
def test_gpu_smpl_backward_guard_bands(built_lib, cuda_dev, pose2rot):
    from tokenhmr_amd.smpl import SMPL
    B = 33
    m = SMPL(_smpl(True), max_batch=B + 3, device=cuda_dev).enable_grad()
    pose, betas, gV, gJ = _dev(cuda_dev, *_inputs(B, 111, pose2rot))
    gp, check_p = G.guarded(B, 72 if pose2rot else 216, device=cuda_dev)
    gb, check_b = G.guarded(B, 10, device=cuda_dev)
    assert gp.is_contiguous() and gb.is_contiguous()
    with torch.cuda.device(cuda_dev):
        st = C.c_void_p(torch.cuda.current_stream(cuda_dev).cuda_stream)
        m._check(m.lib.thmr_smpl_backward(m.h, _p(pose), 1 if pose2rot else 0, _p(betas), B, _p(gV), _p(gJ), _p(gp), _p(gb), st),
                 "thmr_smpl_backward")
    torch.cuda.synchronize()
    check_p()
    check_b()
    for t in (gp, gb):
        assert not (t.contiguous().view(torch.int32) == G.CANARY[torch.float32]).any(), "an output element was left unwritten"
        assert torch.isfinite(t).all()
    want = _backward(m, pose, betas, gV, gJ, pose2rot)
    assert torch.equal(gp.reshape(want[0].shape), want[0]) and torch.equal(gb, want[1])
    m.close()


def test_gpu_smpl_backward_refusals(built_lib, cuda_dev):
    from tokenhmr_amd import _cabi
    from tokenhmr_amd.smpl import SMPL
    B = 4
    m = SMPL(_smpl(), max_batch=B, device=cuda_dev)
    lib = m.lib
    pose, betas, gV, gJ = _dev(cuda_dev, *_inputs(B, 121, False))
    gp, check_p = G.guarded(B, 216, device=cuda_dev)
    gb, check_b = G.guarded(B, 10, device=cuda_dev)
    st = C.c_void_p(torch.cuda.current_stream(cuda_dev).cuda_stream)

    def refused(what, *args):
        rc = lib.thmr_smpl_backward(*args, st)
        msg = (lib.thmr_last_error(None) or b"").decode()
        assert rc == _cabi.ERR_INVALID and what in msg, (rc, msg)

    P, Bt, V, J, GP, GB = _p(pose), _p(betas), _p(gV), _p(gJ), _p(gp), _p(gb)
    refused("first", m.h, P, 0, Bt, B, V, J, GP, GB)                       # not reserved yet
    m.enable_grad()
    assert lib.thmr_smpl_grad_reserve(m.h) == 0                            # idempotent
    refused("null handle", None, P, 0, Bt, B, V, J, GP, GB)
    refused("null handle, pose or betas", m.h, None, 0, Bt, B, V, J, GP, GB)
    refused("null handle, pose or betas", m.h, P, 0, None, B, V, J, GP, GB)
    refused("both null", m.h, P, 0, Bt, B, None, None, GP, GB)
    refused("both null", m.h, P, 0, Bt, B, V, J, None, None)
    refused("max_batch", m.h, P, 0, Bt, 0, V, J, GP, GB)
    refused("max_batch", m.h, P, 0, Bt, B + 1, V, J, GP, GB)
    refused("0 or 1", m.h, P, 2, Bt, B, V, J, GP, GB)
    assert lib.thmr_smpl_grad_reserve(None) == _cabi.ERR_INVALID
    for args in ((None, V, P, 3), (P, None, P, 3), (P, V, None, 3), (P, V, P, 0)):
        assert lib.thmr_op_aa_to_rotmat_backward(*args, st) == _cabi.ERR_INVALID
    torch.cuda.synchronize()
    check_p()
    check_b()
    for t in (gp, gb):                                                     # nothing was launched: every canary is still there
        assert (t.contiguous().view(torch.int32) == G.CANARY[torch.float32]).all()
    m.close()


# ------------------------------------------------------------------------------------------------ 9. ops.aa_to_rotmat
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_gpu_aa_to_rotmat_backward(built_lib, cuda_dev, n):
    from oracle import tokenhmr_oracle as O
    from tokenhmr_amd import ops
    rng = np.random.default_rng(n)
    aa = torch.from_numpy(0.8 * rng.standard_normal((n, 3))).float()
    gR = torch.from_numpy(rng.standard_normal((n, 3, 3))).float()

    def truth(dtype, fn=O.batch_rodrigues):
        t = aa.to(dtype).clone().requires_grad_(True)
        return torch.autograd.grad((fn(t) * gR.to(dtype)).sum(), t)[0]

    x = aa.to(cuda_dev).requires_grad_(True)
    R = ops.aa_to_rotmat(x)
    assert R.grad_fn is not None and torch.equal(R.detach(), ops.aa_to_rotmat(x.detach()))
    g, = torch.autograd.grad((R * gR.to(cuda_dev)).sum(), x)
    with torch.no_grad():
        assert ops.aa_to_rotmat(x).grad_fn is None
    # the fp32 reference is the tighter of the two forms against the SAME truth (tests/test_gpu_rotation_edges.py): the quaternion form the
    # operator computes (geometry.py:5-44) or the Rodrigues form its adjoint is written from; the bound can only be the earlier one or less
    r64 = truth(torch.float64)
    name, r32 = RC.tighter({"rod": truth(torch.float32), "quat": truth(torch.float32, O.aa_to_rotmat)}, r64, 0, n)
    ok, line = SB.check(f"aa_to_rotmat backward, n = {n} (fp32 reference: {name}):", g.cpu(), r32, r64, MULT)
    assert ok, line
