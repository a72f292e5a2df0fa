"""SMPL-H's backward on the device (thmr_smplh_backward, both paths) against float64 autograd of smplx's formulation
(tests/smplh_backward_numpy.py::smplh_forward_generic), under the project's rule (tests/stage_bounds.py): the device may be MULT x as far
from float64 as the same autograd in fp32 on the CPU is on the same inputs, and never needs to be closer than 4 ulp of the tensor's largest
element.  Every check prints the measured ratio.  The truth of the folded path is the 52-joint model with identity hands."""
import ctypes as C

import numpy as np
import pytest
import torch

import smplh_backward_numpy as HB
import stage_bounds as SB
from tests import guarded as G

pytestmark = pytest.mark.gpu

MULT = 2.0            # the project's rule; no tensor of this file carries more
POOL = 11             # coprime to every poses-per-workgroup value: row b holds pool item b % 11
NAMES = ("grad_pose", "grad_betas", "grad_transl")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _asset(dup=False, seed=0):
    from tokenhmr_amd.smpl_assets import make_synthetic_smplh
    c = make_synthetic_smplh(seed=seed)
    if dup:                   # slots 0 and 1, 4 and 9 name one vertex each
        ev = c["extra_verts"].clone()
        ev[1], ev[9] = ev[0], ev[4]
        c["extra_verts"] = ev
    return c


def _inputs(B, seed, body_only, pose2rot):
    from smplh_oracle import random_rotations
    nj = 22 if body_only else 52
    rng = np.random.default_rng(seed)
    if pose2rot:
        pose = torch.from_numpy(0.6 * rng.standard_normal((B, nj, 3))).float()
        pose[0, 5] = 0.0                                               # an all-zero joint
        pose[min(1, B - 1), 7] = torch.tensor([6e-5, -7e-5, 4e-5])     # one of norm 1e-4
        pose = pose.reshape(B, nj * 3)
    else:
        pose = torch.from_numpy(random_rotations(B * nj, seed=seed).reshape(B, nj, 3, 3)).float()
    betas = torch.from_numpy(rng.standard_normal((B, 10))).float()
    transl = torch.from_numpy(0.3 * rng.standard_normal((B, 3))).float()
    gV = torch.from_numpy(rng.standard_normal((B, 6890, 3))).float()
    gJ = torch.from_numpy(rng.standard_normal((B, 73, 3))).float()
    return pose, betas, transl, gV, gJ


def _truth(c, pose, betas, transl, gV, gJ, body_only, pose2rot, dtype):
    """torch autograd through smplx's formulation on the CPU in `dtype`: (grad_pose, grad_betas, grad_transl)."""
    s = SB.to64(c) if dtype == torch.float64 else c
    B, nj = pose.shape[0], 22 if body_only else 52
    pose, betas, transl = (t.to(dtype).clone().requires_grad_(True) for t in (pose, betas, transl))
    R = HB.batch_rodrigues_generic(pose.reshape(-1, 3)).view(B, nj, 3, 3) if pose2rot else pose
    v, j = HB.smplh_forward_generic(HB.with_identity_hands(R) if body_only else R, betas, s, transl, dtype)
    loss = (0 if gV is None else (v * gV.to(dtype)).sum()) + (0 if gJ is None else (j * gJ.to(dtype)).sum())
    return torch.autograd.grad(loss, (pose, betas, transl))


def _model(c, max_batch, dev, paths=("folded", "full")):
    from tokenhmr_amd.smplh import SMPLHLayer
    return SMPLHLayer(c, max_batch=max_batch, device=dev).enable_grad(paths)


def _backward(m, pose, betas, transl, gV, gJ, body_only, pose2rot, want=(True, True, True)):
    """thmr_smplh_backward through the C call: device tensors in, (grad_pose, grad_betas, grad_transl) out."""
    B = pose.shape[0]
    gp = torch.empty_like(pose) if want[0] else None
    gb = torch.empty(B, 10, device=pose.device) if want[1] else None
    gt = torch.empty(B, 3, device=pose.device) if want[2] else None
    m._backward(pose, pose2rot, betas, transl, body_only, B, gV, gJ, gp, gb, gt)
    return gp, gb, gt


def _dev(dev, *ts):
    return [None if t is None else t.to(dev).contiguous() for t in ts]


def _hold(tag, got, ref32, ref64, fails):
    for name, g, r32, r64 in zip(NAMES, got, ref32, ref64):
        ok, line = SB.check(f"{tag} {name}", g.cpu(), r32, r64, MULT)
        if not ok:
            fails.append(line)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.fixture(scope="module")
def parity_model(cuda_dev):
    m = _model(_asset(), 8, cuda_dev)
    yield m
    m.close()


@pytest.mark.parametrize("arm", ["both", "gV", "gJ"])
@pytest.mark.parametrize("pose2rot", [False, True], ids=["rotmat", "axis_angle"])
@pytest.mark.parametrize("body_only", [True, False], ids=["folded", "full"])
def test_gpu_smplh_backward_parity(built_lib, cuda_dev, parity_model, body_only, pose2rot, arm):
    c = _asset()
    pose, betas, transl, gV, gJ = _inputs(5, 51, body_only, pose2rot)
    gV, gJ = (gV if arm != "gJ" else None), (gJ if arm != "gV" else None)
    r64 = _truth(c, pose, betas, transl, gV, gJ, body_only, pose2rot, torch.float64)
    r32 = _truth(c, pose, betas, transl, gV, gJ, body_only, pose2rot, torch.float32)
    got = _backward(parity_model, *_dev(cuda_dev, pose, betas, transl, gV, gJ), body_only, pose2rot)
    torch.cuda.synchronize()
    fails = []
    _hold(f"5 poses, {'folded' if body_only else 'full'}, pose2rot={pose2rot}, {arm}:", got, r32, r64, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ 2. every joint path, one call
@pytest.mark.parametrize("dup", [False, True], ids=["plain_ids", "duplicate_ids"])
@pytest.mark.parametrize("body_only", [True, False], ids=["folded", "full"])
def test_gpu_smplh_backward_every_joint_path(built_lib, cuda_dev, body_only, dup):
    """Row b's gJ is one-hot on joint b (all three coordinates), gV is absent: each chain joint, each picked vertex and — folded, rows
    22..51 — the wrist term, each held to the bound on its own row."""
    c = _asset(dup, seed=4 if dup else 0)
    pose, betas, transl, _, _ = _inputs(73, 61, body_only, False)
    gJ = torch.zeros(73, 73, 3)
    gJ[torch.arange(73), torch.arange(73)] = torch.tensor([1.0, -0.75, 0.5])
    r64 = _truth(c, pose, betas, transl, None, gJ, body_only, False, torch.float64)
    r32 = _truth(c, pose, betas, transl, None, gJ, body_only, False, torch.float32)
    m = _model(c, 73, cuda_dev, "folded" if body_only else "full")
    got = _backward(m, *_dev(cuda_dev, pose, betas, transl, None, gJ), body_only, False)
    torch.cuda.synchronize()
    m.close()
    fails = []
    for b in range(73):
        _hold(f"joint {b} ({'folded' if body_only else 'full'}, duplicate ids={dup}):", [g[b] for g in got], [r[b] for r in r32],
              [r[b] for r in r64], fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ 3. batch independence, reproducibility
# launch_smplh_backward (tokenhmr_amd/csrc/body_model.hip) walks the forward's poses per workgroup, smplh_poses_per_workgroup: 1 below
# 64 poses, 2 from 64, 4 from 128, 8 from 256, with the bone matrices double-buffered on c & 1; the blend GEMM's reverse is ONE tile shape
# (64 rows x 128) and ONE ksplit (38) at every size
EDGE_BATCHES = (63, 64, 65, 127, 128, 129, 255, 256, 257)


@pytest.fixture(scope="module", params=[True, False], ids=["folded", "full"])
def edge_case(request, cuda_dev):
    body_only = request.param
    c = _asset()
    host = _inputs(POOL, 71, body_only, False)
    case = dict(body_only=body_only, host=host, r64=_truth(c, *host, body_only, False, torch.float64),
                r32=_truth(c, *host, body_only, False, torch.float32),
                model=_model(c, 257, cuda_dev, "folded" if body_only else "full"))
    yield case
    case["model"].close()


def _edge_run(case, B, dev):
    sel = torch.arange(B) % POOL
    return _backward(case["model"], *_dev(dev, *(t[sel] for t in case["host"])), case["body_only"], False)


@pytest.mark.parametrize("B", EDGE_BATCHES)
def test_gpu_smplh_backward_batch_edges(built_lib, cuda_dev, edge_case, B):
    got = _edge_run(edge_case, B, cuda_dev)
    again = _edge_run(edge_case, B, cuda_dev)
    torch.cuda.synchronize()
    for name, g, a in zip(NAMES, got, again):
        assert torch.equal(g[POOL:], g[:B - POOL]), f"{name}: rows b and b + 11 hold the same inputs but differ"
        assert torch.equal(g, a), f"{name}: two identical calls differ"
    fails = []
    _hold(f"{B} poses, first {POOL} rows:", [g[:POOL] for g in got], edge_case["r32"], edge_case["r64"], fails)
    assert not fails, "\n".join(fails)


def test_gpu_smplh_backward_after_an_unrelated_forward(built_lib, cuda_dev, edge_case):
    m, body_only = edge_case["model"], edge_case["body_only"]
    want = _edge_run(edge_case, 65, cuda_dev)
    other = _dev(cuda_dev, *_inputs(40, 99, not body_only, False)[:2])
    with torch.no_grad():
        m(global_orient=other[0][:, :1], body_pose=other[0][:, 1:22], betas=other[1],
          **({} if not body_only else dict(left_hand_pose=other[0][:, 22:37], right_hand_pose=other[0][:, 37:])))
    got = _edge_run(edge_case, 65, cuda_dev)
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g, w)


def test_gpu_smplh_backward_paths_keep_their_workspaces_apart(built_lib, cuda_dev):
    """One handle with BOTH paths reserved (two workspaces of one type, BodyGradWorkspace in csrc/abi_util.h): folded, full, folded again at
    B = max_batch = 3 from axis-angle poses, so each path's own rotation-gradient scratch is in play.  Each result is byte for byte what
    the same call gives on a fresh handle that reserved that path alone."""
    c, B = _asset(), 3
    ins = {body_only: _dev(cuda_dev, *_inputs(B, 81 + body_only, body_only, True)) for body_only in (True, False)}
    both = _model(c, B, cuda_dev)
    alone = {True: _model(c, B, cuda_dev, "folded"), False: _model(c, B, cuda_dev, "full")}
    for step, body_only in enumerate((True, False, True)):
        got = _backward(both, *ins[body_only], body_only, True)
        want = _backward(alone[body_only], *ins[body_only], body_only, True)
        torch.cuda.synchronize()
        for name, g, w in zip(NAMES, got, want):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32)), f"call {step} ({'folded' if body_only else 'full'}) {name}"
    for m in (both, *alone.values()):
        m.close()


# ------------------------------------------------------------------------------------------------ 4. NULL arms, guard bands, refusals
@pytest.mark.parametrize("body_only", [True, False], ids=["folded", "full"])
def test_gpu_smplh_backward_null_arms_and_guard_bands(built_lib, cuda_dev, parity_model, body_only):
    B, m, nj = 5, parity_model, 22 if body_only else 52
    pose, betas, transl, gV, gJ = _dev(cuda_dev, *_inputs(B, 111, body_only, False))
    full = _backward(m, pose, betas, transl, gV, gJ, body_only, False)
    # each output absent in turn: the others are the same bits, and nothing outside a window is written
    for skip in range(3):
        outs = [G.guarded(B, n, device=cuda_dev) for n in (nj * 9, 10, 3)]
        args = [None if k == skip else outs[k][0] for k in range(3)]
        m._backward(pose, False, betas, transl, body_only, B, gV, gJ, *args)
        torch.cuda.synchronize()
        for k in range(3):
            outs[k][1]()
            w = outs[k][0].contiguous().view(torch.int32)
            if k == skip:
                assert (w == G.CANARY[torch.float32]).all()
            else:
                assert not (w == G.CANARY[torch.float32]).any(), "an output element was left unwritten"
                assert torch.equal(outs[k][0].reshape(full[k].shape), full[k])
    # each optional input absent in turn: zeros in its place give the same bits (transl does not enter the gradient at all)
    zeros = dict(betas=torch.zeros_like(betas), gV=torch.zeros_like(gV), gJ=torch.zeros_like(gJ))
    for name in ("betas", "transl", "gV", "gJ"):
        kw = dict(betas=betas, transl=transl, gV=gV, gJ=gJ)
        kw[name] = None
        got = _backward(m, pose, kw["betas"], kw["transl"], kw["gV"], kw["gJ"], body_only, False)
        kw[name] = zeros.get(name, transl)
        want = _backward(m, pose, kw["betas"], kw["transl"], kw["gV"], kw["gJ"], body_only, False)
        torch.cuda.synchronize()
        for g, w in zip(got, want):
            assert torch.equal(g, w), name


def test_gpu_smplh_backward_refusals(built_lib, cuda_dev):
    from tokenhmr_amd import _cabi
    from tokenhmr_amd.smplh import SMPLHLayer
    B = 4
    m = SMPLHLayer(_asset(), max_batch=B, device=cuda_dev)
    m._handle()
    lib = m.lib
    pose, betas, transl, gV, gJ = _dev(cuda_dev, *_inputs(B, 121, True, False))
    outs = [G.guarded(B, n, device=cuda_dev) for n in (22 * 9, 10, 3)]
    st = C.c_void_p(torch.cuda.current_stream(cuda_dev).cuda_stream)

    def refused(what, *args):
        rc = lib.thmr_smplh_backward(*args, st)
        msg = (lib.thmr_last_error(None) or b"").decode()
        assert rc == _cabi.ERR_INVALID and what in msg, (rc, msg)

    P, Bt, T, V, J = _p(pose), _p(betas), _p(transl), _p(gV), _p(gJ)
    GP, GB, GT = (_p(o[0]) for o in outs)
    refused("folded path was not reserved", m.h, P, 0, Bt, T, 1, B, V, J, GP, GB, GT)
    assert lib.thmr_smplh_grad_reserve(m.h, 1) == 0
    assert lib.thmr_smplh_grad_reserve(m.h, 1) == 0                        # idempotent
    refused("full path was not reserved", m.h, P, 0, Bt, T, 0, B, V, J, GP, GB, GT)
    refused("null handle", None, P, 0, Bt, T, 1, B, V, J, GP, GB, GT)
    refused("null handle or pose", m.h, None, 0, Bt, T, 1, B, V, J, GP, GB, GT)
    refused("both null", m.h, P, 0, Bt, T, 1, B, None, None, GP, GB, GT)
    refused("all null", m.h, P, 0, Bt, T, 1, B, V, J, None, None, None)
    refused("max_batch", m.h, P, 0, Bt, T, 1, 0, V, J, GP, GB, GT)
    refused("max_batch", m.h, P, 0, Bt, T, 1, B + 1, V, J, GP, GB, GT)
    refused("0 or 1", m.h, P, 2, Bt, T, 1, B, V, J, GP, GB, GT)
    refused("0 or 1", m.h, P, 0, Bt, T, 2, B, V, J, GP, GB, GT)
    assert lib.thmr_smplh_grad_reserve(None, 1) == _cabi.ERR_INVALID
    for paths in (0, 4, -1):
        assert lib.thmr_smplh_grad_reserve(m.h, paths) == _cabi.ERR_INVALID
    torch.cuda.synchronize()
    for w, check in outs:                                                  # nothing was launched: every canary is still there
        check()
        assert (w.contiguous().view(torch.int32) == G.CANARY[torch.float32]).all()
    m.close()


# ------------------------------------------------------------------------------------------------ 5. the autograd surface
def test_gpu_smplhlayer_autograd(built_lib, cuda_dev):
    from tokenhmr_amd.smplh import SMPLHLayer
    c, B = _asset(), 4
    pose, betas, transl, gV, gJ = _inputs(B, 131, True, False)
    bp = pose[:, 1:]
    eye = torch.eye(3).expand(B, 1, 3, 3)

    def truth(dtype):
        s = SB.to64(c) if dtype == torch.float64 else c
        x = bp.to(dtype).clone().requires_grad_(True)
        v, j = HB.smplh_forward_generic(HB.with_identity_hands(torch.cat([eye.to(dtype), x], 1)), torch.zeros(B, 10, dtype=dtype), s, None, dtype)
        return torch.autograd.grad((v * gV.to(dtype)).sum() + (j * gJ.to(dtype)).sum(), x)[0]

    never = SMPLHLayer(c, max_batch=B, device=cuda_dev)
    m = SMPLHLayer(c, max_batch=B, device=cuda_dev)
    x = bp.to(cuda_dev).requires_grad_(True)
    out = m(body_pose=x)
    plain = m(body_pose=x.detach())
    ref = never(body_pose=x.detach())
    assert out.vertices.grad_fn is not None and out.joints.grad_fn is not None
    assert plain.vertices.grad_fn is None and not plain.vertices.requires_grad and ref.joints.grad_fn is None
    for a in ("vertices", "joints"):
        assert torch.equal(getattr(out, a).detach(), getattr(plain, a)) and torch.equal(getattr(plain, a), getattr(ref, a)), a
    assert never._grad_paths == 0 and m._grad_paths == 1 and m.folded_calls == 2
    loss = (out.vertices * gV.to(cuda_dev)).sum() + (out.joints * gJ.to(cuda_dev)).sum()
    loss.backward()
    ok, line = SB.check("SMPLHLayer(body_pose=R.requires_grad_()) .grad:", x.grad.cpu(), truth(torch.float32), truth(torch.float64), MULT)
    with pytest.raises(RuntimeError, match="second time|already been freed"):
        loss.backward()
    with torch.no_grad():
        assert m(body_pose=x).vertices.grad_fn is None
    torch.cuda.synchronize()
    never.close()
    m.close()
    assert ok, line


def test_gpu_smplh_autograd_through_the_pca_hands(built_lib, cuda_dev):
    from tokenhmr_amd.smplh import SMPLH
    c, B = _asset(), 3
    rng = np.random.default_rng(141)
    aa = torch.from_numpy(0.5 * rng.standard_normal((B, 63))).float()
    lh, rh = (torch.from_numpy(rng.standard_normal((B, 6))).float() for _ in range(2))
    betas = torch.from_numpy(rng.standard_normal((B, 10))).float()
    gV = torch.from_numpy(rng.standard_normal((B, 6890, 3))).float()

    def truth(dtype):
        s = SB.to64(c) if dtype == torch.float64 else c
        a, l, r, bt = (t.to(dtype).clone().requires_grad_(True) for t in (aa, lh, rh, betas))
        mean = torch.cat([torch.zeros(66, dtype=dtype), s["hands_meanl"].reshape(45).to(dtype), s["hands_meanr"].reshape(45).to(dtype)])
        full = torch.cat([torch.zeros(B, 3, dtype=dtype), a, l @ s["hands_componentsl"][:6].to(dtype), r @ s["hands_componentsr"][:6].to(dtype)],
                         dim=1) + mean
        v, _ = HB.smplh_forward_generic(HB.batch_rodrigues_generic(full.reshape(-1, 3)).view(B, 52, 3, 3), bt, s, None, dtype)
        return torch.autograd.grad((v * gV.to(dtype)).sum(), (a, l, r, bt))

    r64, r32 = truth(torch.float64), truth(torch.float32)
    m = SMPLH(c, max_batch=B, device=cuda_dev)
    a, l, r, bt = (t.to(cuda_dev).requires_grad_(True) for t in (aa, lh, rh, betas))
    out = m(betas=bt, body_pose=a, left_hand_pose=l, right_hand_pose=r)
    (out.vertices * gV.to(cuda_dev)).sum().backward()
    torch.cuda.synchronize()
    fails = []
    for name, g, x32, x64 in zip(("body_pose", "left_hand_pose (PCA)", "right_hand_pose (PCA)", "betas"), (a.grad, l.grad, r.grad, bt.grad), r32, r64):
        ok, line = SB.check(f"SMPLH autograd, grad {name}:", g.cpu(), x32, x64, MULT)
        if not ok:
            fails.append(line)
    assert m._grad_paths == 2 and m.full_calls == 1
    m.close()
    assert not fails, "\n".join(fails)


def test_gpu_smplh_forward_backward_captured(built_lib, cuda_dev):
    """After enable_grad(): forward + backward captured in one graph on one stream; replayed on new input values it equals eager."""
    B = 9
    m = _model(_asset(), B, cuda_dev, "folded")
    ins = [_dev(cuda_dev, *_inputs(B, 150 + k, True, True)) for k in range(3)]
    pose, betas, transl, gV, gJ = (t.clone() for t in ins[0])
    verts, joints = torch.empty(B, 6890, 3, device=cuda_dev), torch.empty(B, 73, 3, device=cuda_dev)
    gp, gb, gt = torch.empty_like(pose), torch.empty_like(betas), torch.empty_like(transl)

    def run(stream):
        st = C.c_void_p(stream.cuda_stream)
        m._check(m.lib.thmr_smplh_forward(m.h, _p(pose), 1, _p(betas), _p(transl), 1, B, _p(verts), _p(joints), st), "thmr_smplh_forward")
        m._check(m.lib.thmr_smplh_backward(m.h, _p(pose), 1, _p(betas), _p(transl), 1, B, _p(gV), _p(gJ), _p(gp), _p(gb), _p(gt), st),
                 "thmr_smplh_backward")

    eager = []
    for k in range(3):
        for dst, src in zip((pose, betas, transl, gV, gJ), ins[k]):
            dst.copy_(src)
        run(torch.cuda.current_stream(cuda_dev))
        torch.cuda.synchronize()
        eager.append([t.clone() for t in (verts, joints, gp, gb, gt)])
    assert not torch.equal(eager[1][2], eager[2][2])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(torch.cuda.current_stream(cuda_dev))
    for k in (1, 2):
        for dst, src in zip((pose, betas, transl, gV, gJ), ins[k]):
            dst.copy_(src)
        for t in (verts, joints, gp, gb, gt):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for t, e in zip((verts, joints, gp, gb, gt), eager[k]):
            assert torch.equal(t, e), k
    del graph
    m.close()
