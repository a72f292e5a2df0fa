"""SMPL-H on the device (csrc/body_model.hip, tokenhmr_amd/smplh.py) and the tokenizer's mesh evaluation (thmr_op_mean_row_dist,
tokenhmr_amd/tokenizer_eval.py).

Bound of the mesh tests: max(2e-6 m, 2 x d_ref) against the independent fp64 derivation (a) of tests/smplh_oracle.py, where d_ref is
the distance of smplx's formulation in torch fp32 on the CPU (b) to (a) ON THE SAME INPUTS, computed here — the device may be twice as
far from the truth as the reference's own arithmetic, and never needs to be closer than the 2e-6 m tests/test_smpl_bounds.py allows
the 24-joint kernels.  On this module's own pools (seeds 21 and 22) (b) is 6.1e-7 to 7.6e-7 m on vertices and 4.9e-7 to 6.4e-7 m on joints from
(a) for the 52-joint pool, 5.9e-7 to 6.2e-7 m and 3.6e-7 to 3.8e-7 m for the body-only pool (two hosts), so every bound here is the
2e-6 m floor; the device measured 5.7e-7 / 3.5e-7 m (full) and 4.5e-7 / 2.0e-7 m (folded) at most, the axis-angle cases 9.8e-7 / 5.7e-7 m.  The axis-angle cases hand
(a) the device's OWN fp32 rotation matrices (thmr_op_aa_to_rotmat, the kernel thmr_smplh_forward(pose2rot=1) runs), so the same bound
applies to them without an allowance for Rodrigues' formula.

The references are computed ONCE per module for a pool of 11 distinct poses; item b of a batch is pose b % 11 (11 is coprime to the
1 / 2 / 4 / 8 poses a skin workgroup walks, so an item that received a neighbour's bone matrices or vertices cannot go unnoticed).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

import smplh_oracle as S
import tokenizer_rt_oracle as T
from oracle import tokenhmr_oracle as O
from oracle.gen_golden_encode import make_pose
from tokenhmr_amd import _cabi
from tokenhmr_amd import weights as W
from tokenhmr_amd.config import HMRConfig, RELEASE, SMPL_EXTRA_VERTS
from tokenhmr_amd.smpl_assets import make_synthetic_smplh
from tokenhmr_amd.smplh import SMPLH, SMPLHLayer
from tokenhmr_amd.tokenizer_eval import TokenizerEvaluator, mean_row_dist, run_eval

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_golden_tokenizer_eval as GE          # noqa: E402

pytestmark = pytest.mark.gpu
FLOOR_M = 2e-6
POOL = 11

def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@pytest.fixture(scope="module")
def consts():
    return make_synthetic_smplh(0)


@pytest.fixture(scope="module")
def pool(consts):
    """Inputs and both references, once: 'full' = 52 random rotations, 'body' = random root + body, identity hands; random betas."""
    out = {}
    for name, seed in (("full", 21), ("body", 22)):
        R = S.random_rotations(POOL * 52, seed=seed).reshape(POOL, 52, 3, 3)
        if name == "body":
            R[:, 22:] = np.eye(3)
        betas = np.random.default_rng(seed + 100).standard_normal((POOL, 10))
        R32, b32 = torch.from_numpy(R).float(), torch.from_numpy(betas).float()
        v64, j64 = S.smplh_forward_independent(R32.double().numpy(), b32.double().numpy(), consts)
        v32, j32 = S.smplh_forward_smplx32(R32, b32, consts)
        dv = np.abs(v32.double().numpy() - v64).max(axis=(1, 2))
        dj = np.abs(j32.double().numpy() - j64).max(axis=(1, 2))
        print(f"reference arithmetic (smplx formulation, torch fp32, CPU) vs fp64, {name} pool: verts {dv.max():.2e} m, joints {dj.max():.2e} m")
        out[name] = dict(R=R32, betas=b32, v64=v64, j64=j64, tol_v=max(FLOOR_M, 2 * dv.max()), tol_j=max(FLOOR_M, 2 * dj.max()))
    return out


_layers = {}


@pytest.fixture(scope="module")
def layer_of(built_lib, cuda_dev, consts):
    def get(max_batch, cls=SMPLHLayer, **kw):
        key = (max_batch, cls.__name__, tuple(sorted(kw.items())))
        if key not in _layers:
            _layers[key] = cls(consts, max_batch=max_batch, device=cuda_dev, **kw)
        return _layers[key]
    yield get
    for m in _layers.values():
        m.close()
    _layers.clear()


def _dist(out, ref, sel):
    v = np.abs(out.vertices.cpu().double().numpy() - ref["v64"][sel]).max()
    j = np.abs(out.joints.cpu().double().numpy() - ref["j64"][sel]).max()
    return v, j


def _picked_equal(out):
    return torch.equal(out.joints[:, 52:], out.vertices[:, SMPL_EXTRA_VERTS])


# poses per skin workgroup (body_model.hip smplh_poses_per_workgroup): 1 below 64 poses, 2 from 64, 4 from 128, 8 from 256
BATCHES = [(1, 256, "one pose"), (5, 5, "5 = max_batch"), (5, 256, "5 of 256"), (63, 256, "63: last batch of 1 pose per workgroup"),
           (64, 256, "64: first of 2 per workgroup"), (127, 256, "127: last of 2, ragged group"), (128, 256, "128: first of 4"),
           (255, 256, "255: last of 4, ragged group"), (256, 256, "256 = max_batch: first of 8")]


@pytest.mark.parametrize("B,max_batch,name", BATCHES, ids=[b[2] for b in BATCHES])
def test_full_and_folded_paths_match_independent_derivation(layer_of, pool, cuda_dev, B, max_batch, name):
    m = layer_of(max_batch)
    sel = np.arange(B) % POOL
    full, body = pool["full"], pool["body"]
    o = m(betas=full["betas"][sel], global_orient=full["R"][sel, :1], body_pose=full["R"][sel, 1:22],
          left_hand_pose=full["R"][sel, 22:37], right_hand_pose=full["R"][sel, 37:])
    dv, dj = _dist(o, full, sel)
    print(f"full 52-joint path, {B} poses: verts {dv:.2e} m (bound {full['tol_v']:.2e}), joints {dj:.2e} m (bound {full['tol_j']:.2e})")
    assert o.vertices.shape == (B, 6890, 3) and o.joints.shape == (B, 73, 3) and o.full_pose.shape == (B, 52, 3, 3)
    assert dv <= full["tol_v"] and dj <= full["tol_j"] and _picked_equal(o)
    before = (m.folded_calls, m.full_calls)
    f = m(betas=body["betas"][sel], global_orient=body["R"][sel, :1], body_pose=body["R"][sel, 1:22])
    assert (m.folded_calls, m.full_calls) == (before[0] + 1, before[1])
    dv, dj = _dist(f, body, sel)
    print(f"folded 22-joint path, {B} poses: verts {dv:.2e} m (bound {body['tol_v']:.2e}), joints {dj:.2e} m (bound {body['tol_j']:.2e})")
    assert dv <= body["tol_v"] and dj <= body["tol_j"] and _picked_equal(f)
    assert f.full_pose.shape == (B, 52, 3, 3) and torch.equal(f.full_pose[:, 22:], torch.eye(3, device=cuda_dev).expand(B, 30, 3, 3))


def test_full_and_folded_paths_agree_on_identity_hands(layer_of, pool, cuda_dev):
    """The same call down both paths; which one ran shows in the layer's counters, not in timing."""
    m = layer_of(256)
    body = pool["body"]
    B = 7
    sel = np.arange(B)
    eye = torch.eye(3).expand(B, 15, 3, 3)
    n_fold, n_full = m.folded_calls, m.full_calls
    f = m(betas=body["betas"][sel], global_orient=body["R"][sel, :1], body_pose=body["R"][sel, 1:22])
    assert (m.folded_calls, m.full_calls) == (n_fold + 1, n_full)
    g = m(betas=body["betas"][sel], global_orient=body["R"][sel, :1], body_pose=body["R"][sel, 1:22], left_hand_pose=eye, right_hand_pose=eye)
    assert (m.folded_calls, m.full_calls) == (n_fold + 1, n_full + 1)
    dv, dj = (f.vertices - g.vertices).abs().max().item(), (f.joints - g.joints).abs().max().item()
    gv, gj = _dist(g, body, sel)
    print(f"folded vs full on identity hands: verts {dv:.2e} m, joints {dj:.2e} m; full vs fp64 {gv:.2e} / {gj:.2e} m")
    assert dv <= body["tol_v"] and dj <= body["tol_j"] and gv <= body["tol_v"] and gj <= body["tol_j"]
    # the tokenizer's own call: body_pose alone (identity root, zero betas)
    t = m(body_pose=body["R"][sel, 1:22])
    R0 = body["R"][sel].clone()
    R0[:, 0] = torch.eye(3)
    v64, j64 = S.smplh_forward_independent(R0.double().numpy(), np.zeros((B, 10)), make_synthetic_smplh(0))
    assert np.abs(t.vertices.cpu().double().numpy() - v64).max() <= body["tol_v"]
    assert np.abs(t.joints.cpu().double().numpy() - j64).max() <= body["tol_j"]
    assert torch.equal(t.betas, torch.zeros(B, 10, device=cuda_dev))


@pytest.mark.parametrize("folded", [False, True], ids=["full", "folded"])
def test_transl_is_the_exact_fp32_sum(layer_of, pool, cuda_dev, folded):
    m = layer_of(256)
    B = 66                                     # two poses per workgroup
    sel = np.arange(B) % POOL
    src = pool["body" if folded else "full"]
    kw = dict(betas=src["betas"][sel], global_orient=src["R"][sel, :1], body_pose=src["R"][sel, 1:22])
    if not folded:
        kw.update(left_hand_pose=src["R"][sel, 22:37], right_hand_pose=src["R"][sel, 37:])
    t = torch.randn(B, 3, generator=torch.Generator().manual_seed(9)) * 3
    a, b = m(**kw), m(transl=t, **kw)
    assert torch.equal(b.vertices, a.vertices + t.to(cuda_dev)[:, None]) and torch.equal(b.joints, a.joints + t.to(cuda_dev)[:, None])
    assert _picked_equal(b) and torch.equal(b.transl, t.to(cuda_dev))


def test_smplh_axis_angle(layer_of, consts, cuda_dev):
    B = 4
    g = torch.Generator().manual_seed(5)
    body, orient, betas = 0.5 * torch.randn(B, 63, generator=g), 0.5 * torch.randn(B, 3, generator=g), torch.randn(B, 10, generator=g)
    hl, hr = consts["hands_meanl"], consts["hands_meanr"]
    relaxed, flat45 = layer_of(8, SMPLH), layer_of(8, SMPLH, use_pca=False, flat_hand_mean=True)
    # zero PCA coefficients + the hand mean == the full path fed the hand mean: the same full pose, the same kernels, the same bits
    a = relaxed(betas=betas, global_orient=orient, body_pose=body)
    b = flat45(betas=betas, global_orient=orient, body_pose=body, left_hand_pose=hl.expand(B, 45), right_hand_pose=hr.expand(B, 45))
    assert a.full_pose.shape == (B, 156) and torch.equal(a.full_pose, b.full_pose)
    assert torch.equal(a.vertices, b.vertices) and torch.equal(a.joints, b.joints)
    assert relaxed.full_calls >= 1 and relaxed.folded_calls == 0
    # PCA coefficients are expanded by the first num_pca_comps components
    coef = torch.randn(B, 6, generator=g)
    c = relaxed(body_pose=body, left_hand_pose=coef, right_hand_pose=-coef)
    want = torch.cat([torch.zeros(B, 3), body, coef @ consts["hands_componentsl"][:6] + hl, -coef @ consts["hands_componentsr"][:6] + hr], 1)
    assert (c.full_pose.cpu() - want).abs().max() < 1e-6

    lib = relaxed.lib

    def device_rotmat(aa):
        """(B,n*3) axis-angle -> (B,n,3,3) by the device's Rodrigues kernel."""
        aa = aa.to(cuda_dev).float().contiguous()
        R = torch.empty(aa.numel() // 3, 3, 3, device=cuda_dev)
        _cabi.check(lib.thmr_op_aa_to_rotmat(_p(aa), _p(R), aa.numel() // 3, None), lib=lib)
        return R.view(aa.shape[0], -1, 3, 3)

    def against_fp64(out, bt, what):
        R = device_rotmat(out.full_pose).cpu()
        v64, j64 = S.smplh_forward_independent(R.double().numpy(), bt.double().numpy(), consts)
        v32, j32 = S.smplh_forward_smplx32(R, bt, consts)
        tv = max(FLOOR_M, 2 * np.abs(v32.double().numpy() - v64).max())
        tj = max(FLOOR_M, 2 * np.abs(j32.double().numpy() - j64).max())
        dv, dj = np.abs(out.vertices.cpu().double().numpy() - v64).max(), np.abs(out.joints.cpu().double().numpy() - j64).max()
        print(f"SMPLH {what}: verts {dv:.2e} m (bound {tv:.2e}), joints {dj:.2e} m (bound {tj:.2e})")
        assert dv <= tv and dj <= tj
        return tv, tj

    # the Rodrigues kernel itself against the closed form in fp64: a few ulp of 1 per entry
    dR = np.abs(device_rotmat(a.full_pose).cpu().double().numpy().reshape(-1, 3, 3) - S.batch_rodrigues64(a.full_pose.cpu().double().numpy().reshape(-1, 3))).max()
    print(f"device Rodrigues vs fp64 closed form: {dR:.2e}")
    assert dR < 1e-6
    against_fp64(a, betas, "zero PCA coefficients, relaxed hand mean")
    # use_pca=False: 45 values per hand, the mean added on top
    nopca = layer_of(8, SMPLH, use_pca=False)
    lh, rh = 0.3 * torch.randn(B, 45, generator=g), 0.3 * torch.randn(B, 45, generator=g)
    d = nopca(betas=betas, global_orient=orient, body_pose=body, left_hand_pose=lh, right_hand_pose=rh)
    assert (d.full_pose.cpu() - torch.cat([orient, body, lh + hl, rh + hr], 1)).abs().max() < 1e-6
    against_fp64(d, betas, "use_pca=False")
    # flat_hand_mean=True and no hands: SMPLHLayer's mesh on the same (device-made) rotation matrices — the full path against the folded one
    e = flat45(body_pose=body)
    tv, tj = against_fp64(e, torch.zeros(B, 10), "flat_hand_mean=True, body pose only")
    assert torch.equal(device_rotmat(e.full_pose)[:, 22:], torch.eye(3, device=cuda_dev).expand(B, 30, 3, 3))      # Rodrigues of 0 is exactly I
    lay = layer_of(8)(body_pose=device_rotmat(body))
    dv, dj = (e.vertices - lay.vertices).abs().max().item(), (e.joints - lay.joints).abs().max().item()
    print(f"SMPLH(flat_hand_mean=True) vs SMPLHLayer on the same rotation matrices: verts {dv:.2e} m, joints {dj:.2e} m (bounds {tv:.2e} / {tj:.2e})")
    assert dv <= tv and dj <= tj


# ------------------------------------------------------------------------------------------------ thmr_op_mean_row_dist
def _mrd_case(name):
    if name == "mesh fixture":
        seed, shape, _ = GE.CASES["mesh"]
        return (*GE.eval_inputs(seed, shape), 0, None)
    g = torch.Generator().manual_seed(77)
    shape, lo, hi = {"one row": ((1, 1, 3), 0, None), "one item": ((1, 300, 3), 0, None), "rows 1..21 of 73": ((5, 73, 3), 1, 22),
                     "63 rows x 9 items": ((9, 63, 3), 0, None), "64 x 6890": ((64, 6890, 3), 0, None)}[name]
    a = torch.randn(*shape, generator=g)
    return a, a + 0.05 * torch.randn(*shape, generator=g), lo, hi


@pytest.mark.parametrize("name", ["one row", "one item", "mesh fixture", "rows 1..21 of 73", "63 rows x 9 items", "64 x 6890"])
def test_mean_row_dist_against_fp64(built_lib, cuda_dev, name):
    """Relative error <= 1e-5: the worst case of a fixed-order fp32 sum of this length (at most 441k terms, 7 per lane, then trees),
    not a measurement."""
    a, b, lo, hi = _mrd_case(name)
    ref = S.mean_row_dist64(a.numpy(), b.numpy(), lo, hi)
    ad, bd = a.to(cuda_dev), b.to(cuda_dev)
    r1 = mean_row_dist(ad, bd, lo, hi)
    r2 = mean_row_dist(ad, bd, lo, hi)
    assert r1.dim() == 0 and r1.is_cuda and r1.dtype == torch.float32
    rel = abs(float(r1) - ref) / ref
    msg = f"mean_row_dist [{name}]: device {float(r1):.8f}, fp64 {ref:.10f}, relative error {rel:.1e}"
    if name == "mesh fixture":
        rec = float(np.load(os.path.join(GOLDEN_DIR, "tokenizer_eval.npz"))["mesh.value"])
        msg += f"; the reference's recorded torch-fp32 result {rec:.8f}: relative error {abs(rec - ref) / ref:.1e}"
    print(msg)
    assert rel <= 1e-5
    assert torch.equal(r1, r2)                                           # two runs are bit-equal
    assert float(mean_row_dist(ad, ad.clone(), lo, hi)) == 0.0           # equal inputs give exactly 0
    if name == "rows 1..21 of 73":                                       # rows outside the range do not enter
        a2 = a.clone()
        a2[:, 0], a2[:, 22:] = 1e6, -1e6
        assert torch.equal(mean_row_dist(a2.to(cuda_dev), bd, lo, hi), r1)


def test_mean_row_dist_refusals(built_lib, cuda_dev):
    a = torch.zeros(2, 73, 3, device=cuda_dev)
    out, ws = torch.zeros((), device=cuda_dev), torch.zeros(_cabi.MEAN_ROW_DIST_WS, device=cuda_dev)
    call = lambda *x: built_lib.thmr_op_mean_row_dist(*x, None)     # noqa: E731
    assert call(_p(a), _p(a), 73, 1, 22, 2, _p(out), _p(ws)) == 0
    for bad in ((None, _p(a), 73, 1, 22, 2, _p(out), _p(ws)), (_p(a), _p(a), 73, 1, 22, 2, None, _p(ws)), (_p(a), _p(a), 73, 1, 22, 2, _p(out), None),
                (_p(a), _p(a), 73, 1, 22, 0, _p(out), _p(ws)), (_p(a), _p(a), 73, 22, 22, 2, _p(out), _p(ws)),
                (_p(a), _p(a), 73, -1, 22, 2, _p(out), _p(ws)), (_p(a), _p(a), 73, 1, 74, 2, _p(out), _p(ws)),
                (_p(a), _p(a), 1 << 29, 0, 1, 2, _p(out), _p(ws))):
        assert call(*bad) != 0
        assert b"mean_row_dist" in built_lib.thmr_last_error(None)
    with pytest.raises(ValueError):
        mean_row_dist(a, a[:, :70])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ C ABI
def _desc(c, **over):
    keys = ["v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights"]
    ts = {k: c[k].float().contiguous() for k in keys}
    ts.update({k: c[k].to(torch.int32).contiguous() for k in ("parents", "extra_verts")})
    ts.update(over)
    d = _cabi.SmplhDesc(**{k: (v.data_ptr() if v is not None else None) for k, v in ts.items()}, on_device=0)
    return d, ts


def test_c_abi_refusals(built_lib, cuda_dev, consts):
    lib = built_lib

    def create(max_batch=4, **over):
        d, keep = _desc(consts, **over)
        h = C.c_void_p(0)
        rc = lib.thmr_smplh_create(C.byref(d), max_batch, cuda_dev.index or 0, C.byref(h))
        return rc, h, lib.thmr_last_error(None).decode()

    for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights", "parents", "extra_verts"):
        rc, h, msg = create(**{k: None})
        assert rc != 0 and not h.value and "null field" in msg
    par = consts["parents"].to(torch.int32).clone()
    par[0] = 0
    rc, h, msg = create(parents=par)
    assert rc != 0 and not h.value and "parents[0]" in msg
    for i, v in ((30, 30), (30, 45), (7, -1)):                       # not below its index / no second root
        par = consts["parents"].to(torch.int32).clone()
        par[i] = v
        rc, h, msg = create(parents=par)
        assert rc != 0 and not h.value and f"parents[{i}]" in msg
    for v in (6890, -1):
        ev = consts["extra_verts"].to(torch.int32).clone()
        ev[20] = v
        rc, h, msg = create(extra_verts=ev)
        assert rc != 0 and not h.value and "extra_verts[20]" in msg
    assert create(max_batch=0)[0] != 0
    rc, h, _ = create(max_batch=4)
    assert rc == 0 and h.value
    pose = torch.eye(3, device=cuda_dev).expand(5, 22, 3, 3).contiguous()
    verts = torch.zeros(5, 6890, 3, device=cuda_dev)
    fwd = lambda p, p2r, bo, B, v: lib.thmr_smplh_forward(h, p, p2r, None, None, bo, B, v, None, None)     # noqa: E731
    assert fwd(_p(pose), 0, 1, 4, _p(verts)) == 0                    # betas, transl, joints all NULL
    for bad in ((_p(pose), 0, 1, 0, _p(verts)), (_p(pose), 0, 1, 5, _p(verts)), (None, 0, 1, 1, _p(verts)), (_p(pose), 0, 1, 1, None),
                (_p(pose), 2, 1, 1, _p(verts)), (_p(pose), 0, 2, 1, _p(verts))):
        assert fwd(*bad) != 0
        assert "smplh_forward" in lib.thmr_last_error(None).decode()
    assert lib.thmr_smplh_forward(None, _p(pose), 0, None, None, 1, 1, _p(verts), None, None) != 0
    torch.cuda.synchronize()
    # zero betas, identity pose: the template itself (the blend product adds exact zeros, every bone matrix is the identity up to J - J)
    assert (verts[:4].cpu() - consts["v_template"]).abs().max() < 1e-6
    lib.thmr_smplh_destroy(h)
    lib.thmr_smplh_destroy(None)


# ------------------------------------------------------------------------------------------------ graph capture
def test_forward_and_metrics_replay_bit_equal_from_a_graph(layer_of, pool, cuda_dev):
    """thmr_smplh_forward + the three metrics: one linear chain of launches, no memset, no allocation, nothing to zero between runs."""
    m = layer_of(8)
    lib, h = m.lib, m._handle()
    B = 6
    body = pool["body"]
    pose = body["R"][:B, :22].to(cuda_dev).contiguous()
    gt_rot = body["R"][1:B + 1, 1:22].to(cuda_dev).contiguous()
    gt = m(body_pose=gt_rot)
    gt_v, gt_j = gt.vertices.clone(), gt.joints.clone()
    verts, joints = torch.zeros(B, 6890, 3, device=cuda_dev), torch.zeros(B, 73, 3, device=cuda_dev)
    res, ws = torch.zeros(3, device=cuda_dev), torch.zeros(_cabi.MEAN_ROW_DIST_WS, device=cuda_dev)
    body_rot = pose[:, 1:].contiguous()

    def run(stream):
        st = C.c_void_p(stream.cuda_stream)
        _cabi.check(lib.thmr_smplh_forward(h, _p(pose), 0, None, None, 1, B, _p(verts), _p(joints), st), lib=lib)
        _cabi.check(lib.thmr_op_mean_row_dist(_p(gt_rot), _p(body_rot), 63, 0, 63, B, _p(res[0]), _p(ws), st), lib=lib)
        _cabi.check(lib.thmr_op_mean_row_dist(_p(gt_v), _p(verts), 6890, 0, 6890, B, _p(res[1]), _p(ws), st), lib=lib)
        _cabi.check(lib.thmr_op_mean_row_dist(_p(gt_j), _p(joints), 73, 1, 22, B, _p(res[2]), _p(ws), st), lib=lib)

    run(torch.cuda.current_stream(cuda_dev))
    torch.cuda.synchronize()
    eager = (verts.clone(), joints.clone(), res.clone())
    assert float(res[1]) > 0 and float(res[2]) > 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(torch.cuda.current_stream(cuda_dev))
    for _ in range(2):
        verts.zero_(); joints.zero_(); res.zero_(); ws.fill_(123.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(verts, eager[0]) and torch.equal(joints, eager[1]) and torch.equal(res, eager[2])


# ------------------------------------------------------------------------------------------------ end to end
def test_tokenizer_mesh_keys_and_evaluator(built_lib, cuda_dev, consts):
    from tokenhmr_amd.engine import Engine
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.tokenizer import VanillaTokenizer
    golden = np.load(os.path.join(GOLDEN_DIR, "tokenizer_rt.npz"))
    cfg = HMRConfig(vit_depth=1, dec_depth=1)
    enc, tok = W.make_synthetic_encoder(RELEASE, 0), dict(W.make_synthetic_tokenizer(RELEASE, 0))
    tok["quantizer.codebook"] = T.make_codebook(torch.from_numpy(golden["mu"]), torch.from_numpy(golden["sd"]), golden["factor"][0],
                                                golden["cb_seed"][0])
    eng = Engine(cfg, max_batch=2, device=cuda_dev)
    eng.load_state(W.make_synthetic_state(cfg, 0), dict(tok, **enc))
    eng.load_smpl(make_synthetic_smpl(cfg, 0))
    eng.finalize()
    net = VanillaTokenizer(engine=eng, mesh_inference=True, body_model=consts)
    assert isinstance(net.body_model, SMPLHLayer) and net.body_model.max_batch == 2
    plain = VanillaTokenizer(engine=eng, mesh_inference=True)
    layer = SMPLHLayer(consts, max_batch=4, device=cuda_dev)
    gt_model = SMPLH(consts, max_batch=2, device=cuda_dev)
    ev = TokenizerEvaluator(device=cuda_dev)
    sums = np.zeros(5)
    loader = []
    for B, seed in ((3, 0), (2, 5)):                                   # the fixture's two batches; 3 poses = two chunks of the engine
        pose = make_pose(B, seed).to(cuda_dev)
        out, commit, perp = net(pose)
        assert "pred_body_vertices" not in plain(pose)[0]
        assert {"pred_body_mesh", "pred_body_vertices", "pred_body_joints", "pred_pose_body_aa"} <= set(out)
        assert out["pred_body_vertices"].shape == (B, 6890, 3) and out["pred_body_joints"].shape == (B, 73, 3)
        assert out["pred_body_mesh"].vertices is out["pred_body_vertices"]
        want = layer(body_pose=out["pred_pose_body_rotmat"])
        assert torch.equal(out["pred_body_vertices"], want.vertices) and torch.equal(out["pred_body_joints"], want.joints)
        assert net.body_model.folded_calls > 0 and net.body_model.full_calls == 0
        # ground truth as the dataset makes it: SMPLH (relaxed hands) on the axis-angle pose, the rotation matrices beside it
        aa = 0.4 * torch.randn(B, 63, generator=torch.Generator().manual_seed(seed))
        gt_rot = torch.from_numpy(S.batch_rodrigues64(aa.double().numpy().reshape(-1, 3)).reshape(B, 21, 3, 3)).float()
        gts = [gt_model(body_pose=aa[i:i + 2]) for i in range(0, B, 2)]
        batch = {"gt_pose_body": gt_rot, "pose_body_aa": aa, "body_vertices": torch.cat([g.vertices for g in gts]).cpu(),
                 "body_joints": torch.cat([g.joints for g in gts]).cpu()}
        loader.append(batch)
        out, commit, perp = net(gt_rot)                                # eval_poseVQ.py:88 feeds the matrices
        ev(batch, out, commit, perp)
        sums += [S.mean_row_dist64(gt_rot.reshape(B, 63, 3).numpy(), out["pred_pose_body_rotmat"].reshape(B, 63, 3).cpu().numpy()),
                 S.mean_row_dist64(batch["body_vertices"].numpy(), out["pred_body_vertices"].cpu().numpy()),
                 S.mean_row_dist64(batch["body_joints"].numpy(), out["pred_body_joints"].cpu().numpy(), 1, 22),
                 float(perp), float(commit)]
    m = ev.get_metrics_dict()
    want = sums / 1.0                                                  # the reference's divisor: batch_idx = 1 after two batches
    got = [m["val/curr_pose_recons"], m["val/curr_mesh_recons"] / 1000, m["val/curr_jnt_recons"] / 1000, m["val/curr_perplexity"], m["val/curr_commit"]]
    print("TokenizerEvaluator over two batches:", {k: f"{v:.6f}" for k, v in m.items()})
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-5 * abs(w)
    assert m["curr_score"] == pytest.approx(m["val/curr_jnt_recons"] + m["val/curr_mesh_recons"])
    # the relaxed-hand ground truth against the flat-hand prediction: the reference's constant hand term is there
    assert m["val/curr_mesh_recons"] > 0
    # run_eval: the same loop with the ground truth computed on the device from pose_body_aa (the loader's meshes are not read)
    stripped = [{k: v for k, v in b.items() if k in ("gt_pose_body", "pose_body_aa")} for b in loader]
    m2 = run_eval(net, stripped, body_model_gt=gt_model)
    for k in m:
        assert abs(m2[k] - m[k]) <= 1e-5 * abs(m[k]), k
    m3 = run_eval(net, loader, mean="batches")
    assert m3["curr_score"] == pytest.approx(m["curr_score"] / 2, rel=1e-5)
    with pytest.raises(ValueError, match="batch_idx"):
        run_eval(net, loader[:1])
    eng.status()
    eng.close()
