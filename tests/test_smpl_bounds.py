"""The SMPL boundary.  smplx==0.1.28 is un-vendored and not installable here, so this stage has no
reference-produced golden ("parity unpinned").  Three layers bound it instead:
  1. an INDEPENDENT fp64 derivation from the SMPL paper (oracle/lbs_independent.py: explicit ancestor paths, explicit 4x4
     inverses of the rest chain, un-precomputed joints) that shares nothing with the oracle's smplx restatement or body_model.hip —
     oracle (CPU) and HIP (GPU) must match it to 2e-6 m on random poses and shapes;
  2. the reference's OWN wrapper smpl_wrapper.py:27-41 (joint_map, update_hips, extra joints) executed in place over a
     stand-in lbs == the oracle bit for bit (pins the wrapper, not lbs);
  3. the staged pin: tests/golden/smplx_lbs.npz, written by oracle/gen_golden_smplx.py the day a smplx wheel exists — the
     tests at the bottom hold the oracle and the kernels to it and SKIP until then.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

TOL_M = 2e-6     # metres: fp32 path vs fp64 independent derivation (measured 7e-7 on |v| ~ 2 m)


def _case(B, seed, hips=False):
    from oracle.lbs_independent import random_rotations
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    smpl = make_synthetic_smpl(seed=0)
    smpl["update_hips"] = hips
    R = torch.from_numpy(random_rotations(B * 24, seed=seed).reshape(B, 24, 3, 3)).float()
    betas = torch.from_numpy(np.random.default_rng(seed + 1).standard_normal((B, 10))).float()
    return smpl, R, betas


@pytest.mark.parametrize("hips", [False, True])
def test_oracle_matches_independent_derivation(hips):
    from oracle import tokenhmr_oracle as O
    from oracle.lbs_independent import smpl_forward_independent
    smpl, R, betas = _case(3, 11, hips)
    v64, j64 = smpl_forward_independent(R.double().numpy(), betas.double().numpy(), smpl)
    v, j = O.smpl_forward(R[:, :1], R[:, 1:], betas, smpl)
    dv, dj = np.abs(v.double().numpy() - v64).max(), np.abs(j.double().numpy() - j64).max()
    print(f"oracle vs independent fp64 derivation: verts {dv:.2e} m, joints {dj:.2e} m")
    assert dv < TOL_M and dj < TOL_M


def test_independent_derivation_does_not_depend_on_joint_order():
    """Relabel the 24 joints by a random permutation (children may now precede their parents in the arrays): the
    independent derivation walks ancestor paths, so vertices are unchanged — i.e. it does not silently rely on the
    parents-first order that smplx (and therefore the oracle and body_model.hip) assume."""
    from oracle.lbs_independent import smpl_forward_independent
    smpl, R, betas = _case(2, 5)
    v0, _ = smpl_forward_independent(R.double().numpy(), betas.double().numpy(), smpl)
    # new index i holds old joint perm[i]; the root stays at 0 (posedirs rows are tied to joints 1..23)
    perm = np.concatenate([[0], 1 + np.random.default_rng(0).permutation(23)])
    inv = np.argsort(perm)
    p_old = smpl["parents"].numpy()
    s2 = dict(smpl)
    s2["parents"] = torch.tensor([-1 if p_old[perm[i]] < 0 else inv[p_old[perm[i]]] for i in range(24)], dtype=torch.int32)
    s2["J_regressor"] = smpl["J_regressor"][perm]
    s2["lbs_weights"] = smpl["lbs_weights"][:, perm]
    assert any(s2["parents"][i] > i for i in range(24)), "the permutation should put some child before its parent"
    pd = smpl["posedirs"].reshape(23, 9, -1)
    s2["posedirs"] = pd[perm[1:] - 1].reshape(207, -1)
    s2["joint_map"] = torch.tensor([inv[j] if j < 24 else j for j in smpl["joint_map"].tolist()], dtype=torch.int32)
    v1, _ = smpl_forward_independent(R.double().numpy()[:, perm], betas.double().numpy(), s2)
    assert np.abs(v1 - v0).max() < 1e-12


def test_reference_wrapper_over_standin_lbs_equals_oracle():
    """Runs oracle/gen_golden_smplx.py --plumbing-check: the reference's own smpl_wrapper.SMPL (update_hips False / True)
    imported in place == oracle.smpl_forward bit for bit; also proves the staged-pin script end to end."""
    if not os.path.isdir("/root/reference"):
        pytest.skip("reference tree not present (GPU box)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "gen_golden_smplx.py"), "--plumbing-check"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plumbing OK" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("hips", [False, True])
def test_gpu_lbs_matches_independent_derivation(built_lib, cuda_dev, hips):
    from oracle.lbs_independent import smpl_forward_independent
    from tokenhmr_amd.smpl import SMPL
    smpl, R, betas = _case(5, 21, hips)
    v64, j64 = smpl_forward_independent(R.double().numpy(), betas.double().numpy(), smpl)
    m = SMPL(smpl, max_batch=8, device=cuda_dev)
    o = m(R[:, :1], R[:, 1:], betas, pose2rot=False)
    dv = np.abs(o.vertices.cpu().double().numpy() - v64).max()
    dj = np.abs(o.joints.cpu().double().numpy() - j64).max()
    print(f"body_model.hip vs independent fp64 derivation (update_hips={hips}): verts {dv:.2e} m, joints {dj:.2e} m")
    assert dv < TOL_M and dj < TOL_M


# launch_lbs (tokenhmr_amd/csrc/body_model.hip) walks cg = B / 32 crops per workgroup pass, capped at 8, the bone matrices double-buffered on c & 1, one
# arrival counter per crop group: both sides of every change of cg that has an odd size or a ragged last group
CROP_GROUP_BATCHES = (31, 32, 63,            # cg 1
                      64, 65, 95,            # cg 2: whole, last group of one, last group of one again at 47 whole groups
                      96, 100,               # cg 3: whole, last group of one
                      160, 161,              # cg 5
                      224, 255,              # cg 7: whole, last group of three
                      256, 257)              # cg 8: whole, last group of one
CROP_GROUP_POOL = 11                         # coprime to every cg and to 32: row b holds pool item b % 11


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "update_hips"])
def crop_group_case(request):
    from oracle.lbs_independent import smpl_forward_independent
    smpl, R, betas = _case(CROP_GROUP_POOL, 41, request.param)
    v64, j64 = smpl_forward_independent(R.double().numpy(), betas.double().numpy(), smpl)
    case = dict(smpl=smpl, R=R, betas=betas, v64=v64, j64=j64, model=None)      # model: ONE SMPL(max_batch=257) per update_hips value, made on first GPU use
    yield case
    if case["model"] is not None:
        case["model"].close()


def _crop_group_model(case, dev):
    from tokenhmr_amd.smpl import SMPL
    if case["model"] is None:
        case["model"] = SMPL(case["smpl"], max_batch=257, device=dev)
    return case["model"]


def _crop_group_run(m, case, B):
    sel = torch.arange(B) % CROP_GROUP_POOL
    R, betas = case["R"][sel], case["betas"][sel]
    o = m(R[:, :1], R[:, 1:], betas, pose2rot=False)
    return o.vertices, o.joints


@pytest.mark.gpu
@pytest.mark.parametrize("B", CROP_GROUP_BATCHES)
def test_gpu_lbs_crop_group_edges(built_lib, cuda_dev, crop_group_case, B):
    """The 24-joint path at every crop-group size, odd sizes and ragged last groups included, held to TOL_M against the independent
    fp64 derivation (5 crops, cg 1, was the only size under that bound).  Row b holds pool item b % 11, so rows b and b + 11 must be
    bit-equal and a crop that received a neighbour's bone matrices, partial sums or picked vertices cannot pass; the extra-vertex
    joints are the kernel's own vertices bit for bit."""
    case = crop_group_case
    m = _crop_group_model(case, cuda_dev)
    v, j = _crop_group_run(m, case, B)
    assert torch.equal(v[CROP_GROUP_POOL:], v[:B - CROP_GROUP_POOL]) and torch.equal(j[CROP_GROUP_POOL:], j[:B - CROP_GROUP_POOL]), \
        "rows b and b + 11 hold the same pose and shape but differ"
    n = min(B, CROP_GROUP_POOL)
    vc, jc = v[:n].cpu(), j[:n].cpu()
    dv = np.abs(vc.double().numpy() - case["v64"][:n]).max()
    dj = np.abs(jc.double().numpy() - case["j64"][:n]).max()
    print(f"body_model.hip at {B} crops (update_hips={case['smpl']['update_hips']}) vs independent fp64 derivation: verts {dv:.2e} m, "
          f"joints {dj:.2e} m, bound {TOL_M:.1e} m")
    assert dv < TOL_M and dj < TOL_M
    # joint_map slots >= 24 are picked vertices (smpl_wrapper.py:19-20, vertex_joint_selector.py); none of them is joint 9 / 12 of update_hips
    jm, ev = case["smpl"]["joint_map"].tolist(), case["smpl"]["extra_verts"].tolist()
    vall, jall = v.cpu(), j.cpu()
    picked = 0
    for slot, src in enumerate(jm):
        if src >= 24 and slot not in (8, 9, 12):
            assert torch.equal(jall[:, slot], vall[:, ev[src - 24]]), (B, slot)
            picked += 1
    assert picked >= 10


@pytest.mark.gpu
def test_gpu_lbs_smaller_call_after_larger_leaves_nothing_behind(built_lib, cuda_dev, crop_group_case):
    """257 -> 65 -> 257 crops on ONE handle give the bits each size gives on a fresh handle: partial joint sums, picked vertices and
    arrival counts a larger call left in the handle's workspace do not leak into a smaller one, nor the other way round."""
    from tokenhmr_amd.smpl import SMPL
    case = crop_group_case
    want = {}
    for B in (257, 65):
        f = SMPL(case["smpl"], max_batch=257, device=cuda_dev)
        want[B] = [t.clone() for t in _crop_group_run(f, case, B)]
        f.close()
    m = SMPL(case["smpl"], max_batch=257, device=cuda_dev)
    for B in (257, 65, 257):
        v, j = _crop_group_run(m, case, B)
        assert torch.equal(v, want[B][0]) and torch.equal(j, want[B][1]), B
    m.close()


@pytest.mark.gpu
def test_gpu_engine_applies_update_hips(built_lib, cuda_dev):
    """The flag travels in the weight arena (SMPL(update_hips=...), smpl_wrapper.py:11,33-36) and reaches thmr_forward's LBS."""
    from oracle import tokenhmr_oracle as O
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.engine import Engine
    cfg = HMRConfig(vit_depth=1, dec_depth=1)
    smpl, R, betas = _case(3, 31, True)
    eng = Engine(cfg, max_batch=4, device=cuda_dev)
    eng.load_state(W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0))
    eng.load_smpl(smpl)
    eng.finalize()
    v, j, _, _ = eng.lbs_forward(R.to(cuda_dev), betas.to(cuda_dev))
    vo, jo = O.smpl_forward(R[:, :1], R[:, 1:], betas, smpl)
    _, jplain = O.smpl_forward(R[:, :1], R[:, 1:], betas, dict(smpl, update_hips=False))
    assert (j.cpu() - jo).abs().max() < 1e-5 and (v.cpu() - vo).abs().max() < 1e-5
    assert (jo - jplain).abs().max() > 1e-3          # the flag does change joints 9 / 12


# ---------------------------------------------------------------------------------------------- staged pin
def _fixture():
    p = os.path.join(GOLDEN_DIR, "smplx_lbs.npz")
    if not os.path.exists(p):
        pytest.skip("parity unpinned: tests/golden/smplx_lbs.npz is absent (no smplx wheel in this image; "
                    "oracle/gen_golden_smplx.py writes it the day one exists)")
    return np.load(p)


def test_oracle_vs_real_smplx_fixture():
    from oracle import tokenhmr_oracle as O
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    g = _fixture()
    R, betas = torch.from_numpy(g["rotmat"]), torch.from_numpy(g["betas"])
    for hips, tag in ((False, "plain"), (True, "hips")):
        smpl = dict(make_synthetic_smpl(seed=0), update_hips=hips)
        v, j = O.smpl_forward(R[:, :1], R[:, 1:], betas, smpl)
        assert np.abs(j.numpy() - g[f"joints_{tag}"]).max() < 1e-6
    assert np.abs(v.numpy()[:, ::7] - g["vertices"]).max() < 1e-6
    assert np.abs(O.batch_rodrigues(torch.from_numpy(g["aa"])).numpy() - g["rodrigues"]).max() < 1e-6


@pytest.mark.gpu
def test_gpu_vs_real_smplx_fixture(built_lib, cuda_dev):
    from tokenhmr_amd.smpl import SMPL
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    g = _fixture()
    R, betas = torch.from_numpy(g["rotmat"]), torch.from_numpy(g["betas"])
    for hips, tag in ((False, "plain"), (True, "hips")):
        m = SMPL(dict(make_synthetic_smpl(seed=0), update_hips=hips), max_batch=8, device=cuda_dev)
        o = m(R[:, :1], R[:, 1:], betas, pose2rot=False)
        assert np.abs(o.joints.cpu().numpy() - g[f"joints_{tag}"]).max() < 1e-5
    assert np.abs(o.vertices.cpu().numpy()[:, ::7] - g["vertices"]).max() < 1e-5


@pytest.mark.gpu
def test_gpu_lbs_duplicate_extra_vertex_ids_and_repeated_calls(built_lib, cuda_dev):
    """the fused skin + joints kernel mapped a vertex to ONE extra-joint slot, so a vertex id that appears twice in
    extra_verts left the earlier slot unwritten; and its arrival counters are now zeroed by the prep kernel of the same call
    instead of by the last arriver.  Two extra-joint slots naming the same vertex must both carry it, at several batch sizes
    (1 / 2 / 8 crops per workgroup pass) and on repeated calls."""
    import torch
    from tokenhmr_amd.smpl import SMPL
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from oracle import tokenhmr_oracle as O
    smpl = make_synthetic_smpl(seed=4)
    ev = smpl["extra_verts"].clone()
    ev[1] = ev[0]                                  # slots 0 and 1 -> mapped joints 0 and 15 (smpl_wrapper.py:19-20)
    ev[9] = ev[4]
    smpl["extra_verts"] = ev
    for B in (3, 64, 300):
        m = SMPL(smpl, max_batch=B, device=cuda_dev)
        g = torch.Generator().manual_seed(B)
        R = O.rot6d_to_rotmat(torch.randn(B * 24, 6, generator=g)).view(B, 24, 3, 3)
        betas = torch.randn(B, 10, generator=g)
        for _ in range(2):
            out = m(R[:, :1], R[:, 1:], betas, pose2rot=False)
            v, j = out.vertices.cpu(), out.joints.cpu()
            assert torch.equal(j[:, 0], v[:, int(ev[0])]) and torch.equal(j[:, 15], v[:, int(ev[0])])
            rv, rj = O.smpl_forward(R[:, :1], R[:, 1:], betas, smpl)
            assert (v - rv).abs().max() < 2e-5 and (j - rj).abs().max() < 2e-5
        m.close()
