"""SMPL-H and the tokenizer's mesh evaluation, host side (no GPU): the two restatements of tests/smplh_oracle.py against each other,
the fold identity of the body-only path in fp64, the asset loader, the C ABI's declarations, the facade's refusals, the evaluator's
divisor, and the reference's own three error functions executed in place (tests/golden/tokenizer_eval.npz)."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

import smplh_oracle as S
from tokenhmr_amd import _cabi
from tokenhmr_amd.smpl_assets import load_smplh_pkl, make_synthetic_smplh
from tokenhmr_amd.smplh import SMPLH, SMPLHLayer
from tokenhmr_amd.tokenizer_eval import TokenizerEvaluator

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_golden_tokenizer_eval as GE          # noqa: E402

TOL_M = 2e-6     # metres, the bound tests/test_smpl_bounds.py uses for 24 joints


@pytest.fixture(scope="module")
def consts():
    return make_synthetic_smplh(0)


def _pose(B, seed, body_only=False):
    R = S.random_rotations(B * 52, seed=seed).reshape(B, 52, 3, 3)
    if body_only:
        R[:, 0] = np.eye(3)
        R[:, 22:] = np.eye(3)
    return R, np.random.default_rng(seed + 1).standard_normal((B, 10))


def test_synthetic_constants_are_structure_faithful(consts):
    from tokenhmr_amd.config import SMPLH_PARENTS, SMPL_EXTRA_VERTS, SMPL_PARENTS
    p = consts["parents"].tolist()
    assert p == SMPLH_PARENTS and len(p) == 52 and p[0] == -1 and all(0 <= p[i] < i for i in range(1, 52))
    assert p[:22] == SMPL_PARENTS[:22]                                   # the body of SMPL
    for wrist, first in ((20, 22), (21, 37)):                            # five three-joint fingers per wrist
        for f in range(5):
            assert p[first + 3 * f: first + 3 * f + 3] == [wrist, first + 3 * f, first + 3 * f + 1]
    assert consts["extra_verts"].tolist() == SMPL_EXTRA_VERTS
    assert consts["posedirs"].shape == (459, 20670) and consts["lbs_weights"].shape == (6890, 52)
    assert torch.allclose(consts["lbs_weights"].sum(1), torch.ones(6890), atol=1e-5)
    assert consts["hands_meanl"].shape == (45,) and consts["hands_componentsr"].shape == (45, 45)


def test_smplx_formulation_matches_independent_derivation(consts):
    R, betas = _pose(2, 11)
    t = np.random.default_rng(3).standard_normal((2, 3))
    v64, j64 = S.smplh_forward_independent(R, betas, consts, t)
    v, j = S.smplh_forward_smplx32(R, betas, consts, t)
    dv, dj = np.abs(v.double().numpy() - v64).max(), np.abs(j.double().numpy() - j64).max()
    print(f"smplx formulation (fp32) vs independent fp64 derivation, 52 joints: verts {dv:.2e} m, joints {dj:.2e} m")
    assert j64.shape == (2, 73, 3) and dv < TOL_M and dj < TOL_M
    assert np.array_equal(j64[:, 52:], v64[:, consts["extra_verts"].numpy()])


def test_independent_derivation_does_not_depend_on_joint_order(consts):
    R, betas = _pose(1, 5)
    v0, j0 = S.smplh_forward_independent(R, betas, consts)
    perm = np.concatenate([[0], 1 + np.random.default_rng(0).permutation(51)])       # new index i holds old joint perm[i]
    inv = np.argsort(perm)
    p_old = consts["parents"].numpy()
    c2 = dict(consts)
    c2["parents"] = torch.tensor([-1 if p_old[perm[i]] < 0 else inv[p_old[perm[i]]] for i in range(52)], dtype=torch.int32)
    assert any(int(c2["parents"][i]) > i for i in range(52))
    c2["J_regressor"] = consts["J_regressor"][perm]
    c2["lbs_weights"] = consts["lbs_weights"][:, perm]
    c2["posedirs"] = consts["posedirs"].reshape(51, 9, -1)[perm[1:] - 1].reshape(459, -1)
    v1, j1 = S.smplh_forward_independent(R[:, perm], betas, c2)
    assert np.abs(v1 - v0).max() < 1e-12 and np.abs(j1[:, :52] - j0[:, perm]).max() < 1e-12


def test_fold_identity_fp64(consts):
    """A joint whose local rotation is the identity has its parent's bone matrix, so the 22-joint model with each hand's weight columns
    added into its wrist IS the 52-joint model with identity hands — to fp64 rounding, with shapes and a rotated root."""
    R, betas = _pose(2, 7)
    R[:, 22:] = np.eye(3)
    v52, j52 = S.smplh_forward_independent(R, betas, consts)
    cf = S.fold_constants(consts)
    assert cf["lbs_weights"].shape == (6890, 22) and cf["posedirs"].shape == (189, 20670)
    v22, j22 = S.smplh_forward_independent(R[:, :22], betas, cf)
    d = np.abs(v22 - v52).max()
    print(f"folded 22-joint model vs 52 joints with identity hands (fp64): {d:.2e} m")
    assert d < 1e-12
    assert np.abs(j22[:, :22] - j52[:, :22]).max() < 1e-12 and np.abs(j22[:, 22:] - j52[:, 52:]).max() < 1e-12


class _DenseStandIn:
    """What load_smplh_pkl needs of a scipy sparse matrix (`toarray`), for an image without scipy."""

    def __init__(self, a):
        self.a = a

    def toarray(self):
        return self.a


def test_load_smplh_pkl_roundtrip(tmp_path, consts):
    try:
        from scipy.sparse import csc_matrix
    except ImportError:
        csc_matrix = _DenseStandIn
    kt = np.stack([np.array([2 ** 32 - 1] + consts["parents"].tolist()[1:], dtype=np.uint32), np.arange(52, dtype=np.uint32)])
    d = {"v_template": consts["v_template"].numpy(), "shapedirs": np.concatenate([consts["shapedirs"].numpy(), np.zeros((6890, 3, 6), np.float32)], 2),
         "posedirs": consts["posedirs"].numpy().T.reshape(6890, 3, 459).copy(),
         "J_regressor": csc_matrix(consts["J_regressor"].numpy() * (consts["J_regressor"].numpy() > 1e-3)),
         "weights": consts["lbs_weights"].numpy(), "kintree_table": kt, "f": np.arange(12, dtype=np.uint32).reshape(4, 3),
         "hands_meanl": consts["hands_meanl"].numpy(), "hands_meanr": consts["hands_meanr"].numpy(),
         "hands_componentsl": consts["hands_componentsl"].numpy(), "hands_componentsr": consts["hands_componentsr"].numpy()}
    os.makedirs(tmp_path / "smplh")
    path = tmp_path / "smplh" / "SMPLH_NEUTRAL.pkl"
    with open(path, "wb") as f:
        pickle.dump(d, f)
    a = load_smplh_pkl(str(path))
    assert a["parents"].tolist() == consts["parents"].tolist() and a["parents"].dtype == torch.int32
    assert torch.equal(a["posedirs"], consts["posedirs"]) and a["shapedirs"].shape == (6890, 3, 10)
    assert torch.equal(a["shapedirs"], consts["shapedirs"]) and torch.equal(a["lbs_weights"], consts["lbs_weights"])
    assert a["J_regressor"].shape == (52, 6890) and a["J_regressor"].dtype == torch.float32
    assert a["faces"].shape == (4, 3) and a["faces"].dtype == torch.int64 and torch.equal(a["hands_meanr"], consts["hands_meanr"])
    # the drop-in resolves a model DIRECTORY the way smplx does (no GPU is touched before the first forward)
    layer = SMPLHLayer(str(tmp_path / "smplh"), num_betas=10, ext="pkl")
    assert layer.faces.shape == (4, 3) and layer.folded_calls == 0
    del d["hands_meanl"]
    with open(tmp_path / "bad.pkl", "wb") as f:
        pickle.dump(d, f)
    with pytest.raises(KeyError, match="hands_meanl"):
        load_smplh_pkl(str(tmp_path / "bad.pkl"))


def test_symbols_declared_exported_and_bound():
    import __graft_entry__
    assert "body_model.hip" in __graft_entry__.SOURCES
    assert {"thmr_smplh_create", "thmr_smplh_destroy", "thmr_smplh_forward", "thmr_op_mean_row_dist"} <= set(_cabi.declared_symbols())
    assert _cabi.ABI_VERSION == 5
    header = open(_cabi.HEADER).read()
    assert "#define THMR_ABI_VERSION 5" in header and f"#define THMR_MEAN_ROW_DIST_WS {_cabi.MEAN_ROW_DIST_WS}" in header
    assert [f[0] for f in _cabi.SmplhDesc._fields_][:8] == ["v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights", "parents",
                                                           "extra_verts", "on_device"]
    if os.path.exists(_cabi.LIB_PATH):
        lib = _cabi.load()              # raises unless the library exports every declared function
        # argument refusals happen before any HIP call, so they can be exercised without a device
        assert lib.thmr_smplh_create(None, 4, 0, None) != 0
        assert lib.thmr_op_mean_row_dist(None, None, 73, 1, 22, 2, None, None, None) != 0
        assert b"null" in lib.thmr_last_error(None)
        assert lib.thmr_smplh_forward(None, None, 0, None, None, 1, 1, None, None, None) != 0


def test_facade_refusals_need_no_gpu(consts):
    with pytest.raises(ValueError, match="num_pca_comps"):
        SMPLH(consts, num_pca_comps=0)
    with pytest.raises(ValueError, match="num_pca_comps"):
        SMPLH(consts, num_pca_comps=46)
    with pytest.raises(ValueError, match="num_betas"):
        SMPLHLayer(consts, num_betas=16)
    with pytest.raises(ValueError, match="posedirs"):
        SMPLHLayer(dict(consts, posedirs=consts["posedirs"][:207]))
    layer, model = SMPLHLayer(consts, max_batch=4), SMPLH(consts, max_batch=4, use_pca=False)
    with pytest.raises(ValueError, match="max_batch"):
        layer(body_pose=torch.zeros(5, 21, 3, 3))
    with pytest.raises(ValueError, match="body_pose"):
        layer(body_pose=torch.zeros(2, 23, 3, 3))
    with pytest.raises(ValueError, match="left_hand_pose"):
        layer(body_pose=torch.zeros(2, 21, 3, 3), left_hand_pose=torch.zeros(2, 15, 3))
    with pytest.raises(ValueError, match="batch size"):
        layer(body_pose=torch.zeros(2, 21, 3, 3), betas=torch.zeros(3, 10))
    with pytest.raises(ValueError, match="body_pose"):
        model(body_pose=torch.zeros(2, 69))
    with pytest.raises(ValueError, match="left_hand_pose"):
        model(body_pose=torch.zeros(2, 63), left_hand_pose=torch.zeros(2, 6))          # use_pca=False: 45 values
    with pytest.raises(ValueError, match="right_hand_pose"):
        SMPLH(consts, max_batch=4)(body_pose=torch.zeros(2, 63), right_hand_pose=torch.zeros(2, 45))      # 6 PCA coefficients
    assert layer.folded_calls == 0 and layer.full_calls == 0 and layer.h is None


def test_evaluator_divisor():
    sums = torch.tensor([0.3, 0.06, 0.09, 30.0, 0.6], dtype=torch.float64)
    ev = TokenizerEvaluator(device="cpu")
    ev.sums, ev.batches = sums.clone(), 3
    m = ev.get_metrics_dict()                       # the reference's divisor: batch_idx = 2
    assert m["val/curr_pose_recons"] == pytest.approx(0.15) and m["val/curr_mesh_recons"] == pytest.approx(30.0)
    assert m["val/curr_jnt_recons"] == pytest.approx(45.0) and m["val/curr_perplexity"] == pytest.approx(15.0)
    assert m["val/curr_commit"] == pytest.approx(0.3) and m["curr_score"] == pytest.approx(75.0)
    assert set(m) == {"val/curr_pose_recons", "val/curr_mesh_recons", "val/curr_jnt_recons", "val/curr_perplexity", "val/curr_commit", "curr_score"}
    ev2 = TokenizerEvaluator(device="cpu", mean="batches")
    ev2.sums, ev2.batches = sums.clone(), 3
    assert ev2.get_metrics_dict()["curr_score"] == pytest.approx(50.0)
    ev.batches = 1
    with pytest.raises(ValueError, match="batch_idx"):
        ev.get_metrics_dict()
    ev2.batches = 1
    assert ev2.get_metrics_dict()["val/curr_pose_recons"] == pytest.approx(0.3)
    with pytest.raises(ValueError):
        TokenizerEvaluator(device="cpu", mean="median")
    with pytest.raises(KeyError, match="pred_body_vertices"):
        ev(dict(), {"pred_pose_body_rotmat": torch.zeros(1, 21, 3, 3)}, torch.zeros(()), torch.zeros(()))


def test_reference_error_functions_match_fixture_and_fp64():
    g = np.load(os.path.join(GOLDEN_DIR, "tokenizer_eval.npz"))
    for name, (seed, shape, _) in GE.CASES.items():
        assert int(g[f"{name}.seed"]) == seed and tuple(g[f"{name}.shape"]) == shape
        gt, pred = GE.eval_inputs(seed, shape)
        B = shape[0]
        lo, hi = (1, 22) if name == "jnts" else (0, None)
        ref64 = S.mean_row_dist64(gt.reshape(B, -1, 3).numpy(), pred.reshape(B, -1, 3).numpy(), lo, hi)
        rel = abs(float(g[f"{name}.value"]) - ref64) / ref64
        print(f"{name}: reference fp32 {float(g[f'{name}.value']):.8f}, fp64 formula {ref64:.10f}, relative difference {rel:.1e}")
        # fp32 rounding: a few ulp per row (subtract, square, sum, sqrt) + torch's pairwise mean over <= 20670 rows (~log2(n) ulp)
        assert rel < 2e-6


def test_reference_error_functions_executed_in_place():
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("reference tree not present")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_golden_tokenizer_eval.py"), "--check"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bit for bit" in r.stdout
