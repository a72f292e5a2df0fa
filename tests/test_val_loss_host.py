"""The validation loss, host side (no GPU): the fp64 restatement of tests/val_loss_oracle.py against the reference's own float64 record
(tests/golden/val_loss.npz, written by scripts/gen_golden_val_loss.py from TokenHMR.compute_loss executed in place), the C ABI's
declarations and exports, ValidationLoss' argument handling on CPU tensors up to the point of the launch, and — where the reference
tree is present — a live re-run of the generator against the committed fixture."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

import val_loss_oracle as VO
from tokenhmr_amd import _cabi
from tokenhmr_amd.losses import LOSS_KEYS, ValidationLoss, load_thresholds
from tokenhmr_amd.model import ConfigNode

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_golden_val_loss as GV          # noqa: E402


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN_DIR, "val_loss.npz"))
    return {k: g[k] for k in g.files}


def _inputs(golden):
    return {k[3:]: v for k, v in golden.items() if k.startswith("in.")}


def _thresholds(golden):
    return {k[7:]: v for k, v in golden.items() if k.startswith("thresh.")}


def _cfg(loose=True):
    return ConfigNode({"MODEL": {"LOOSE_SUP": loose, "LOOSE_WEIGHT": GV.LOOSE_WEIGHT}, "LOSS_WEIGHTS": dict(GV.LOSS_WEIGHTS)})


@pytest.mark.parametrize("mode", ["plain", "loose"])
def test_oracle_matches_the_reference_fp64_record(golden, mode):
    inp = _inputs(golden)
    r = VO.val_loss64(inp, golden["loss_weights"], loose=mode == "loose", loose_weight=float(golden["loose_weight"]),
                      thresholds=_thresholds(golden), valid_3d=inp["valid_3d"])
    ref = golden[f"{mode}.f64.losses"]
    rel = np.abs(r["losses"] - ref) / np.abs(ref)
    print(f"{mode}: oracle vs the reference's float64 losses, relative: " + " ".join(f"{x:.1e}" for x in rel))
    assert rel.max() <= 1e-12
    assert np.allclose(r["per_item"].sum(0), ref[1:], rtol=1e-12, atol=0)
    if mode == "loose":
        for k in ("kp2d_err", "angle_err"):
            assert np.abs(r[k] - golden[f"loose.f64.{k}"]).max() <= 1e-12
        for k in ("valid2d", "weak2d", "valid_rot", "weak_rot", "conf2d_used", "conf3d_used", "has_betas_used"):
            assert np.array_equal(r[k], golden[f"loose.f64.{k}"]), k
        # both sides of both thresholds are exercised, and every flag takes both values
        assert 0.2 < r["valid2d"].mean() < 0.8 and 0.2 < (r["angle_err"] > 0.3).mean() < 0.9 and r["weak_rot"].sum() > 0
        for k in ("has_global_orient", "has_body_pose", "has_betas", "valid_3d"):
            assert set(np.unique(inp[k])) == {0.0, 1.0}, k


def test_fixture_margins_and_token_loss(golden):
    for q in ("angle_err", "kp2d_err"):
        assert golden[f"margin.{q}.min_gap"] > 4 * golden[f"margin.{q}.d_ref"] > 0
    probs, tgt = GV.token_inputs(int(golden["token.seed"]), int(golden["token.rows"]))
    ce = VO.token_ce64(probs.numpy(), tgt.numpy())
    assert abs(ce - float(golden["token.f64"])) <= 1e-12 * abs(ce)
    assert abs(float(golden["token.f32"]) - ce) <= 1e-5 * abs(ce)


def test_oracle_matrix_and_axis_angle_ground_truth_agree(golden):
    inp = _inputs(golden)
    a = VO.val_loss64(inp, golden["loss_weights"])
    inp2 = dict(inp, gt_pose_rotmat=VO.aa_to_rotmat64(inp["gt_pose_aa"].reshape(-1, 3)).reshape(-1, 24, 3, 3))
    b = VO.val_loss64(inp2, golden["loss_weights"], gt_is_axis_angle=False)
    assert np.array_equal(a["losses"], b["losses"])


def test_symbols_declared_exported_and_bound():
    import __graft_entry__
    assert "loss.hip" in __graft_entry__.SOURCES
    assert {"thmr_val_loss", "thmr_op_token_ce"} <= set(_cabi.declared_symbols())
    assert _cabi.ABI_VERSION == 5
    header = open(_cabi.HEADER).read()
    assert "#define THMR_ABI_VERSION 5" in header
    assert f"#define THMR_VAL_LOSS_WS_PER_ITEM {_cabi.VAL_LOSS_WS_PER_ITEM}" in header
    assert f"#define THMR_TOKEN_CE_WS_PER_ROW {_cabi.TOKEN_CE_WS_PER_ROW}" in header
    assert f"#define THMR_VAL_LOSS_PLAIN {_cabi.VAL_LOSS_PLAIN}" in header and f"#define THMR_VAL_LOSS_LOOSE {_cabi.VAL_LOSS_LOOSE}" in header
    # the field lists the facade fills the structs by are the mirrors' fields (and those the header's, in order: tests/test_cabi_header.py)
    assert [n for n, _ in _cabi.ValLossIn._fields_] == _cabi.VAL_LOSS_IN_FIELDS
    assert [n for n, _ in _cabi.ValLossOut._fields_] == _cabi.VAL_LOSS_OUT_FIELDS
    assert C.sizeof(_cabi.ValLossDesc) == 6 * 8 + 4 * 4 and C.sizeof(_cabi.ValLossIn) == 14 * 8 and C.sizeof(_cabi.ValLossOut) == 12 * 8
    # both prototypes as the header states them
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert ("int thmr_val_loss(const thmr_val_loss_desc* desc, const thmr_val_loss_in* in, int32_t B, const thmr_val_loss_out* out, "
            "float* workspace_dev, void* stream);") in flat
    assert ("int thmr_op_token_ce(const float* x_dev, const int32_t* target_dev, int32_t rows, float* out_dev, float* workspace_dev, "
            "void* stream);") in flat


def test_library_exports_both_entry_points_and_refuses_without_a_device(built_lib):
    lib = built_lib
    assert len(lib.thmr_val_loss.argtypes) == 6 and len(lib.thmr_op_token_ce.argtypes) == 6
    # argument refusals happen before any HIP call, so they can be exercised without a device
    assert lib.thmr_val_loss(None, None, 1, None, None, None) == -1
    assert b"val_loss" in lib.thmr_last_error(None)
    assert lib.thmr_op_token_ce(None, None, 1, None, None, None) == -1
    assert b"token_ce" in lib.thmr_last_error(None)


# ------------------------------------------------------------------------------------------------ ValidationLoss, up to the launch
def _dicts(golden, is_axis_angle=True):
    inp = dict(_inputs(golden))
    inp["dataset"] = [str(s) for s in inp["dataset"]]
    return GV.to_batch(inp, torch.float32, is_axis_angle)


def test_missing_thresholds_is_a_value_error_that_names_the_argument(golden):
    batch, output = _dicts(golden)
    vl = ValidationLoss(_cfg(loose=True))
    with pytest.raises(ValueError, match="thresholds"):
        vl.prepare(batch, output, train=True)
    a = vl.prepare(batch, output, train=False)                    # validation never needs them (tokenhmr.py:214: LOOSE_SUP and train)
    assert a["loose"] is False and a["valid_3d"] is None
    assert ValidationLoss(_cfg(loose=False)).prepare(batch, output, train=True)["loose"] is False
    with pytest.raises(ValueError, match="body_pose"):
        ValidationLoss(_cfg(), thresholds={"kp2d": np.zeros(44), "global_orient": np.zeros(1)})
    with pytest.raises(ValueError, match="kp2d"):
        ValidationLoss(_cfg(), thresholds={"kp2d": np.zeros(43), "global_orient": np.zeros(1), "body_pose": np.zeros(23)})
    with pytest.raises(KeyError, match="LOSS_WEIGHTS"):
        ValidationLoss(ConfigNode({"MODEL": {}}))
    with pytest.raises(KeyError, match="BETAS"):
        ValidationLoss(ConfigNode({"MODEL": {}, "LOSS_WEIGHTS": {k: 1.0 for k in ("KEYPOINTS_2D", "KEYPOINTS_3D", "GLOBAL_ORIENT", "BODY_POSE")}}))


def test_thresholds_from_a_mapping_and_from_an_npz(golden, tmp_path):
    th = _thresholds(golden)
    a = load_thresholds(th)
    assert a["kp2d"].shape == (44,) and a["angle"].shape == (24,) and a["kp2d"].dtype == torch.float32
    assert float(a["angle"][0]) == float(th["global_orient"][0]) and torch.equal(a["angle"][1:], torch.from_numpy(th["body_pose"]))
    np.savez(tmp_path / "t.npz", **th)
    b = load_thresholds(str(tmp_path / "t.npz"))
    assert torch.equal(a["kp2d"], b["kp2d"]) and torch.equal(a["angle"], b["angle"])
    vl = ValidationLoss(_cfg(), thresholds=str(tmp_path / "t.npz"))
    assert vl.weights == [0.01, 0.05, 0.001, 0.001, 0.0005] and vl.loose_weight == 0.05 and vl.loose_sup and vl.pelvis_id == 39


def test_mixed_is_axis_angle_is_refused_by_name(golden):
    vl = ValidationLoss(_cfg(loose=False))
    batch, output = _dicts(golden)
    batch["smpl_params_is_axis_angle"]["body_pose"][3] = False
    with pytest.raises(ValueError, match=r"smpl_params_is_axis_angle'\]\['body_pose'\] mixes"):
        vl.prepare(batch, output)
    batch, output = _dicts(golden)
    batch["smpl_params_is_axis_angle"]["global_orient"][:] = False          # says matrices, holds 3 values per item
    with pytest.raises(ValueError, match="global_orient"):
        vl.prepare(batch, output)
    # strict_flags reads the flags wherever they live (one synchronisation for device flags); the same refusals
    batch, output = _dicts(golden)
    batch["smpl_params_is_axis_angle"]["body_pose"][3] = False
    with pytest.raises(ValueError, match="mixes"):
        ValidationLoss(_cfg(loose=False), strict_flags=True).prepare(batch, output)
    assert ValidationLoss(_cfg(loose=False), strict_flags=True).prepare(*_dicts(golden))["gt_pose"].shape == (8, 72)
    # matrices throughout: accepted, and handed on as (B,24,3,3)
    batch, output = _dicts(golden, is_axis_angle=False)
    R = torch.from_numpy(VO.aa_to_rotmat64(golden["in.gt_pose_aa"].reshape(-1, 3)).reshape(-1, 24, 3, 3)).float()
    batch["smpl_params"]["global_orient"], batch["smpl_params"]["body_pose"] = R[:, :1], R[:, 1:]
    a = vl.prepare(batch, output)
    assert a["gt_pose"].shape == (8, 24, 3, 3) and torch.equal(a["gt_pose"], R)
    batch["smpl_params"]["body_pose"] = torch.from_numpy(golden["in.gt_pose_aa"][:, 3:])         # one key axis-angle, the other matrices
    batch["smpl_params_is_axis_angle"]["body_pose"][:] = True
    with pytest.raises(ValueError, match="both"):
        vl.prepare(batch, output)
    a = vl.prepare(*_dicts(golden))
    assert a["gt_pose"].shape == (8, 72) and torch.equal(a["gt_pose"], torch.from_numpy(golden["in.gt_pose_aa"]))


def test_valid_3d_rule_and_no_mutation(golden):
    batch, output = _dicts(golden)
    before = {k: batch[k].clone() for k in ("keypoints_2d", "keypoints_3d")}
    hb = batch["has_smpl_params"]["betas"].clone()
    vl = ValidationLoss(_cfg(), thresholds=_thresholds(golden))
    a = vl.prepare(batch, output, train=True)
    assert a["loose"] is True
    assert torch.equal(a["valid_3d"], torch.from_numpy(golden["in.valid_3d"]))                 # tokenhmr.py:226
    assert a["valid_3d"].tolist() == [float(n in ("H36M-TRAIN-WMASK", "BEDLAM")) for n in batch["dataset"]]
    other = ValidationLoss(_cfg(), thresholds=_thresholds(golden), trusted_3d_datasets=("MPII-TRAIN",))
    assert other.prepare(batch, output, train=True)["valid_3d"].tolist() == [float(n == "MPII-TRAIN") for n in batch["dataset"]]
    batch["dataset"] = batch["dataset"][:-1]
    with pytest.raises(ValueError, match="dataset"):
        vl.prepare(batch, output, train=True)
    assert torch.equal(batch["keypoints_2d"], before["keypoints_2d"]) and torch.equal(batch["keypoints_3d"], before["keypoints_3d"])
    assert torch.equal(batch["has_smpl_params"]["betas"], hb)
    # the two views of one rotmat buffer are handed on without a copy; separate tensors are joined
    R = torch.from_numpy(golden["in.pred_rotmat"]).clone()
    output["pred_smpl_params"]["global_orient"], output["pred_smpl_params"]["body_pose"] = R[:, :1], R[:, 1:]
    batch["dataset"] = [str(s) for s in golden["in.dataset"]]
    assert vl.prepare(batch, output)["pred_rotmat"].data_ptr() == R.data_ptr()
    output["pred_smpl_params"]["body_pose"] = R[:, 1:].clone()
    j = vl.prepare(batch, output)["pred_rotmat"]
    assert j.data_ptr() != R.data_ptr() and torch.equal(j, R)
    assert LOSS_KEYS == tuple(GV.LOSS_KEYS) == VO.LOSS_KEYS


def test_live_reference_reproduces_the_fixture():
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("reference tree not present")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_golden_val_loss.py"), "--check"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "reproduces the committed fixture" in r.stdout
