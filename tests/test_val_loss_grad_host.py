"""The gradient of compute_loss without a device: the NumPy float64 closed form tests/val_loss_grad_oracle.py against
the reference's own float64 autograd (tests/golden/val_loss_grad.npz) and against a torch restatement on fresh inputs; the conditions on
the inputs of tests/test_gpu_val_loss_grad.py, for every seed and shape that file uses; and the two naming constraints the entry point
was designed around."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

import val_loss_grad_oracle as GO

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_golden_val_loss as GV              # noqa: E402
import gen_golden_val_loss_grad as GG         # noqa: E402

WEIGHTS = [GV.LOSS_WEIGHTS[k] for k in ("KEYPOINTS_2D", "KEYPOINTS_3D", "GLOBAL_ORIENT", "BODY_POSE", "BETAS")]


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN_DIR, "val_loss_grad.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def thresholds(golden):
    return {k[7:]: v for k, v in golden.items() if k.startswith("thresh.")}


def _oracle(inp, thresholds, mode, gt, pelvis_id=39):
    return GO.val_loss_grad64(inp, WEIGHTS, loose=mode == "loose", loose_weight=GV.LOOSE_WEIGHT, thresholds=thresholds,
                              valid_3d=GG.valid_3d(inp), pelvis_id=pelvis_id, gt_is_axis_angle=gt == "aa",
                              focal_length=GG.FOCAL_LENGTH, image_size=GG.IMAGE_SIZE)


def _close(name, got, want, rel=1e-12):
    d, scale = np.abs(np.asarray(got) - np.asarray(want)).max(), np.abs(want).max()
    assert got.shape == want.shape and d <= rel * scale, f"{name}: {d:.3e} against {scale:.3e}"


@pytest.mark.parametrize("mode,gt", GG.CASES)
def test_the_oracle_equals_the_reference_record(golden, thresholds, mode, gt):
    inp = {k[3:]: v for k, v in golden.items() if k.startswith("in.")}
    inp["dataset"] = [str(s) for s in inp["dataset"]]
    assert float(golden["focal_length"]) == GG.FOCAL_LENGTH and float(golden["image_size"]) == GG.IMAGE_SIZE
    assert np.array_equal(golden["loss_weights"], np.array(WEIGHTS)) and float(golden["loose_weight"]) == GV.LOOSE_WEIGHT
    GO.input_conditions(inp, thresholds, GG.valid_3d(inp), 39, GG.PLANT)
    got = _oracle(inp, thresholds, mode, gt)
    for k in ("kp2d", "kp3d", "rotmat", "betas"):
        _close(f"{mode} {gt} {k}", got[k], golden[f"{mode}.{gt}.{k}"])
    # the record's chain run projected in float64: (u, v) there are the float64 projection, which the closed form reads from its input
    chain = _oracle(GO.chain_view(inp, GG.FOCAL_LENGTH, GG.IMAGE_SIZE), thresholds, mode, gt)
    for k in ("joints", "cam"):
        _close(f"{mode} {gt} {k}", chain[k], golden[f"{mode}.{gt}.{k}"])
    assert (golden[f"{mode}.{gt}.joints"][0, GG.PLANT] == golden[f"{mode}.{gt}.kp3d"][0, GG.PLANT]).all()      # no projection term there
    assert (got["kp2d"][0, GG.PLANT] == 0).all() and (got["kp3d"][0, GG.PLANT] == 0).all()          # sign(0) = 0


@pytest.mark.parametrize("pelvis_id", [0, 39, 43])
@pytest.mark.parametrize("B", [1, 4, 5])
def test_the_oracle_equals_float64_autograd_of_a_torch_restatement(thresholds, B, pelvis_id):
    inp = GG.make_inputs(B, 900 + 10 * B + pelvis_id, pelvis_id=pelvis_id, thresholds=thresholds)
    seen = GO.chain_view(inp, GG.FOCAL_LENGTH, GG.IMAGE_SIZE)
    for mode, gt in GG.CASES:
        kw = dict(loose=mode == "loose", loose_weight=GV.LOOSE_WEIGHT, thresholds=thresholds, valid_3d=GG.valid_3d(inp), pelvis_id=pelvis_id,
                  gt_is_axis_angle=gt == "aa", focal_length=GG.FOCAL_LENGTH, image_size=GG.IMAGE_SIZE)
        want = {k: v.numpy() for k, v in GO.torch_grads(inp, WEIGHTS, torch.float64, **kw).items()}
        got, chain = GO.val_loss_grad64(inp, WEIGHTS, **kw), GO.val_loss_grad64(seen, WEIGHTS, **kw)
        for k in GO.SLOTS:
            _close(f"B = {B}, pelvis {pelvis_id}, {mode} {gt}: {k}", (chain if k in ("joints", "cam") else got)[k], want[k])
        assert np.abs(want["kp3d"][:, pelvis_id]).max() > 0          # the pelvis row collects the other rows' terms


@pytest.mark.parametrize("B,pelvis_id", GO.GPU_SHAPES)
def test_the_gpu_tests_inputs_meet_the_conditions(thresholds, B, pelvis_id):
    """Every seed and shape of tests/test_gpu_val_loss_grad.py.  A single item cannot take both values of a per-item flag: the full set of
    conditions is asked of the batches of at least four items."""
    inp = GG.make_inputs(B, GO.gpu_seed(B, pelvis_id), pelvis_id=pelvis_id, thresholds=thresholds)
    GO.input_conditions(inp, thresholds, GG.valid_3d(inp), pelvis_id, GG.PLANT, GG.FOCAL_LENGTH, GG.IMAGE_SIZE, full=B >= 4)
    assert (inp["gt_keypoints_2d"][:, :, 2] == 0).any() and (inp["gt_keypoints_3d"][:, :, 3] == 0).any()


def test_the_conditions_bite():
    """input_conditions refuses inputs that break one of them."""
    g = np.load(os.path.join(GOLDEN_DIR, "val_loss_grad.npz"))
    th = {k[7:]: g[k] for k in g.files if k.startswith("thresh.")}
    base = GG.make_inputs(5, GG.SEED, thresholds=th)
    GO.input_conditions(base, th, GG.valid_3d(base), 39, GG.PLANT)

    def broken(change):
        inp = {k: (v.copy() if isinstance(v, np.ndarray) else list(v)) for k, v in base.items()}
        change(inp)
        with pytest.raises(AssertionError):
            GO.input_conditions(inp, th, GG.valid_3d(inp), 39, GG.PLANT)

    broken(lambda i: i["gt_keypoints_2d"].__setitem__((2, 3, 0), i["pred_keypoints_2d"][2, 3, 0] + 1e-4))
    broken(lambda i: i["gt_keypoints_3d"].__setitem__((0, GG.PLANT, 1), i["gt_keypoints_3d"][0, GG.PLANT, 1] + 1e-2))
    broken(lambda i: i["pred_cam"].__setitem__((1, 0), 40.0))                    # t_z = 0.98: X_z below 1
    broken(lambda i: i["has_betas"].fill(1.0))


def test_the_entry_point_keeps_the_two_naming_constraints():
    """thmr_val_loss_grad takes its outputs as a table in host memory and adds no struct: the guard-band bookkeeping
    (tests/test_guarded_host.py) does not count it, and the header keeps its 21 structs (tests/test_cabi_header.py).  Both are intended:
    its guard-band cases live in tests/test_gpu_val_loss_grad.py."""
    from tokenhmr_amd import _cabi
    from test_cabi_header import header_structs
    from test_guarded_host import device_output_entry_points
    with open(_cabi.HEADER) as f:
        text = f.read()
    assert "thmr_val_loss_grad" in _cabi.declared_functions()
    names = device_output_entry_points(text)
    assert "thmr_val_loss_grad" not in names and "thmr_val_loss" in names
    structs = header_structs(re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert len(structs) == 21 and set(structs) == set(_cabi.STRUCTS)
    params = _cabi.declared_functions()["thmr_val_loss_grad"][1]
    assert params == ["thmr_val_loss_desc*", "thmr_val_loss_in*", "float*", "double", "double", "int32_t", "float**", "void*"]
    assert [getattr(_cabi, "LOSS_GRAD_" + k.upper()) for k in GO.SLOTS] == list(range(_cabi.LOSS_GRAD_SLOTS))
