"""The discriminator without a device: tests/discriminator_oracle.py against the reference's own record
(tests/golden/discriminator.npz, both precisions) and, where the reference tree exists, against the live class; the rule that accepts a
seed, for every shape and seed of tests/test_gpu_discriminator.py; the weight block's layout and load_state_dict's strictness; reading a
checkpoint; the entry points' naming constraints."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

import discriminator_oracle as DO
from tokenhmr_amd import _cabi
from tokenhmr_amd import discriminator as DM
from tokenhmr_amd import weights as W

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_golden_discriminator as GD          # noqa: E402

ULP32 = 2.0 ** -23
KEYS = ("out", "loss_adv", "loss_fake", "loss_real", "loss_disc", "grad_poses", "grad_betas", "vjp_poses", "vjp_betas")


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN_DIR, "discriminator.npz"))
    return g, {k[3:]: g[k] for k in g.files if k.startswith("in.")}


def test_the_seeded_weights_and_inputs_have_not_drifted(golden):
    g, inp = golden
    sd = W.make_synthetic_discriminator(DO.WEIGHT_SEED)
    assert [k for k, _ in W.discriminator_spec()] == list(sd) and sum(v.numel() for v in sd.values()) == 1807619
    for k, v in sd.items():
        assert np.array_equal(g["w." + k], v.reshape(-1)[:GD.LEAD].numpy()), k
        assert v.abs().max() > 0, k                                          # the biases too: a zero bias would hide a bias bug
    fresh = DO.make_inputs(DO.BATCH, DO.SEED)
    assert set(fresh) == set(inp) and all(np.array_equal(fresh[k], inp[k]) for k in inp)
    heads = torch.cat([sd[f"pose_out.{j}.weight"] for j in range(23)])
    assert len({tuple(r.tolist()) for r in heads}) == 23                     # 23 distinct heads: a wrong joint -> head pairing shows
    with pytest.raises(ValueError):
        W.make_synthetic_discriminator(0, style="trained")


@pytest.mark.parametrize("name,dtype", [("f32", torch.float32), ("f64", torch.float64)])
def test_the_oracle_equals_the_references_record(golden, name, dtype):
    """float64: to rounding (the real branch goes through another Rodrigues than the reference's quaternions: 1e-9); float32: a few ulp of
    each tensor's largest element."""
    g, inp = golden
    r = DO.run(inp, dtype)
    for k in KEYS:
        ref = g[f"{name}.{k}"]
        assert r[k].dtype == ref.dtype and r[k].shape == ref.shape, k
        d = np.abs(r[k].astype(np.float64) - ref.astype(np.float64)).max() / np.abs(ref).max()
        tol = (1e-9 if "real" in k or "disc" in k else 1e-13) if name == "f64" else 8 * ULP32
        print(f"{name} {k}: relative distance {d:.2e} (bound {tol:.1e})")
        assert d <= tol, (k, d)
    # the columns are different numbers: a swapped pair could not hide
    assert len(np.unique(np.round(g["f64.out"][0], 6))) == 25


def test_the_oracle_equals_the_live_reference():
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("reference tree not present")
    inp = DO.make_inputs(3, 77)
    want, got = GD.run_reference(inp, torch.float64), DO.run(inp, torch.float64)
    for k in KEYS:
        tol = 1e-9 if "real" in k or "disc" in k else 1e-13
        assert np.abs(got[k] - want[k]).max() <= tol * np.abs(want[k]).max(), k
    # the flatten is channel-major: index c * 23 + j (discriminator.py:91)
    x = torch.arange(2 * 32 * 23.0).reshape(2, 32, 23, 1)
    assert torch.equal(x.reshape(2, -1)[0, 23:46], x[0, 1, :, 0])


@pytest.mark.parametrize("B", DO.GPU_BATCHES)
def test_the_gpu_tests_seeds_are_accepted(B):
    """Every (B, seed) of tests/test_gpu_discriminator.py, with the doubled margin discriminator_oracle.GPU_SEED states."""
    ratio = DO.accept(DO.make_inputs(B, DO.GPU_SEED[B]))
    print(f"B = {B}, seed {DO.GPU_SEED[B]}: smallest |z| / precisions' distance = {ratio:.1f}")
    assert ratio >= 2 * DO.MARGIN
    if B == DO.BATCH:
        assert DO.GPU_SEED[B] == DO.SEED                                     # the fixture's inputs


def test_the_rule_bites():
    """Seeds next to the accepted ones fail it (which is why it is asserted and not assumed), and a planted near-zero does."""
    with pytest.raises(AssertionError):
        DO.accept(DO.make_inputs(17, 1000))
    inp = DO.make_inputs(3, 1000)
    taps = {}
    sd = DO.weights(torch.float64)
    DO.forward(sd, torch.from_numpy(inp["poses"]).double(), torch.from_numpy(inp["betas"]).double(), taps=taps)
    inp["betas"] = inp["betas"].copy()
    # move item 0 along betas_fc1's first row until that unit's pre-activation is 1e-8
    w = sd["betas_fc1.weight"][0].numpy()
    inp["betas"][0] -= ((taps["betas_fc1"][0, 0].item() - 1e-8) * w / (w @ w)).astype(np.float32)
    with pytest.raises(AssertionError, match="betas_fc1"):
        DO.accept(inp)


# ------------------------------------------------------------------------------------------------ the weight block
def _packed_forward(block, poses, betas):
    """The forward as the DEVICE reads the block (float64 numpy): h in joint-major order against the permuted, padded fc1."""
    L = {name: block[off:off + int(np.prod(shape))].reshape(shape).astype(np.float64) for name, off, shape in DM.weight_layout()}
    B = betas.shape[0]
    relu = lambda x: np.maximum(x, 0)      # noqa: E731
    a1 = relu(poses.reshape(B, 23, 9) @ L["conv1_t"] + L["conv1_b"])
    a2 = relu(a1 @ L["conv2_t"] + L["conv2_b"])
    heads = (a2 * L["pose_out_w"][None]).sum(-1) + L["pose_out_b"]
    s = relu(relu(betas @ L["betas_fc1_w"].T + L["betas_fc1_b"]) @ L["betas_fc2_w"].T + L["betas_fc2_b"]) @ L["betas_out_w"] + L["betas_out_b"]
    h = np.concatenate([a2.reshape(B, 736), np.full((B, 32), 1e30)], 1)                          # the pad columns meet zero weights
    f2 = relu(relu(h @ L["fc1"].T + L["fc1_b"]) @ L["fc2"].T + L["fc2_b"])
    return np.concatenate([heads, s[:, None], (f2 @ L["out_w"] + L["out_b"])[:, None]], 1), L


def test_the_weight_block_is_the_references_network(golden):
    g, inp = golden
    sd = W.make_synthetic_discriminator(DO.WEIGHT_SEED)
    block = DM.pack_weights(sd).numpy()
    assert block.shape == (_cabi.DISC_WEIGHT_FLOATS,) and all(off % 64 == 0 for _, off, _ in DM.weight_layout())
    out, L = _packed_forward(block, inp["poses"].astype(np.float64), inp["betas"].astype(np.float64))
    assert np.abs(out - g["f64.out"]).max() <= 1e-12 * np.abs(g["f64.out"]).max()
    assert np.array_equal(L["fc1_t"], L["fc1"][:, :736].T) and np.array_equal(L["fc2_t"], L["fc2"].T) and (L["fc1"][:, 736:] == 0).all()
    assert np.array_equal(L["conv1"], L["conv1_t"].T) and np.array_equal(L["conv2"], L["conv2_t"].T)
    # under a prefix, and with the 4-D conv weights as the reference keeps them
    assert sd["D_conv1.weight"].dim() == 4
    assert np.array_equal(DM.pack_weights({"discriminator." + k: v for k, v in sd.items()} | {"backbone.x": torch.zeros(1)}, "discriminator.").numpy(), block)


def test_load_state_dict_is_strict():
    sd = W.make_synthetic_discriminator(1)
    with pytest.raises(KeyError, match="pose_out.22.bias"):
        DM.pack_weights({k: v for k, v in sd.items() if k != "pose_out.22.bias"})
    with pytest.raises(KeyError, match="fc.weight"):
        DM.pack_weights(dict(sd, **{"fc.weight": torch.zeros(4, 4)}))
    with pytest.raises(ValueError, match="D_conv2.weight"):
        DM.pack_weights(dict(sd, **{"D_conv2.weight": sd["D_conv2.weight"].reshape(32, 32)}))
    with pytest.raises(KeyError):
        DM.pack_weights(sd, prefix="discriminator.")


def test_from_checkpoint_reads_the_discriminator_and_load_tokenhmr_ignores_it(tmp_path):
    from _ref_files import write_reference_files
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd.model import read_reference_files
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    cfg = HMRConfig(vit_depth=1, dec_depth=2)
    sd, tok, smpl = W.make_synthetic_state(cfg, 3), W.make_synthetic_tokenizer(cfg, 3), make_synthetic_smpl(cfg, 3)
    dsd = W.make_synthetic_discriminator(2)
    ck, yml = write_reference_files(tmp_path, cfg, sd, tok, smpl, extra_state={"discriminator." + k: v for k, v in dsd.items()})
    # the helper's file also carries a made-up 'discriminator.fc.weight': strict refuses it by name, lenient skips it with a warning
    with pytest.raises(KeyError, match="discriminator.fc.weight"):
        DM.Discriminator.state_from_checkpoint(ck)
    with pytest.warns(RuntimeWarning, match="discriminator.fc.weight"):
        got = DM.Discriminator.state_from_checkpoint(ck, strict=False)
    assert set(got) == {"discriminator." + k for k in dsd} and all(torch.equal(got["discriminator." + k], dsd[k]) for k in dsd)
    assert torch.equal(DM.pack_weights(got, "discriminator."), DM.pack_weights(dsd))
    # load_tokenhmr's host half is unaffected: the same state as without them
    _, state, _, _, _ = read_reference_files(ck, yml)
    assert set(state) == set(sd) and all(torch.equal(state[k], sd[k]) for k in sd)
    plain = tmp_path / "plain"
    plain.mkdir()
    ck2, _ = write_reference_files(plain, cfg, sd, tok, smpl)
    with pytest.raises(KeyError):
        DM.Discriminator.state_from_checkpoint(ck2, strict=False)           # nothing of the module in it
    with pytest.raises(RuntimeError, match="HIP device"):
        DM.Discriminator(device="cpu")


# ------------------------------------------------------------------------------------------------ the C surface
def test_the_entry_points_and_their_constants():
    """New symbols under the current ABI: typed from the header, no new struct, outputs in a host table (so the guard-band bookkeeping of
    tests/test_guarded_host.py does not count them: their guard bands are in tests/test_gpu_discriminator.py)."""
    from test_cabi_header import header_structs
    from test_guarded_host import device_output_entry_points
    with open(_cabi.HEADER) as f:
        text = f.read()
    funcs = _cabi.declared_functions()
    assert funcs["thmr_disc_forward"][1] == ["float*", "float*", "int64_t", "float*", "int32_t", "int32_t", "double", "float**", "void*"]
    assert funcs["thmr_disc_backward"][1] == ["float*", "float*", "int64_t", "float*", "float*", "int32_t", "int32_t", "double", "float**", "void*"]
    assert not {"thmr_disc_forward", "thmr_disc_backward"} & device_output_entry_points(text)
    assert len(header_structs(re.sub(r"/\*.*?\*/", "", text, flags=re.S))) == 21
    for k in ("OUT", "LOSS", "GRAD_POSES", "GRAD_BETAS", "WORKSPACE", "SLOTS", "MAX_BATCH", "KPAD", "WEIGHT_FLOATS", "WS_PER_ITEM"):
        assert f"#define THMR_DISC_{k} {getattr(_cabi, 'DISC_' + k)}\n" in text, k
    assert _cabi.DISC_WS_PER_ITEM == 2 * _cabi.DISC_KPAD + 4 * 1024 + 32 + 1
    lib = _cabi.load()
    assert lib.thmr_disc_forward(None, None, 207, None, 1, 0, 0.0, None, None) == _cabi.ERR_INVALID
    assert b"disc_forward" in lib.thmr_last_error(None)
    assert lib.thmr_disc_backward(None, None, 207, None, None, 1, 0, 0.0, None, None) == _cabi.ERR_INVALID
    assert b"disc_backward" in lib.thmr_last_error(None)
    assert _cabi.ABI_VERSION == 5
