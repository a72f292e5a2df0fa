"""The tokenizer round trip (VanillaTokenizer drop-in, hard decode, quantiser statistics, matrix_to_axis_angle) — what needs no GPU:
the CPU restatement (tests/tokenizer_rt_oracle.py) against the fixture recorded from the reference's own classes
(tests/golden/tokenizer_rt.npz, scripts/gen_golden_tokenizer_rt.py) and, where the reference tree exists, against those classes live;
the facade's refusals before any GPU is touched; the declared and exported symbols."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT
from tokenhmr_amd.config import HMRConfig, RELEASE
from tokenhmr_amd import weights as W
from oracle import ref_import
from oracle.gen_golden_encode import make_pose
import tokenizer_rt_oracle as T

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_golden_tokenizer_rt as G          # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "tokenizer_rt.npz"))


@pytest.fixture(scope="module")
def state(golden):
    """(enc, tok) with the fixture's codebook regenerated from what it stores, every checksum verified."""
    enc, tok = W.make_synthetic_encoder(RELEASE, 0), dict(W.make_synthetic_tokenizer(RELEASE, 0))
    cb = T.make_codebook(torch.from_numpy(golden["mu"]), torch.from_numpy(golden["sd"]), golden["factor"][0], golden["cb_seed"][0])
    for got, key in ((W.checksum({"cb": cb}), "cb_checksum"), (W.checksum(enc), "enc_checksum"), (W.checksum(tok), "dec_checksum")):
        assert abs(got - golden[key][0]) <= 1e-9 * abs(golden[key][0]), key
    tok["quantizer.codebook"] = cb
    return enc, tok


@pytest.fixture(scope="module")
def restated(golden, state):
    enc, tok = state
    out = {}
    with torch.no_grad():
        for tag, B, seed in json.loads(str(golden["batches"])):
            out[tag] = T.roundtrip(make_pose(B, seed), enc, tok, RELEASE)
    return out


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def test_fixture_spreads_the_codes(golden):
    """What the fixture exists for: many winners, and at least 90 % of the tokens away from a near-tie (the GPU test's condition)."""
    for tag, B, _ in json.loads(str(golden["batches"])):
        assert len(golden[f"{tag}.code_ids"]) >= 40 and int(golden[f"{tag}.code_counts"].sum()) == B * 160
        assert (golden[f"{tag}.gap64"] > golden["gap"][0]).mean() >= 0.90
        assert np.array_equal(golden[f"{tag}.idx"], golden[f"{tag}.idx64"])       # the reference's fp32 argmin == its fp64 argmin here


def test_restatement_matches_fixture(golden, restated):
    for tag, B, _ in json.loads(str(golden["batches"])):
        r = restated[tag]
        assert np.array_equal(r["idx"].numpy().astype(np.int32), golden[f"{tag}.idx"])
        assert np.abs(r["latent"].reshape(-1, 256)[::7].numpy() - golden[f"{tag}.latent_sample"]).max() < 1e-6
        assert _rel(r["commit_loss"], golden[f"{tag}.commit_loss"]) < 1e-6
        assert _rel(r["perplexity"], golden[f"{tag}.perplexity"]) < 1e-6
        nz = r["code_count"].nonzero().reshape(-1)
        assert np.array_equal(nz.numpy().astype(np.int32), golden[f"{tag}.code_ids"])
        assert np.array_equal(r["code_count"][nz].numpy().astype(np.int32), golden[f"{tag}.code_counts"])
        for k in ("pose6d", "rotmat", "aa"):
            d = np.abs(r[k].numpy() - golden[f"{tag}.{k}"]).max()
            assert d < 1e-6, (tag, k, d)


def test_restatement_float64(golden, state):
    """The restatement is dtype-generic: in float64 it reproduces the reference's float64 run."""
    enc, tok = state
    enc64, tok64 = {k: v.double() for k, v in enc.items()}, {k: v.double() for k, v in tok.items()}
    with torch.no_grad():
        r = T.roundtrip(make_pose(2, 5).double(), enc64, tok64, RELEASE)
    assert r["pose6d"].dtype == torch.float64 and r["aa"].dtype == torch.float64
    assert np.array_equal(r["idx"].numpy().astype(np.int32), golden["b2.idx64"])
    for k in ("pose6d", "rotmat", "aa"):
        assert np.abs(r[k].numpy() - golden[f"b2.{k}.f64"]).max() < 1e-9, k


def test_straight_through_differs_from_the_code_row(golden, restated, state):
    """quantize_cnn.py:124 x + (c - x) is not c: the two lookup modes of the kernel are two modes."""
    _, tok = state
    r = restated["b3"]
    lat, idx = r["latent"].reshape(-1, 256), r["idx"].reshape(-1)
    st, c = T.straight_through(lat, tok["quantizer.codebook"], idx), tok["quantizer.codebook"][idx]
    n = int((st != c).sum())
    assert 0 < n < st.numel() // 4
    assert ((st - c).abs() <= 2.0 ** -23 * c.abs().clamp(min=lat.abs())).all()


def _assert_aa_within_fp32_class(aa, golden, spans):
    """The branch set reaches angles of 2 pi, where one fp32 ulp is 4.8e-7, and torch's CPU atan2 / sin differ by an ulp or two between
    instruction sets: another fp32 evaluation of the same route is held to what the GPU kernel is held to — per group of the set,
    max(1e-6, 2 x the reference's own fp32-vs-float64 distance on that group) per element."""
    own = json.loads(str(golden["rot.ref32_vs_f64"]))
    for name, (s, e) in spans.items():
        d = np.abs(aa[s:e].numpy() - golden["rot.aa"][s:e]).max()
        assert d <= max(1e-6, 2.0 * own[name]), (name, d)


def test_axis_angle_restatement_matches_fixture(golden):
    R, spans = G.rotation_set(torch.from_numpy(golden["rot.special"]))
    assert json.loads(str(golden["rot.spans"])) == spans
    a, b = spans["random"]
    assert abs(G.rotation_checksum(R[a:b]) - golden["rot.random_checksum"][0]) <= 1e-12 * abs(golden["rot.random_checksum"][0])
    aa = T.matrix_to_axis_angle(R)
    _assert_aa_within_fp32_class(aa, golden, spans)
    aa64 = T.matrix_to_axis_angle(R.double())
    assert aa64.dtype == torch.float64 and np.abs(aa64.numpy() - golden["rot.aa.f64"]).max() < 1e-12
    winner, q0 = T.quaternion_of(R)
    assert np.array_equal(winner.numpy().astype(np.int8), golden["rot.winner"])
    assert int((q0 < 0).sum()) == int(golden["rot.q0_negative"][0]) > 0
    # no standardisation: those are the angles above pi, kept
    assert int((aa.norm(dim=-1) > G.ABOVE_PI).sum()) == int(golden["rot.angle_above_pi"][0]) > 0
    # the branch set takes every branch
    assert sorted(set(winner.tolist())) == [0, 1, 2, 3]
    s = spans["angle_1e-7"]
    assert (aa[s[0]:s[1]].norm(dim=-1) < 1e-6).all() and (aa[s[0]:s[1]].norm(dim=-1) > 0).all()
    assert (aa[spans["identity"][0]] == 0).all()


@pytest.mark.skipif(not ref_import.available(), reason="the reference tree is not on this machine")
def test_restatement_matches_reference_live(golden, state, restated):
    enc, tok = state
    net = G.reference_tokenizer(tok["quantizer.codebook"])
    ns = ref_import.load()
    for tag, B, seed in json.loads(str(golden["batches"])):
        ref = G.run_reference(net, make_pose(B, seed))
        r = restated[tag]
        assert torch.equal(r["idx"], ref["idx"])
        assert _rel(r["commit_loss"], ref["commit_loss"]) < 1e-6 and _rel(r["perplexity"], ref["perplexity"]) < 1e-6
        for k in ("latent", "pose6d", "rotmat", "aa"):
            assert (r[k] - ref[k]).abs().max() < 1e-6, (tag, k)
    R, _ = G.rotation_set()
    assert (R[:golden["rot.special"].shape[0]] - torch.from_numpy(golden["rot.special"])).abs().max() < 1e-7
    assert torch.equal(T.matrix_to_axis_angle(R), ns.rotation_utils.matrix_to_axis_angle(R))      # same machine, same torch kernels: same bits
    # the reference's own encode() raises (it skips preprocess): the facade's encode documents that it has nothing to match
    with pytest.raises(RuntimeError, match="cannot be multiplied"):
        net.encode(make_pose(2, 5))
    # rotation_6d_to_matrix of the tokenizer == geometry.rot6d_to_rotmat on the decoder's output, bit for bit
    p = ref["pose6d"].reshape(-1, 6)
    assert torch.equal(ns.rotation_utils.rotation_6d_to_matrix(p), ns.geometry.rot6d_to_rotmat(p))


# ------------------------------------------------------------------------------------------------ the facade, before any GPU
def _write(tmp_path, cfg, with_encoder=True, arch_overrides=None):
    from _ref_files import write_reference_files
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    sd, tok, smpl = W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0), make_synthetic_smpl(cfg, 0)
    net = dict(tok)
    if with_encoder:
        net.update(W.make_synthetic_encoder(cfg, 0))
    write_reference_files(tmp_path, cfg, sd, net, smpl, arch_overrides=arch_overrides)
    return str(tmp_path / "tokenizer.pth")


def test_vanilla_tokenizer_refuses_before_touching_a_gpu(tmp_path, monkeypatch):
    from tokenhmr_amd import engine as E
    from tokenhmr_amd import ckpt_io
    from tokenhmr_amd.tokenizer import VanillaTokenizer

    def no_engine(*a, **k):
        raise AssertionError("an engine was created before the arguments were checked")
    monkeypatch.setattr(E, "Engine", no_engine)
    cfg = HMRConfig(vit_depth=1, dec_depth=1)
    for d in "abc":
        (tmp_path / d).mkdir()
    path = _write(tmp_path / "a", cfg, arch_overrides={"NB_CODE": 1024})
    with pytest.raises(ValueError, match="NB_CODE"):
        VanillaTokenizer(ckpt_path=path)
    with pytest.raises(ValueError, match="WIDTH"):                     # arch_params themselves, node or dict
        VanillaTokenizer(dict(G.ARCH, WIDTH=256))
    with pytest.raises(ValueError, match="NB_JOINTS"):
        VanillaTokenizer(dict(G.ARCH, NB_JOINTS=52))
    path = _write(tmp_path / "b", cfg, with_encoder=False)
    with pytest.raises(KeyError, match="encoder"):
        VanillaTokenizer(ckpt_path=path)
    torch.save({"state_dict": {}}, tmp_path / "c" / "x.pth")
    with pytest.raises(KeyError, match="net"):
        VanillaTokenizer(ckpt_path=str(tmp_path / "c" / "x.pth"))
    with pytest.raises(NotImplementedError):
        VanillaTokenizer(G.ARCH, add_noise=True)
    with pytest.raises(ValueError, match="6D"):
        VanillaTokenizer(G.ARCH, input_joint_dim=3)
    # the EVAL_ONLY call site: arch from the file's hparams, weights through load_state_dict
    ckpt = ckpt_io.load_checkpoint(_write(tmp_path / "c", cfg))
    net = VanillaTokenizer(ckpt["hparams"].ARCH, mesh_inference=True)
    assert net.eval() is net and net.train(False) is net
    with pytest.raises(NotImplementedError):
        net.train(True)
    with pytest.raises(NotImplementedError):
        net.train()
    with pytest.raises(RuntimeError, match="load_state_dict"):
        net(torch.zeros(1, 21, 6))
    half = {k: v for k, v in ckpt["net"].items() if not k.startswith("encoder.")}
    with pytest.raises(KeyError, match="encoder"):
        net.load_state_dict(half)
    with pytest.raises(KeyError, match="unexpected"):
        net.load_state_dict(dict(ckpt["net"], **{"quantizer.code_sum": torch.zeros(3)}), strict=True)
    assert "body_model.shapedirs" in ckpt["net"]                      # ignored, not "unexpected": only the engine's absence stops this one
    with pytest.raises(AssertionError, match="engine was created"):
        net.load_state_dict(ckpt["net"], strict=True)


def test_new_symbols_declared_and_exported(built_lib):
    from tokenhmr_amd import _cabi, ops
    from tokenhmr_amd.engine import Engine
    # (exported and typed in both builds, like every declared function: tests/test_cabi_header.py)
    assert {"thmr_vq_decode_idx", "thmr_tokenizer_roundtrip", "thmr_op_vq_stats", "thmr_op_rotmat_to_aa"} <= set(_cabi.declared_symbols())
    assert [n for n, _ in _cabi.TokenizerOut._fields_] == ["idx", "latent", "pose6d", "rotmat", "aa", "commit_loss", "perplexity", "code_count",
                                                          "accumulate_counts", "reserved"]
    assert callable(Engine.vq_decode_idx) and callable(Engine.tokenizer_roundtrip) and callable(ops.vq_stats) and callable(ops.rotmat_to_aa)
    # argument checks of the stateless entries come before any HIP call
    assert built_lib.thmr_op_rotmat_to_aa(None, None, 1, None) != 0 and b"null buffer" in built_lib.thmr_last_error(None)
    assert built_lib.thmr_op_vq_stats(None, None, None, 1, None, 0, None, None, None, None) != 0
    assert built_lib.thmr_vq_decode_idx(None, None, 1, None, None) != 0 and built_lib.thmr_tokenizer_roundtrip(None, None, 1, None, None) != 0
