"""The tokenizer round trip on the GPU: hard decode (thmr_vq_decode_idx), thmr_tokenizer_roundtrip, the quantiser-statistics and
matrix_to_axis_angle kernels alone, and the VanillaTokenizer drop-in — against tests/golden/tokenizer_rt.npz (the reference's own
VanillaTokenizer, scripts/gen_golden_tokenizer_rt.py) and the CPU restatement tests/tokenizer_rt_oracle.py.  Engines are
HMRConfig(vit_depth=1, dec_depth=1) with max_batch=8 unless the test is about another size."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT
from tokenhmr_amd.config import HMRConfig, RELEASE
from tokenhmr_amd import weights as W
from oracle.gen_golden_encode import make_pose
import tokenizer_rt_oracle as T

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_golden_tokenizer_rt as G          # noqa: E402

pytestmark = pytest.mark.gpu
CFG = HMRConfig(vit_depth=1, dec_depth=1)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "tokenizer_rt.npz"))


@pytest.fixture(scope="module")
def state(golden):
    enc, tok = W.make_synthetic_encoder(RELEASE, 0), dict(W.make_synthetic_tokenizer(RELEASE, 0))
    cb = T.make_codebook(torch.from_numpy(golden["mu"]), torch.from_numpy(golden["sd"]), golden["factor"][0], golden["cb_seed"][0])
    assert abs(W.checksum({"cb": cb}) - golden["cb_checksum"][0]) <= 1e-9 * abs(golden["cb_checksum"][0])
    tok["quantizer.codebook"] = cb
    return enc, tok


def _engine(state, dev, max_batch=8, cfg=CFG, encoder=True):
    from tokenhmr_amd.engine import Engine
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    enc, tok = state
    eng = Engine(cfg, max_batch=max_batch, device=dev)
    eng.load_state(W.make_synthetic_state(cfg, 0), dict(tok, **enc) if encoder else tok)
    eng.load_smpl(make_synthetic_smpl(cfg, 0))
    eng.finalize()
    return eng


@pytest.fixture(scope="module")
def eng(built_lib, cuda_dev, state):
    e = _engine(state, cuda_dev)
    yield e
    e.close()


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


# ------------------------------------------------------------------------------------------------ 1. hard decode
@pytest.mark.parametrize("B", [2, 7], ids=["tiny-M regime", "tile regime"])
def test_hard_decode_is_bit_identical_to_one_hot(eng, cuda_dev, B):
    """A one-hot row contributes one non-zero fp32 term to probs @ codebook, so the GEMM returns the code row exactly and the two
    paths must agree bit for bit — on both sides of vq_decode's B * 192 <= kSmallM switch (6 | 7 poses)."""
    idx = torch.randint(0, 2048, (B, 160), generator=torch.Generator().manual_seed(70 + B))
    idx[0, 0], idx[0, 1], idx[-1, -1] = 0, 2047, 2047
    onehot = torch.zeros(B, 160, 2048).scatter_(2, idx.unsqueeze(-1), 1.0)
    hard = eng.vq_decode_idx(idx.to(cuda_dev))
    soft = eng.vq_decode(onehot.to(cuda_dev))
    eng.status()
    assert hard.shape == (B, 21, 6) and torch.equal(hard, soft)
    assert torch.equal(eng.vq_decode_idx(idx.to(cuda_dev).to(torch.int32)), hard)          # int64 and int32 callers alike


def test_hard_decode_ragged_batch_and_parity(eng, cuda_dev, golden, state):
    _, tok = state
    idx = torch.randint(0, 2048, (5, 160), generator=torch.Generator().manual_seed(75)).to(cuda_dev)
    all5 = eng.vq_decode_idx(idx)                                                          # 5 of max_batch 8
    for i in range(5):
        assert torch.equal(eng.vq_decode_idx(idx[i:i + 1])[0], all5[i]), i
    # decode(fixture idx) against the reference's pred_pose_body_6d (which went through the straight-through value: an ulp of the
    # operand away) and against the restatement's plain decode
    for tag in ("b3", "b2"):
        gi = torch.from_numpy(golden[f"{tag}.idx"])
        got = eng.vq_decode_idx(gi.to(cuda_dev)).cpu()
        d = (got - torch.from_numpy(golden[f"{tag}.pose6d"])).abs().max().item()
        with torch.no_grad():
            d2 = (got - T.decode_indices(gi, tok, CFG)).abs().max().item()
        print(f"[{tag}] decode(fixture idx): max|diff| {d:.3e} against the fixture's pose, {d2:.3e} against the plain restatement")
        assert d < 1e-4 and d2 < 1e-4
    eng.status()


def test_hard_decode_reports_an_out_of_range_index(eng, cuda_dev):
    """A bad index is clamped on the device (the result is the clamped indices' — nothing foreign was read) and reported once."""
    from tokenhmr_amd._cabi import EngineError
    good = torch.randint(0, 2048, (3, 160), generator=torch.Generator().manual_seed(76))
    bad = good.clone()
    bad[1, 17], bad[2, 159], bad[0, 0] = 2048, -1, 1 << 30
    out = eng.vq_decode_idx(bad.to(cuda_dev))
    with pytest.raises(EngineError, match="code index outside"):
        eng.status()
    eng.status()                                                                           # reported once, the engine stays usable
    assert torch.equal(out, eng.vq_decode_idx(bad.clamp(0, 2047).to(cuda_dev)))
    eng.status()
    # ... and without a status read the next hard-decode call reports it
    eng.vq_decode_idx(bad.to(cuda_dev))
    torch.cuda.synchronize()
    with pytest.raises(EngineError, match="code index outside"):
        eng.vq_decode_idx(good.to(cuda_dev))
    eng.vq_decode_idx(good.to(cuda_dev))
    eng.status()


# ------------------------------------------------------------------------------------------------ 2. the round trip
@pytest.mark.parametrize("tag", ["b3", "b2"])
def test_roundtrip_against_the_fixture(eng, cuda_dev, golden, state, tag):
    enc, tok = state
    _, B, seed = next(b for b in json.loads(str(golden["batches"])) if b[0] == tag)
    pose = make_pose(B, seed)
    want = ("idx", "latent", "pose6d", "rotmat", "aa", "commit_loss", "perplexity", "code_count")
    o = eng.tokenizer_roundtrip(pose.to(cuda_dev), want=want)
    again = eng.tokenizer_roundtrip(pose.to(cuda_dev), want=want)
    eng.status()
    for k in want:
        assert torch.equal(o[k], again[k]), f"{k}: two runs differ"
    c = {k: v.cpu() for k, v in o.items()}
    # latent: the project's bound for this stage
    lat = c["latent"].reshape(-1, 256)
    d = np.abs(lat[::7].numpy() - golden[f"{tag}.latent_sample"]).max()
    print(f"[{tag}] latent max|diff| = {d:.3e}")
    assert d < 1e-4
    # indices wherever the reference's fp64 top-2 gap exceeds 1e-5 (~100 x the fp32 rounding of the expanded distance at |x|^2 ~ 0.17)
    safe = golden[f"{tag}.gap64"] > golden["gap"][0]
    got = c["idx"].reshape(-1).numpy()
    flips = int((got != golden[f"{tag}.idx"].reshape(-1)).sum())
    print(f"[{tag}] compared {100 * safe.mean():.1f} % of the tokens; {flips} indices differ over all tokens")
    assert safe.mean() >= 0.90
    assert np.array_equal(got[safe], golden[f"{tag}.idx"].reshape(-1)[safe])
    assert len(np.unique(got)) >= 40
    # pose against the restatement fed the device's own latent and indices (near-tie flips move the pose)
    with torch.no_grad():
        r = T.roundtrip(pose, enc, tok, CFG, latent=c["latent"], idx=c["idx"])
    d = (c["pose6d"] - r["pose6d"]).abs().max().item()
    print(f"[{tag}] pose6d max|diff| = {d:.3e}")
    assert d < 1e-4
    # the statistics of the device's own latent and indices
    assert torch.equal(c["code_count"].long(), torch.bincount(c["idx"].reshape(-1).long(), minlength=2048))
    assert _rel(c["commit_loss"], r["commit_loss"]) < 1e-5 and _rel(c["perplexity"], r["perplexity"]) < 1e-5
    assert c["commit_loss"].dim() == 0 and c["perplexity"].dim() == 0
    if flips == 0:
        assert _rel(c["perplexity"], golden[f"{tag}.perplexity"]) < 1e-5
    # the rotation outputs are the stand-alone kernels' on the same bits
    from tokenhmr_amd import ops
    assert torch.equal(o["rotmat"].reshape(-1, 3, 3), ops.rot6d_to_rotmat(o["pose6d"]))
    assert torch.equal(o["aa"].reshape(-1, 3), ops.rotmat_to_aa(o["rotmat"]))
    # straight-through, not the plain lookup: the two modes differ in the operand (an ulp on ~6 % of its elements)
    plain = eng.vq_decode_idx(o["idx"])
    assert (plain - o["pose6d"]).abs().max() < 1e-5
    # a subset of the outputs, and the latent left in scratch, give the same bits
    few = eng.tokenizer_roundtrip(pose.to(cuda_dev), want=("pose6d", "perplexity"))
    assert set(few) == {"pose6d", "perplexity"} and torch.equal(few["pose6d"], o["pose6d"]) and torch.equal(few["perplexity"], o["perplexity"])
    eng.status()


def test_roundtrip_is_captured_into_a_hip_graph(eng, cuda_dev):
    """thmr_tokenizer_roundtrip allocates nothing and never synchronises the host: captured through torch.cuda.CUDAGraph as the forward
    is in tests/test_gpu_pipeline.py, the replay reproduces the eager call bit for bit, with new inputs between replays."""
    B = 3
    want = ("idx", "latent", "pose6d", "rotmat", "aa", "commit_loss", "perplexity", "code_count")
    poses = [make_pose(B, 40 + i).to(cuda_dev) for i in range(3)]
    ref = [{k: v.clone() for k, v in eng.tokenizer_roundtrip(p, want=want).items()} for p in poses]
    eng.status()
    buf = poses[0].clone()
    outs = {k: torch.zeros_like(v) for k, v in ref[0].items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eng.tokenizer_roundtrip(buf, want=want, outputs=outs)                     # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        eng.tokenizer_roundtrip(buf, want=want, outputs=outs)
    for rep in range(2):
        for p, w in zip(poses, ref):
            buf.copy_(p)
            for k in want:
                outs[k].zero_()
            graph.replay()
            torch.cuda.synchronize()
            for k in want:
                assert torch.equal(outs[k], w[k]), (rep, k)
    eng.status()


def test_roundtrip_guards(built_lib, cuda_dev, state):
    from dataclasses import replace
    from tokenhmr_amd._cabi import EngineError
    from tokenhmr_amd.engine import Engine
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    pose = make_pose(2, 1).to(cuda_dev)
    e = _engine(state, cuda_dev, max_batch=2, encoder=False)
    with pytest.raises(EngineError, match="encoder"):                          # the encoder half is absent: a loud error, no fallback
        e.tokenizer_roundtrip(pose)
    assert e.vq_decode_idx(torch.zeros(2, 160, dtype=torch.int32)).shape == (2, 21, 6)      # the hard decode needs the decoder half only
    with pytest.raises(EngineError, match="batch 3"):
        e.vq_decode_idx(torch.zeros(3, 160, dtype=torch.int32))
    with pytest.raises(ValueError):
        e.vq_decode_idx(torch.zeros(2, 100, dtype=torch.int32))
    e.close()
    hcfg = replace(CFG, head="hmr2")
    h = Engine(hcfg, max_batch=2, device=cuda_dev)
    h.load_state(W.make_synthetic_state(hcfg, 0), None)
    h.load_smpl(make_synthetic_smpl(hcfg, 0))
    h.finalize()
    from tokenhmr_amd import _cabi
    from tokenhmr_amd.engine import _ptr, _stream_ptr
    idx, out6 = torch.zeros(2, 160, dtype=torch.int32, device=cuda_dev), torch.zeros(2, 21, 6, device=cuda_dev)
    st = _cabi.TokenizerOut(pose6d=out6.data_ptr())
    import ctypes
    assert h.lib.thmr_vq_decode_idx(h.h, _ptr(idx), 2, _ptr(out6), _stream_ptr(cuda_dev)) != 0
    assert b"thmr_vq_decode_idx does not exist" in h.lib.thmr_last_error(h.h)
    assert h.lib.thmr_tokenizer_roundtrip(h.h, _ptr(pose), 2, ctypes.byref(st), _stream_ptr(cuda_dev)) != 0
    assert b"thmr_tokenizer_roundtrip does not exist" in h.lib.thmr_last_error(h.h)
    from tokenhmr_amd.tokenizer import VanillaTokenizer
    with pytest.raises(EngineError, match="HMR2"):                              # the drop-in on an HMR2 engine: refused by the library
        VanillaTokenizer(engine=h)(pose)
    h.close()


# ------------------------------------------------------------------------------------------------ 3. the statistics kernel alone
def _stats_ref(x, cb, idx, counts=None):
    commit, perp, c = T.quantizer_stats(x.double(), cb.double(), idx, counts)
    return float(commit), float(perp), c


def test_vq_stats_on_the_fixture(cuda_dev, built_lib, golden, state):
    from tokenhmr_amd import ops
    _, tok = state
    cb = tok["quantizer.codebook"].to(cuda_dev)
    x = torch.from_numpy(golden["b2.latent"]).reshape(-1, 256).to(cuda_dev)
    idx = torch.from_numpy(golden["b2.idx"]).reshape(-1).to(cuda_dev)
    commit, perp, counts = ops.vq_stats(x, cb, idx)
    print(f"commit {float(commit):.6e} (reference {float(golden['b2.commit_loss']):.6e}), perplexity {float(perp):.6f} "
          f"(reference {float(golden['b2.perplexity']):.6f})")
    assert commit.dim() == 0 and perp.dim() == 0 and commit.is_cuda
    assert _rel(commit, golden["b2.commit_loss"]) < 1e-5 and _rel(perp, golden["b2.perplexity"]) < 1e-5
    want = np.zeros(2048, dtype=np.int32)
    want[golden["b2.code_ids"]] = golden["b2.code_counts"]
    assert np.array_equal(counts.cpu().numpy(), want)


@pytest.mark.parametrize("case", ["one row", "every code once", "one code", "160 x 8 rows", "33 rows"])
def test_vq_stats_edge_shapes(cuda_dev, built_lib, golden, state, case):
    from tokenhmr_amd import ops
    _, tok = state
    cb = tok["quantizer.codebook"]
    g = torch.Generator().manual_seed(90)
    if case == "one row":
        idx = torch.tensor([1234])
    elif case == "every code once":
        idx = torch.randperm(2048, generator=g)
    elif case == "one code":
        idx = torch.full((777,), 2047)
    elif case == "160 x 8 rows":
        idx = torch.randint(0, 2048, (1280,), generator=g)
    else:
        idx = torch.randint(0, 64, (33,), generator=g)            # one row into a second workgroup; repeated codes
    rows = idx.numel()
    x = cb[idx] + 5e-3 * torch.randn(rows, 256, generator=g)      # latents a commit distance of the fixture's size away from their codes
    commit, perp, counts = ops.vq_stats(x.to(cuda_dev), cb.to(cuda_dev), idx.to(cuda_dev, torch.int32))
    rc, rp, rcount = _stats_ref(x, cb, idx)
    print(f"[{case}] commit {float(commit):.6e} / {rc:.6e}, perplexity {float(perp):.7f} / {rp:.7f}")
    assert torch.equal(counts.cpu().long(), rcount)
    assert _rel(commit, rc) < 1e-5 and _rel(perp, rp) < 1e-5
    if case == "one code":
        assert _rel(perp, 0.99999988) < 1e-5                      # what the reference's fp32 yields: log(1 + 1e-7) is one ulp
    if case == "every code once":
        assert _rel(perp, 2048.0) < 1e-3                          # uniform usage: the codebook size, less the 1e-7 term's 2048e-7 in the exponent
    # two runs are bit-equal
    c2, p2, n2 = ops.vq_stats(x.to(cuda_dev), cb.to(cuda_dev), idx.to(cuda_dev, torch.int32))
    assert torch.equal(c2, commit) and torch.equal(p2, perp) and torch.equal(n2, counts)


def test_vq_stats_accumulates(cuda_dev, built_lib, state):
    from tokenhmr_amd import ops
    _, tok = state
    cb = tok["quantizer.codebook"]
    g = torch.Generator().manual_seed(91)
    idx = torch.randint(0, 300, (160 * 3 + 5,), generator=g)
    x = cb[idx] + 5e-3 * torch.randn(idx.numel(), 256, generator=g)
    xd, cbd, idd = x.to(cuda_dev), cb.to(cuda_dev), idx.to(cuda_dev, torch.int32)
    c_all, p_all, n_all = ops.vq_stats(xd, cbd, idd)
    k = 160 * 2
    counts = torch.full((2048,), 7, device=cuda_dev, dtype=torch.int32)      # overwritten by a call without accumulate
    c1, p1, _ = ops.vq_stats(xd[:k], cbd, idd[:k], code_count=counts)
    c2, p2, _ = ops.vq_stats(xd[k:], cbd, idd[k:], code_count=counts, accumulate=True)
    assert torch.equal(counts, n_all)
    assert torch.equal(p2, p_all)                                            # the perplexity of the summed histogram, bit for bit
    rows = idx.numel()
    merged = float(c1) * (k / rows) + float(c2) * ((rows - k) / rows)
    assert _rel(merged, c_all) < 1e-6                                        # rows-weighted means: equal up to fp32 rounding of the sums
    assert _rel(p1, _stats_ref(x[:k], cb, idx[:k])[1]) < 1e-5


# ------------------------------------------------------------------------------------------------ 4. matrix_to_axis_angle
def test_rotmat_to_aa_against_the_reference(cuda_dev, built_lib, golden):
    """Against the reference's function on the same input bits, on the fixture's branch set.  Bound per group of the set:
    max(1e-6, 2 x the reference's own fp32-vs-float64 distance on that group), per element — the project's rule for joints / vertices."""
    from tokenhmr_amd import ops
    R, spans = G.rotation_set(torch.from_numpy(golden["rot.special"]))
    a, b = spans["random"]
    assert abs(G.rotation_checksum(R[a:b]) - golden["rot.random_checksum"][0]) <= 1e-12 * abs(golden["rot.random_checksum"][0])
    got = ops.rotmat_to_aa(R.to(cuda_dev)).cpu()
    ref = torch.from_numpy(golden["rot.aa"])
    own = json.loads(str(golden["rot.ref32_vs_f64"]))
    assert got.shape == ref.shape == (R.shape[0], 3)
    assert int(golden["rot.q0_negative"][0]) > 0 and int((got.norm(dim=-1) > G.ABOVE_PI).sum()) == int(golden["rot.angle_above_pi"][0])
    worst = {}
    for name, (s, e) in spans.items():
        worst[name] = ((got[s:e] - ref[s:e]).abs().max().item(), max(1e-6, 2.0 * own[name]))
    print("rotmat_to_aa max|diff| (bound): " + ", ".join(f"{k} {d:.2e} ({bd:.1e})" for k, (d, bd) in worst.items()))
    for name, (d, bd) in worst.items():
        assert d <= bd, (name, d, bd)
    assert torch.equal(got[spans["identity"][0]], torch.zeros(3))
    # one matrix, and a batch shape
    assert torch.equal(ops.rotmat_to_aa(R[40:41].to(cuda_dev)).cpu(), got[40:41])
    assert torch.equal(ops.rotmat_to_aa(R[:42].view(2, 21, 3, 3).to(cuda_dev)).cpu(), got[:42])


# ------------------------------------------------------------------------------------------------ 5. the drop-in
def test_vanilla_tokenizer_dropin(built_lib, cuda_dev, tmp_path, golden, state):
    """VanillaTokenizer on a file in the reference's format, built the way train_poseVQ.py:63-66 builds it; 9 poses at max_batch=4 are
    three chunks whose merged statistics must be a single max_batch=16 engine's."""
    from _ref_files import write_reference_files
    from tokenhmr_amd import ckpt_io
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.tokenizer import VanillaTokenizer, EncodeTokens
    enc, tok = state
    ck, yml = write_reference_files(tmp_path, CFG, W.make_synthetic_state(CFG, 0), dict(tok, **enc), make_synthetic_smpl(CFG, 0))
    path = str(tmp_path / "tokenizer.pth")
    ckpt = ckpt_io.load_checkpoint(path)
    net = VanillaTokenizer(ckpt["hparams"].ARCH, mesh_inference=True, device=cuda_dev, max_batch=4)
    net.load_state_dict(ckpt["net"], strict=True)
    assert net.cuda() is net and net.eval() is net
    pose = make_pose(9, 2)
    out, commit, perp = net(pose.to(cuda_dev))
    assert set(out) == {"pred_pose_body_6d", "pred_pose_body_rotmat", "pred_pose_body_aa"}          # no body model: no mesh keys
    assert out["pred_pose_body_6d"].shape == (9, 21, 6) and out["pred_pose_body_rotmat"].shape == (9, 21, 3, 3)
    assert out["pred_pose_body_aa"].shape == (9, 63) and all(v.is_cuda and v.dtype == torch.float32 for v in out.values())
    assert commit.dim() == 0 and perp.dim() == 0 and commit.is_cuda and perp.is_cuda
    counts = net.code_count.clone()
    assert int(counts.sum()) == 9 * 160
    # (B,21,3,3) input: the first two rows are taken
    R = torch.zeros(9, 21, 3, 3)
    R[:, :, :2, :] = pose.view(9, 21, 2, 3)
    R[:, :, 2, :] = 99.0
    out_r, commit_r, perp_r = net(R.to(cuda_dev))
    assert all(torch.equal(out[k], out_r[k]) for k in out) and torch.equal(commit, commit_r) and torch.equal(perp, perp_r)
    # one engine that holds the batch whole: the same histogram, perplexity and (to fp32 rounding) commit loss
    big = VanillaTokenizer(ckpt_path=path, mesh_inference=False, device=cuda_dev, max_batch=16)
    out_b, commit_b, perp_b = big(pose.to(cuda_dev))
    assert set(out_b) == {"pred_pose_body_6d", "pred_pose_body_rotmat"}
    assert torch.equal(big.code_count, counts)
    assert torch.equal(perp, perp_b)
    print(f"commit {float(commit):.8e} (3 chunks) / {float(commit_b):.8e} (one call); perplexity {float(perp):.5f}")
    assert _rel(commit, commit_b) < 1e-6
    assert (out["pred_pose_body_6d"] - out_b["pred_pose_body_6d"]).abs().max() < 1e-4      # tiny-M (4 poses) and tile (9) regimes of the decoder
    with torch.no_grad():
        r = T.roundtrip(pose, enc, tok, CFG)
    assert len(np.unique(r["idx"].numpy())) >= 40
    assert _rel(commit_b, r["commit_loss"]) < 1e-3              # a near-tie flip moves a token's distance by less than its top-2 gap
    # encode / decode
    idx = net.encode(pose.to(cuda_dev))
    assert idx.dtype == torch.int64 and idx.shape == (9, 160)
    assert torch.equal(idx.reshape(-1), EncodeTokens(engine=big.engine)(pose.to(cuda_dev)))
    assert torch.equal(torch.bincount(idx.reshape(-1), minlength=2048).to(torch.int32), counts)
    dec = net.decode(idx)
    assert dec.shape == (9, 21, 6) and (dec - out["pred_pose_body_6d"]).abs().max() < 1e-5
    assert torch.equal(big.decode(idx), big.engine.vq_decode_idx(idx))
    # sharing the engine of a loaded model (its tokenizer file holds both halves); a body model, when given, supplies the mesh keys
    from tokenhmr_amd.model import load_tokenhmr
    model, _ = load_tokenhmr(ck, yml, max_batch=16, device=cuda_dev)
    body = lambda body_pose: types.SimpleNamespace(vertices=body_pose.sum((2, 3)), joints=body_pose[:, :, 0])     # noqa: E731
    shared = VanillaTokenizer(engine=model.engine, mesh_inference=True, body_model=body)
    assert shared.max_batch == 16 and shared.device == model.engine.device
    out_s, commit_s, perp_s = shared(pose.to(cuda_dev))
    assert torch.equal(out_s["pred_pose_body_6d"], out_b["pred_pose_body_6d"]) and torch.equal(commit_s, commit_b) and torch.equal(perp_s, perp_b)
    assert {"pred_body_mesh", "pred_body_vertices", "pred_body_joints"} <= set(out_s) and out_s["pred_body_joints"].shape == (9, 21, 3)
    with pytest.raises(ValueError, match="shares"):
        shared.load_state_dict(ckpt["net"])
    with pytest.raises(ValueError):
        net(torch.zeros(2, 21, 4, device=cuda_dev))
    with pytest.raises(NotImplementedError):
        net.train()
    net.engine.status()
    big.engine.status()
    model.engine.status()
    net.engine.close()
    big.engine.close()
