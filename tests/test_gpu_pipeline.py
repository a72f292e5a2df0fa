"""End-to-end (-m gpu): the loop body of the reference's eval.py / demo.py with every GPU drop-in at once —
frame + boxes -> crops (N2, tokenhmr_amd.preprocess) -> TokenHMR forward (the hot path) -> metrics against ground-truth
meshes (N1 evaluator, N3 stand-alone SMPL) — compared with the same pipeline assembled from the CPU oracles
(oracle.crop_oracle -> oracle.tokenhmr_oracle.forward -> oracle.eval_oracle).  north_star asks MPJPE parity within
+-0.1 mm; asserted here at 0.02 mm."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

if os.path.join(ROOT, "scripts") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_golden_prof_accounting as PA      # noqa: E402

pytestmark = pytest.mark.gpu

KP = [25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 43]      # 3DPW-TEST keypoint list (datasets_eval.yaml:12)


class _N(dict):
    __getattr__ = dict.__getitem__


def test_eval_loop_with_all_dropins(built_lib, cuda_dev):
    from oracle import crop_oracle as CO, eval_oracle as EO, tokenhmr_oracle as O
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.model import TokenHMR
    from tokenhmr_amd.preprocess import ViTDetDataset
    from tokenhmr_amd.evaluator import Evaluator
    from tokenhmr_amd.smpl import SMPL

    cfg = HMRConfig(vit_depth=2, dec_depth=2)
    sd, tok, smpl = W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0), make_synthetic_smpl(cfg, 0)
    model = TokenHMR.from_state(cfg, sd, tok, smpl, max_batch=8, device=cuda_dev)
    mcfg = _N(MODEL=_N(IMAGE_SIZE=256, IMAGE_MEAN=[0.485, 0.456, 0.406], IMAGE_STD=[0.229, 0.224, 0.225], BBOX_SHAPE=[192, 256]))

    rng = np.random.default_rng(21)
    H, Wd = 720, 1280
    yy, xx = np.mgrid[0:H, 0:Wd]
    frame = np.clip(np.stack([120 + 90 * np.sin(xx / 43.0 + c) * np.cos(yy / 31.0) for c in range(3)], -1)
                    + rng.normal(0, 15, (H, Wd, 3)), 0, 255).astype(np.uint8)
    boxes = np.array([[100, 80, 400, 700], [500, 10, 1270, 715], [-50, 300, 300, 760], [900, 200, 1000, 420], [300, 100, 620, 400]], float)
    n = len(boxes)

    # ground truth: random SMPL parameters -> meshes / joints on the GPU (N3), and by the restated smplx on the CPU
    g = torch.Generator().manual_seed(5)
    gt_pose = 0.3 * torch.randn(n, 72, generator=g)
    gt_betas = torch.randn(n, 10, generator=g)
    gt_model = SMPL(smpl, max_batch=8, device=cuda_dev)
    gt_gpu = gt_model(global_orient=gt_pose[:, :3], body_pose=gt_pose[:, 3:], betas=gt_betas)
    gt_v_cpu, gt_j_cpu = O.smpl_forward_axis_angle(gt_pose[:, :3], gt_pose[:, 3:], gt_betas, smpl)
    assert (gt_gpu.vertices.cpu() - gt_v_cpu).abs().max() < 1e-4

    # ---- GPU pipeline (what eval.py / demo.py run after the three import swaps)
    batch = ViTDetDataset(mcfg, frame, boxes, device=cuda_dev).batch()
    with torch.no_grad():
        out = model(batch)
    ones = torch.ones(n, 44, 1, device=cuda_dev)
    ev = Evaluator(int(1e8), KP, 39, metrics=["mode_re", "mode_mpjpe", "mode_pve"], dataset="3DPW-TEST")
    ev(out, {"imgname": [f"f{i}" for i in range(n)], "keypoints_3d": torch.cat([gt_gpu.joints, ones], -1), "vertices": gt_gpu.vertices})
    got = ev.get_metrics_dict()

    # ---- the same pipeline from the CPU oracles
    imgs = torch.from_numpy(np.stack([CO.vitdet_item(frame, b, 256, [192, 256])["img"] for b in boxes]))
    assert (batch["img"].cpu() - imgs).abs().max() < 2e-6
    with torch.no_grad():
        ref = O.forward(imgs, sd, tok, smpl, cfg)
    mp, re, pve = EO.evaluate_batch(ref["pred_keypoints_3d"], ref["pred_vertices"], torch.cat([gt_j_cpu, torch.ones(n, 44, 1)], -1),
                                    gt_v_cpu, KP, 39)
    print("GPU pipeline:", got, "| oracle pipeline:", float(mp.mean()), float(re.mean()), float(pve.mean()))
    assert abs(got["mode_mpjpe"] - float(mp.mean())) < 0.02
    assert abs(got["mode_re"] - float(re.mean())) < 0.02
    assert abs(got["mode_pve"] - float(pve.mean())) < 0.02
    top2 = ref["cls_logits"].topk(2, dim=-1).values
    safe = (top2[..., 0] - top2[..., 1]) > 1e-2
    assert (out["token_idx"].cpu() == ref["token_idx"])[safe].all()


def test_track_py_style_sliced_input(built_lib, cuda_dev):
    """track.py:33-39 hands the model a NON-contiguous view: batch['img'] = x[:, :3] of a 4-channel (RGB + mask) crop."""
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.model import TokenHMR
    cfg = HMRConfig(vit_depth=1, dec_depth=1)
    model = TokenHMR.from_state(cfg, W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0), make_synthetic_smpl(cfg, 0),
                                max_batch=4, device=cuda_dev)
    x = torch.randn(3, 4, 256, 256, generator=torch.Generator().manual_seed(2)).to(cuda_dev)
    view = x[:, :3, :, :]
    assert not view.is_contiguous()
    a, b = model({"img": view, "mask": x[:, 3].clip(0, 1)}), model({"img": view.contiguous()})
    assert torch.equal(a["pred_vertices"], b["pred_vertices"]) and torch.equal(a["pred_cam"], b["pred_cam"])
    assert set(a["pred_smpl_params"]) == {"global_orient", "body_pose", "betas"}


def test_second_engine_shares_the_weight_arena(built_lib, cuda_dev):
    """Several engines on one GPU (e.g. one per caller thread / stream) can share one packed weight arena: the second engine
    only adds its scratch.  Results are bit-identical, also when both run concurrently on two streams."""
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.engine import Engine
    cfg = HMRConfig(vit_depth=2, dec_depth=2)
    e1 = Engine(cfg, max_batch=4, device=cuda_dev)
    e1.load_state(W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0))
    e1.load_smpl(make_synthetic_smpl(cfg, 0))
    e1.finalize()
    img = torch.randn(4, 3, 256, 256, generator=torch.Generator().manual_seed(3)).to(cuda_dev)
    # the reference result is taken BEFORE the second engine exists: creating / finalising e2 must not touch e1's weights
    # (round 1 zeroed the read-out rows of a shared arena in thmr_create and this test compared corrupted with corrupted)
    ref = {k: v.clone() for k, v in e1.forward(img).items()}
    torch.cuda.synchronize()
    arena_before = e1.weight_arena.clone()
    e2 = Engine(cfg, max_batch=4, device=cuda_dev, weight_arena=e1.weight_arena)
    e2.finalize(assume_all_loaded=True)
    torch.cuda.synchronize()
    assert torch.equal(arena_before, e1.weight_arena), "creating a second engine on a shared arena modified the weights"
    del arena_before
    # and the read-outs are not the bias-only values a zeroed read-out matrix would give
    assert (ref["pred_cam"] - ref["pred_cam"][0]).abs().max() > 0
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a = e1.forward(img)
    with torch.cuda.stream(s2):
        b = e2.forward(img)
    torch.cuda.synchronize()
    for k in ("pred_vertices", "pred_keypoints_3d", "token_idx"):
        assert torch.equal(a[k], ref[k]) and torch.equal(b[k], ref[k]), k
    with pytest.raises(ValueError):
        Engine(HMRConfig(vit_depth=1, dec_depth=1), max_batch=4, device=cuda_dev, weight_arena=e1.weight_arena)


def test_creation_flags_and_shared_split_weights(built_lib, cuda_dev):
    """ABI 5.  (1) An engine CREATED in the opt-out mode (vit_gemm="f32" -> THMR_CFG_VIT_GEMM_F32) finalizes without building
    any split3 copy: device memory grows by the arenas only, results = the default engine switched to "f32".  (2) Engines that share a
    weight arena share ONE split3 weight copy: the second engine's finalize allocates its activation operands only.  (3) An engine
    created without the co-residency-dependent kernels (persistent=False -> THMR_CFG_NO_PERSISTENT: launch-chain head, per-tile split3
    GEMMs) gives the default engine's ViT features bit for bit and its outputs to fp32 summation-order differences (the launch-chain head
    associates its sums differently from the persistent decoder kernel: test_head_regimes_agree_and_persistent_decoders_coexist)."""
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.engine import Engine
    cfg = HMRConfig(vit_depth=2, dec_depth=2)
    sd, tok, smpl = W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0), make_synthetic_smpl(cfg, 0)
    img = torch.randn(40, 3, 256, 256, generator=torch.Generator().manual_seed(5)).to(cuda_dev)

    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info(cuda_dev)
        return total - free

    def make(**kw):
        e = Engine(cfg, max_batch=40, device=cuda_dev, **kw)
        if "weight_arena" not in kw:
            e.load_state(sd, tok)
            e.load_smpl(smpl)
        return e

    keys = ("pred_vertices", "pred_keypoints_3d", "token_idx", "cls_logits_softmax")
    # (1) created in the opt-out mode
    f = make(vit_gemm="f32")
    assert f.vit_gemm() == "f32" and f.mode_bytes() == {"split_weights": 0, "split_activations": 0, "workspace": 0}
    before = used()
    f.finalize()
    grown = used() - before
    assert grown <= 64 * 2 ** 20, f"finalize of an engine created in the f32 mode allocated {grown} bytes"      # (allocator granularity: 0-8 MiB measured; the split copies would be ~0.3 GB here)
    out_f = {k: v.clone() for k, v in f.forward(img).items()}
    # default engine: finalize builds the copies thmr_mode_bytes announces
    d = make()
    mb = d.mode_bytes()
    assert d.vit_gemm() == "split3" and mb["split_weights"] > 0 and mb["split_activations"] > 0
    before = used()
    d.finalize()
    grown = used() - before
    want = mb["split_weights"] + mb["split_activations"] + mb["workspace"]
    assert want <= grown <= want + 64 * 2 ** 20, (grown, mb)
    out_d = {k: v.clone() for k, v in d.forward(img).items()}
    d.set_vit_gemm("f32")
    out_df = d.forward(img)
    for k in keys:
        assert torch.equal(out_df[k], out_f[k]), k
    d.set_vit_gemm("split3")
    # (2) a second engine on the same arena: activations (+ workspace) only
    before = used()
    d2 = make(weight_arena=d.weight_arena)
    d2.finalize(assume_all_loaded=True)
    grown = used() - before
    own = d2.scratch_bytes + mb["split_activations"] + mb["workspace"]
    assert grown <= own + 64 * 2 ** 20 and grown < own + mb["split_weights"] // 2, (grown, own, mb)
    out_d2 = d2.forward(img)
    for k in keys:
        assert torch.equal(out_d2[k], out_d[k]), k
    d2.close()                                                   # the shared copy outlives one of its holders
    out_d3 = d.forward(img)
    torch.cuda.synchronize()
    assert torch.equal(out_d3["pred_vertices"], out_d["pred_vertices"])
    # (3) no persistent kernels
    n = make(persistent=False)
    assert n.mode_bytes()["workspace"] == 0
    n.finalize()
    for b in (40, 8, 3):
        o_n, o_d = n.forward(img[:b], taps=True), d.forward(img[:b], taps=True)
        assert torch.equal(o_n["vit_features"], o_d["vit_features"]), b
        assert (o_n["pred_vertices"] - o_d["pred_vertices"]).abs().max() < 1e-4, b
        assert (o_n["cls_logits_softmax"] - o_d["cls_logits_softmax"]).abs().max() < 1e-5, b
    n.status()
    d.status()
    for e in (f, d, n):
        e.close()
    torch.cuda.empty_cache()


def test_run_eval_loop_matches_manual_loop(built_lib, cuda_dev):
    """tokenhmr_amd.eval_dp.run_eval (eval.py:116-158 as a shardable job) on one process = the hand-written loop, for any
    batch size (per-sample metrics, so batching cannot change the means beyond fp32 regime differences)."""
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.model import TokenHMR
    from tokenhmr_amd.evaluator import Evaluator
    from tokenhmr_amd.eval_dp import run_eval, recursive_to

    cfg = HMRConfig(vit_depth=1, dec_depth=1)
    model = TokenHMR.from_state(cfg, W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0), make_synthetic_smpl(cfg, 0),
                                max_batch=16, device=cuda_dev)
    n = 19
    g = torch.Generator().manual_seed(17)
    imgs = torch.randn(n, 3, 256, 256, generator=g)
    kp3d = torch.cat([0.3 * torch.randn(n, 44, 3, generator=g), torch.ones(n, 44, 1)], -1)
    verts = 0.3 * torch.randn(n, 6890, 3, generator=g)

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return n

        def __getitem__(self, i):
            return {"img": imgs[i], "keypoints_3d": kp3d[i], "vertices": verts[i], "imgname": f"im{i:03d}", "idx": i}

    def make_ev():
        return Evaluator(int(1e6), KP, 39, metrics=["mode_re", "mode_mpjpe", "mode_pve"], dataset="3DPW-TEST")

    ev_a, ev_b, ev_m = make_ev(), make_ev(), make_ev()
    a = run_eval(model, DS(), ev_a, batch_size=8, device=cuda_dev)
    b = run_eval(model, DS(), ev_b, batch_size=16, device=cuda_dev)
    for s in range(0, n, 8):
        batch = recursive_to({"img": imgs[s:s + 8], "keypoints_3d": kp3d[s:s + 8], "vertices": verts[s:s + 8],
                              "imgname": [f"im{i:03d}" for i in range(s, min(n, s + 8))]}, cuda_dev)
        ev_m(model(batch), batch)
    m = ev_m.get_metrics_dict()
    assert ev_a.counter == n and ev_a.get_imgnames() == [f"im{i:03d}" for i in range(n)] == ev_m.get_imgnames()
    for k in m:
        assert a[k] == m[k], (k, a[k], m[k])                      # same batches -> same bits
        assert abs(b[k] - m[k]) < 1e-3, (k, b[k], m[k])           # other batching: mm-scale metrics agree to 1e-3 mm
    assert np.isfinite(list(m.values())).all() and m["mode_mpjpe"] > 0


def test_head_regimes_agree_and_persistent_decoders_coexist(built_lib, cuda_dev):
    """The head has two regimes (csrc/engine_paths.hip kFusedHeadMaxB): up to 128 crops the persistent decoder kernel + the
    one-workgroup-per-crop mixer kernel, above it the chain of tiled GEMMs.  (1) Both must agree with the CPU oracle, and a crop
    must get the same answer (to fp32 summation-order differences) whichever regime its batch falls in.  (2) Two engines that
    launch their persistent decoder kernels concurrently on two streams at a batch size where EACH asks for every CU (>= 49
    crops) must both finish (the per-device turnstile chains them) with bit-identical results and no barrier timeout."""
    from oracle import tokenhmr_oracle as O
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.engine import Engine
    cfg = HMRConfig(vit_depth=1, dec_depth=6)
    sd, tok, smpl = W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0), make_synthetic_smpl(cfg, 0)
    e1 = Engine(cfg, max_batch=136, device=cuda_dev)
    e1.load_state(sd, tok)
    e1.load_smpl(smpl)
    e1.finalize()
    img = torch.randn(136, 3, 256, 256, generator=torch.Generator().manual_seed(11))
    d = img.to(cuda_dev)
    big = {k: v.clone() for k, v in e1.forward(d, taps=True).items()}            # 136 crops: chain-of-GEMMs regime
    small = {k: v.clone() for k, v in e1.forward(d[:64], taps=True).items()}     # 64 crops: fused regime
    e1.status()
    with torch.no_grad():
        orc = O.forward(img[:4], sd, tok, smpl, cfg)
    for o, tag in ((big, "chain"), (small, "fused")):
        assert (o["token_out"][:4].cpu() - orc["token_out"]).abs().max() < 1e-3, tag
        assert (o["cls_logits"][:4].cpu() - orc["cls_logits"]).abs().max() < 1e-3, tag
        assert (o["pred_vertices"][:4].cpu() - orc["pred_vertices"]).abs().max() < 1e-4, tag
    assert (big["pred_vertices"][:64] - small["pred_vertices"]).abs().max() < 1e-4
    assert (big["cls_logits_softmax"][:64] - small["cls_logits_softmax"]).abs().max() < 1e-5
    # (2) two engines, two streams, 64 crops each -> two 256-workgroup persistent kernels in flight
    e2 = Engine(cfg, max_batch=64, device=cuda_dev, weight_arena=e1.weight_arena)
    e2.finalize(assume_all_loaded=True)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            a = e1.forward(d[:64])
        with torch.cuda.stream(s2):
            b = e2.forward(d[:64])
        outs.append((a, b))
    torch.cuda.synchronize()
    e1.status()
    e2.status()
    for a, b in outs:
        for k in ("pred_vertices", "token_idx", "pred_cam"):
            assert torch.equal(a[k], small[k]) and torch.equal(b[k], small[k]), k


@pytest.mark.parametrize("mode", ["split3", "f32"])
def test_fused_head_equals_chain_head_across_batch_sizes(built_lib, cuda_dev, monkeypatch, mode):
    """The persistent decoder kernel picks its grid from the batch (64 workgroups up to 16 crops, 128 / 192 / 256 above) and
    deals (column tile x 16-row sub-tile) items over it; the mixer stack runs inside that kernel, ten workgroups per crop, up to 25
    crops and as its own kernel, one workgroup per crop, above (bit-identical by construction: both call mixer_device.h).  For
    batch sizes on both sides of every boundary — 1, 2, 6, 7, 15, 16, 17, 25, 26, 33, 48, 49, 64, 100, 128 (ragged last sub-tiles
    included) — the fused head must
    agree with the chain-of-GEMMs head (THMR_LEGACY_HEAD=1: same maths as separate tiled launches, the round-1 path) to fp32
    summation-order differences, be deterministic, and give a crop the same bits whatever batch it rides in.
    Both modes of the engine: in the default "split3" mode the decoder's stacked to_kv GEMM runs on the bf16 pipe from 3 crops on, so one and two
    crops (exact-fp32 to_kv) are a regime of their own there; "f32" is the round-2 regime structure."""
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.engine import Engine
    cfg = HMRConfig(vit_depth=1, dec_depth=6)
    sd, tok, smpl = W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0), make_synthetic_smpl(cfg, 0)
    fused = Engine(cfg, max_batch=128, device=cuda_dev)
    fused.load_state(sd, tok)
    fused.load_smpl(smpl)
    fused.finalize()
    # the forcing knobs exist only in the experiments build of the library (experiments=True); `fused` is the shipped one
    monkeypatch.setenv("THMR_LEGACY_HEAD", "1")          # read once, at thmr_create
    chain = Engine(cfg, max_batch=128, device=cuda_dev, weight_arena=fused.weight_arena, experiments=True)
    chain.finalize(assume_all_loaded=True)
    monkeypatch.delenv("THMR_LEGACY_HEAD")
    monkeypatch.setenv("THMR_MIXER_CLUSTER", "0")        # the mixer stack as its own kernel, one workgroup per crop, at every batch size
    plain = Engine(cfg, max_batch=128, device=cuda_dev, weight_arena=fused.weight_arena, experiments=True)
    plain.finalize(assume_all_loaded=True)
    monkeypatch.delenv("THMR_MIXER_CLUSTER")
    for e in (fused, chain, plain):
        assert e.vit_gemm() == "split3"                                   # the creation default (ABI 4)
        e.set_vit_gemm(mode)
    ctx = torch.randn(128, 192, 1280, generator=torch.Generator().manual_seed(12)).to(cuda_dev)
    keys = ("token_out", "cls_logits", "pose6d", "pred_vertices", "pred_cam")
    ref128 = {k: v.clone() for k, v in fused.head_forward(ctx, taps=True).items()}
    ref6 = {k: v.clone() for k, v in fused.head_forward(ctx[:6], taps=True).items()}
    ref2 = {k: v.clone() for k, v in fused.head_forward(ctx[:2], taps=True).items()}
    if mode == "split3":      # one and two crops: exact-fp32 to_kv, fp32-rounding-close to the bf16-pipe product of the larger batches
        assert (ref2["token_out"] - ref6["token_out"][:2]).abs().max() < 1e-4 and not torch.equal(ref2["token_out"], ref6["token_out"][:2])
    else:
        assert torch.equal(ref2["token_out"], ref6["token_out"][:2])
    # up to six crops the VQ decoder's GEMMs run on the tiny-M kernel (another association of the K sum): its own regime.  What comes
    # BEFORE the VQ decoder (decoder, mixers, logits) is the same arithmetic in both regimes.
    for k in ("token_out", "cls_logits"):
        assert torch.equal(ref6[k], ref128[k][:6]), k
    assert (ref6["pred_vertices"] - ref128["pred_vertices"][:6]).abs().max() < 1e-5
    assert (ref6["pose6d"] - ref128["pose6d"][:6]).abs().max() < 1e-5
    for B in (1, 2, 6, 7, 15, 16, 17, 25, 26, 33, 48, 49, 64, 100, 128):
        a = {k: v.clone() for k, v in fused.head_forward(ctx[:B], taps=True).items()}
        b = fused.head_forward(ctx[:B], taps=True)
        c = chain.head_forward(ctx[:B], taps=True)
        ref = (ref2 if (B <= 2 and mode == "split3") else ref6) if B <= 6 else ref128
        for k in keys:
            assert torch.equal(a[k], b[k]), (B, k)                                   # deterministic
            assert torch.equal(a[k], ref[k][:B]), (B, k)                             # batch-invariant within a regime of the fused head
        if B in (1, 6, 25, 26, 49, 128):                                             # 10 / 5 / 2 workgroups per crop == one workgroup per crop
            d = plain.head_forward(ctx[:B], taps=True)
            for k in keys:
                assert torch.equal(a[k], d[k]), (B, k)
        assert (a["token_out"] - c["token_out"]).abs().max() < 1e-4, B
        assert (a["cls_logits"] - c["cls_logits"]).abs().max() < 1e-4, B
        assert (a["pred_vertices"] - c["pred_vertices"]).abs().max() < 1e-5, B
        assert (a["token_idx"] != c["token_idx"]).float().mean() < 0.01, B           # only near-tie tokens may differ between regimes
    fused.status()
    chain.status()
    plain.status()


def test_decoder_timeout_is_reported_once_and_the_engine_recovers(built_lib, cuda_dev, monkeypatch):
    """when the persistent decoder kernel's bounded grid barrier times out, the sticky error word used to
    poison every later forward, and thmr_forward kept returning 0.  Now the NEXT forward-type call (host-mapped copy of the word)
    or thmr_engine_status reports it ONCE, the engine resets its barrier words and switches its head to the launch chain (no
    co-residency needed), and a re-submitted batch gives the chain head's bits.  THMR_DEC_FORCE_TIMEOUT=1 makes the kernel report a
    timeout that did not happen (and abandon its work, as a real one does)."""
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W, _cabi
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.engine import Engine
    cfg = HMRConfig(vit_depth=1, dec_depth=2)
    sd, tok, smpl = W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0), make_synthetic_smpl(cfg, 0)
    # THMR_LEGACY_HEAD / THMR_DEC_FORCE_TIMEOUT are hooks of the experiments build (experiments=True); the recovery code they exercise
    # (check_ready / thmr_engine_status -> recover_decoder_timeout) is the shipped library's, compiled from the same source
    monkeypatch.setenv("THMR_LEGACY_HEAD", "1")
    chain = Engine(cfg, max_batch=4, device=cuda_dev, experiments=True)
    chain.load_state(sd, tok)
    chain.load_smpl(smpl)
    chain.finalize()
    monkeypatch.delenv("THMR_LEGACY_HEAD")
    monkeypatch.setenv("THMR_DEC_FORCE_TIMEOUT", "1")          # read at finalize
    a = Engine(cfg, max_batch=4, device=cuda_dev, weight_arena=chain.weight_arena, experiments=True)
    a.finalize(assume_all_loaded=True)
    b = Engine(cfg, max_batch=4, device=cuda_dev, weight_arena=chain.weight_arena, experiments=True)
    b.finalize(assume_all_loaded=True)
    monkeypatch.delenv("THMR_DEC_FORCE_TIMEOUT")
    img = torch.randn(4, 3, 256, 256, generator=torch.Generator().manual_seed(3)).to(cuda_dev)
    ref = {k: v.clone() for k, v in chain.forward(img).items()}
    # (1) reported by the next forward
    a.forward(img)
    torch.cuda.synchronize()
    with pytest.raises(_cabi.EngineError, match="timed out in a previous forward"):
        a.forward(img)
    out = a.forward(img)                                        # re-submit: works, on the chain head
    torch.cuda.synchronize()
    a.status()                                                  # and the error is not sticky
    for k in ("pred_vertices", "pred_cam", "token_idx", "cls_logits_softmax"):
        assert torch.equal(out[k], ref[k]), k
    # (2) reported by thmr_engine_status at the caller's sync point
    b.forward(img)
    with pytest.raises(_cabi.EngineError, match="timed out"):
        b.status()
    b.status()
    out = b.forward(img)
    torch.cuda.synchronize()
    assert torch.equal(out["pred_vertices"], ref["pred_vertices"])


def test_split3_handover_timeout_is_reported_once_and_the_engine_falls_back(built_lib, cuda_dev, monkeypatch):
    """The persistent split3 GEMM hands accumulators from one workgroup to another with a bounded wait; when it runs out (another kernel
    held the device for ~0.5 s) thmr_engine_status reports it ONCE, resets the workspace and switches the engine to the per-tile kernel —
    whose results are the same bits, so the re-submitted batch equals what the persistent kernels give.  THMR_SPLIT3_FORCE_TIMEOUT=1
    (experiments build) makes the status call report a timeout that did not happen."""
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W, _cabi
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.engine import Engine
    if torch.cuda.get_device_properties(cuda_dev).multi_processor_count != 256:
        pytest.skip("the persistent split3 GEMM needs 8 XCDs x 32 CUs")
    cfg = HMRConfig(vit_depth=1, dec_depth=1)
    sd, tok, smpl = W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0), make_synthetic_smpl(cfg, 0)
    good = Engine(cfg, max_batch=32, device=cuda_dev)                    # shipped library, persistent kernels
    good.load_state(sd, tok)
    good.load_smpl(smpl)
    good.finalize()
    assert good.vit_gemm() == "split3"                                   # the creation default (ABI 4)
    img = torch.randn(32, 3, 256, 256, generator=torch.Generator().manual_seed(5)).to(cuda_dev)
    ref = {k: v.clone() for k, v in good.forward(img).items()}
    good.status()
    monkeypatch.setenv("THMR_SPLIT3_FORCE_TIMEOUT", "1")
    e = Engine(cfg, max_batch=32, device=cuda_dev, weight_arena=good.weight_arena, experiments=True)
    e.finalize(assume_all_loaded=True)
    e.forward(img)
    with pytest.raises(_cabi.EngineError, match="hand-over wait timed out"):
        e.status()
    e.status()                                                          # reported once
    out = e.forward(img)                                                # per-tile kernels from here on
    torch.cuda.synchronize()
    e.status()
    for k in ("pred_vertices", "pred_cam", "token_idx", "cls_logits_softmax"):
        assert torch.equal(out[k], ref[k]), k
    # (2) ADVICE r4: the NEXT forward-type call reports it too, without anybody calling status(): a timed-out consumer also writes a
    # host-mapped word that thmr_forward tests on entry (= 2: the experiments build writes that word itself after one forward)
    monkeypatch.setenv("THMR_SPLIT3_FORCE_TIMEOUT", "2")
    f = Engine(cfg, max_batch=32, device=cuda_dev, weight_arena=good.weight_arena, experiments=True)
    f.finalize(assume_all_loaded=True)
    f.forward(img)
    torch.cuda.synchronize()
    with pytest.raises(_cabi.EngineError, match="hand-over wait timed out"):
        f.forward(img)
    out = f.forward(img)                                                # re-submit: works (per-tile kernels), and the error is not sticky
    torch.cuda.synchronize()
    f.status()
    for k in ("pred_vertices", "pred_cam", "token_idx", "cls_logits_softmax"):
        assert torch.equal(out[k], ref[k]), k
    # the engine that never timed out still runs its persistent kernels, repeatedly, with the same bits (epochs advance per launch)
    for _ in range(3):
        again = good.forward(img)
    torch.cuda.synchronize()
    good.status()
    assert torch.equal(again["pred_vertices"], ref["pred_vertices"])


@pytest.mark.parametrize("mode", ["f32", "split3"])
def test_forward_is_captured_into_a_hip_graph_and_replays_bit_identically(built_lib, cuda_dev, mode):
    """include/tokenhmr_hip.h: thmr_forward allocates nothing and never synchronises the host, "so a call in either mode can be captured
    in a hipGraph".  Captured through torch.cuda.CUDAGraph (hipGraph on ROCm) on a side stream at 2 crops (exact-fp32 kernels, key-split
    attention, the small-batch GEMM regime), at 9 and 12 crops (round 6, split3: qkv / fc1 as the 128 x 128 tile stream — ragged M at 9 — and
    fc2's split-K partial sums through it: several hand-over launches per layer on one workspace) and at 40 crops (split3: the persistent
    fc2 with its flag hand-over, the bf16-pipe attention walking two items per workgroup, the persistent decoder kernel with its grid
    barrier): every replay must reproduce the eager call bit
    for bit — a kernel whose device-side state (barrier counters, hand-over flags) is not re-armed by stream order alone would differ or hang —
    with new inputs copied into the captured buffer between replays."""
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.engine import Engine
    cfg = HMRConfig(vit_depth=2, dec_depth=6)
    eng = Engine(cfg, max_batch=40, device=cuda_dev)
    eng.load_state(W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0))
    eng.load_smpl(make_synthetic_smpl(cfg, 0))
    eng.finalize()
    eng.set_vit_gemm(mode)
    keys = ("pred_vertices", "pred_keypoints_2d", "pred_cam", "token_idx", "cls_logits_softmax")
    for B in (2, 9, 12, 40):
        imgs = [torch.randn(B, 3, 256, 256, generator=torch.Generator().manual_seed(50 + B + i)).to(cuda_dev) for i in range(3)]
        want = []
        for im in imgs:
            o = eng.forward(im, outputs=eng._alloc_outputs(B, taps=False, want_probs=True))
            want.append({k: o[k].clone() for k in keys})
        eng.status()
        buf = imgs[0].clone()
        outs = eng._alloc_outputs(B, taps=False, want_probs=True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eng.forward(buf, outputs=outs)                      # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            eng.forward(buf, outputs=outs)
        for rep in range(2):
            for im, w in zip(imgs, want):
                buf.copy_(im)
                for k in keys:
                    outs[k].zero_()
                graph.replay()
                torch.cuda.synchronize()
                for k in keys:
                    assert torch.equal(outs[k], w[k]), (mode, B, rep, k)
        eng.status()


@pytest.mark.parametrize("case", PA.CASES, ids=[c["name"] for c in PA.CASES])
def test_profiler_accounting_is_pinned(built_lib, cuda_dev, case):
    """Every ProfScope of csrc/engine_paths.hip records a class, flops and bytes computed on the host from the call's shapes and the plan: after one
    thmr_forward, launches / flops / bytes of EVERY profiler class equal what the library of the commit named in
    tests/golden/prof_accounting.json reported for the same call (scripts/gen_golden_prof_accounting.py) — exactly: nothing here is
    measured, `ms` is never compared.  A census of the launch sequence per class and of the accounting formulas in every regime of
    vit_plan.h, both modes, both heads, the every-fourth-fc1 sampling of profiler mode "fc1", and the experiments library's
    THMR_SPLIT3_SMALL path — which is also held to the oracle here, under test_small_vs_oracle's bounds (nothing else runs it on the GPU)."""
    with open(os.path.join(GOLDEN_DIR, "prof_accounting.json")) as f:
        golden = json.load(f)
    assert [{k: v for k, v in c.items() if k != "expect"} for c in golden["cases"]] == list(PA.CASES), "the fixture's cases are not the script's"
    assert (golden["dec_depth"], golden["max_batch"]) == (PA.DEC_DEPTH, PA.MAX_BATCH) and golden["commit"]
    expect = next(c["expect"] for c in golden["cases"] if c["name"] == case["name"])
    inputs = PA.case_inputs(case)
    prof, out = PA.run_case(case, cuda_dev, {"shipped": None, "exp": True}, inputs)
    assert set(prof) == set(expect)
    assert any(v["launches"] for v in expect.values())
    for cls in expect:
        got = {k: prof[cls][k] for k in ("launches", "flops", "bytes")}
        print(f"[{case['name']}] {cls}: {got}")
        assert got == expect[cls], (case["name"], cls, got, expect[cls])
    if case["env"].get("THMR_SPLIT3_SMALL") != "1":
        return
    from oracle import tokenhmr_oracle as O
    from test_gpu_model import _check_against
    cfg, sd, tok, smpl, img = inputs
    with torch.no_grad():
        orc = O.forward(img, sd, tok, smpl, cfg)
    o = {k: v.cpu() for k, v in out.items()}
    o["pred_smpl_params"] = {"global_orient": o["rotmat"][:, :1], "body_pose": o["rotmat"][:, 1:], "betas": o["betas"]}
    top2 = orc["cls_logits"].topk(2, dim=-1).values
    ref = dict(vit_features=orc["vit_features"], token_out=orc["token_out"], cls_logits=orc["cls_logits"],
               rotmat=torch.cat([orc["pred_smpl_params"]["global_orient"], orc["pred_smpl_params"]["body_pose"]], 1),
               betas=orc["pred_smpl_params"]["betas"], cam=orc["pred_cam"], verts=orc["pred_vertices"],
               joints=orc["pred_keypoints_3d"], kp2d=orc["pred_keypoints_2d"], token_idx=orc["token_idx"])
    _check_against(o, ref, top2[..., 0] - top2[..., 1], case["name"] + " vs oracle")
    assert torch.allclose(o["cls_logits_softmax"], orc["cls_logits_softmax"], atol=1e-5)
    assert torch.allclose(o["pred_cam_t"], orc["pred_cam_t"], rtol=1e-4, atol=1e-3)
    assert torch.equal(o["focal_length"], orc["focal_length"])
    assert torch.allclose(o["pose6d"].reshape(orc["pose6d"].shape), orc["pose6d"], atol=1e-4)
