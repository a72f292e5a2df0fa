"""The HMR2 head (THMR_CFG_HEAD_HMR2 / HMRConfig.head == "hmr2") on the GPU (-m gpu): against the reference-produced fixture
tests/golden/hmr2_head.npz, against the CPU restatement (tests/hmr2_oracle.py) end to end, against the token engine's decoder bit for
bit, across its two forms (persistent kernel + finish / launch chain) and batch regimes, its refusals, graph capture, and the facade."""
import ctypes as C
import json
import os
import sys
from dataclasses import replace

import numpy as np
import pytest
import torch

from _ref_files_hmr2 import write_hmr2_reference_files

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "scripts") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hmr2_head.npz")
KP = [25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 43]      # 3DPW-TEST keypoint list (datasets_eval.yaml:12)


def make_engine(cfg, sd, smpl, cuda_dev, max_batch, tokenizer=None, **kw):
    from tokenhmr_amd.engine import Engine
    e = Engine(cfg, max_batch=max_batch, device=cuda_dev, **kw)
    e.load_state(sd, tokenizer)
    e.load_smpl(smpl)
    e.finalize()
    return e


# ---------------------------------------------------------------------------------------------- head against the fixture
@pytest.mark.parametrize("case", [0, 1], ids=["init", "trained"])
def test_head_against_the_reference_fixture(built_lib, cuda_dev, case):
    """thmr_head_forward at 2 and at 64 crops against what the reference's own module computed.  Bounds: the ones the token head's
    same quantities are held to (token_out 1e-3; rotmat, betas, cam, pose6d 1e-4); trained-like weights max(1e-4, 2 x the reference's
    own fp32-vs-fp64 distance recorded in the fixture).  Both forms: the persistent kernel + finish, and the launch chain."""
    import gen_golden_hmr2 as G
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    golden = np.load(GOLDEN)
    assert json.loads(str(golden["cases"])) == [list(c) for c in G.CASES]
    name, wseed, style, cseed = G.CASES[case]
    sd = W.make_synthetic_state(G.CFG, wseed, style=style, head="hmr2")
    assert abs(W.checksum(sd) - float(golden[f"{name}.weights_checksum"][0])) < 1e-6 * max(1.0, abs(W.checksum(sd)))
    smpl = make_synthetic_smpl(G.CFG, 0)
    fused = make_engine(G.CFG, sd, smpl, cuda_dev, 64)
    chain = make_engine(G.CFG, sd, smpl, cuda_dev, 64, persistent=False)
    for B in G.BATCHES:
        ctx = G.make_context(cseed, B)
        assert np.array_equal(G.context_sample(ctx).numpy(), golden[f"{name}.b{B}.ctx_sample"])
        for tag, eng in (("fused", fused), ("chain", chain)):
            o = eng.head_forward(ctx.to(cuda_dev), taps=True)
            eng.status()
            got = {"token_out": o["token_out"], "pose6d": o["pose6d"], "rotmat": o["rotmat"], "betas": o["betas"], "cam": o["pred_cam"]}
            for i, k in enumerate(G.OUTPUTS):
                ref = torch.from_numpy(golden[f"{name}.b{B}.{k}"])
                d = float((got[k].cpu().reshape(ref.shape) - ref).abs().max())
                own = float(golden[f"{name}.b{B}.ref32_vs_f64"][i])
                bound = 1e-3 if k == "token_out" else 1e-4
                if style == "trained":
                    bound = max(bound, 2 * own)
                print(f"[{name}, {B} crops, {tag}] {k}: max|diff| = {d:.3e} (bound {bound:.1e}, reference's own fp32-vs-fp64 {own:.2e})")
                assert d < bound, (name, B, tag, k, d, bound)
            assert "token_idx" not in o and "cls_logits_softmax" not in o and "cls_logits" not in o
    fused.close()
    chain.close()


# ---------------------------------------------------------------------------------------------- full forward
@pytest.mark.parametrize("mode", ["split3", "f32"])
@pytest.mark.parametrize("depths", [(2, 2), (32, 6)], ids=["reduced", "full"])
def test_full_forward_vs_oracle(built_lib, cuda_dev, depths, mode):
    """thmr_forward against oracle ViT -> tests/hmr2_oracle.py -> oracle SMPL.  Bounds: vertices and joints 1e-4 m, keypoints 1e-3."""
    from tests import hmr2_oracle as HO
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    cfg = HMRConfig(vit_depth=depths[0], dec_depth=depths[1], head="hmr2")
    sd, smpl = W.make_synthetic_state(cfg, 0), make_synthetic_smpl(cfg, 0)
    B = 4
    img = torch.randn(B, 3, 256, 256, generator=torch.Generator().manual_seed(4200))
    eng = make_engine(cfg, sd, smpl, cuda_dev, B, vit_gemm=mode)
    assert eng.vit_gemm() == mode
    o = eng.forward(img.to(cuda_dev), taps=True)
    eng.status()
    with torch.no_grad():
        ref = HO.forward(img, sd, smpl, cfg)
    for k, bound in (("pred_vertices", 1e-4), ("pred_keypoints_3d", 1e-4), ("pred_keypoints_2d", 1e-3), ("token_out", 1e-3),
                     ("pose6d", 1e-4), ("pred_cam", 1e-4), ("betas", 1e-4)):
        r = ref[k] if k in ref else ref["pred_smpl_params"][k]
        d = float((o[k].cpu() - r).abs().max())
        print(f"[{depths}, {mode}] {k}: max|diff| = {d:.3e}")
        assert d < bound, (depths, mode, k, d)
    R = torch.cat([ref["pred_smpl_params"]["global_orient"], ref["pred_smpl_params"]["body_pose"]], 1)
    assert float((o["rotmat"].cpu() - R).abs().max()) < 1e-4
    assert torch.equal(o["focal_length"].cpu(), ref["focal_length"])
    # pred_cam_t = [cam1, cam2, z = 2 f / (256 cam0 + 1e-9)]: x and y carry cam's bound; dz = |z / cam0| dcam0, so the bound on cam
    # (1e-4) propagates to |z / cam0| 1e-4 — synthetic weights can put cam0 near zero, where z is thousands of metres
    ct, rt, rc = o["pred_cam_t"].cpu(), ref["pred_cam_t"], ref["pred_cam"]
    assert float((ct[:, :2] - rt[:, :2]).abs().max()) < 1e-4
    dz, zb = (ct[:, 2] - rt[:, 2]).abs(), (rt[:, 2] / rc[:, 0]).abs() * 1e-4
    print(f"[{depths}, {mode}] pred_cam_t z: max|diff| = {float(dz.max()):.3e}, smallest bound {float(zb.min()):.3e}")
    assert bool((dz < zb).all()), (dz, zb)
    eng.close()


# ---------------------------------------------------------------------------------------------- decoder identity
def test_token_out_is_bit_identical_to_the_token_engines(built_lib, cuda_dev):
    """The decoder is the token head's code: for the same smpl_head.transformer.* weights and context, token_out of the two engines is
    equal bit for bit in every head regime — 1 / 2 / 8 / 64 crops (persistent kernel; the grid differs: 64 vs 128 workgroups up to 16
    crops) and 130 (launch chain)."""
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    cfg = HMRConfig(vit_depth=1, dec_depth=6)
    hcfg = replace(cfg, head="hmr2")
    tsd, tok, smpl = W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0), make_synthetic_smpl(cfg, 0)
    hsd = W.make_synthetic_state(hcfg, 0)
    assert all(torch.equal(hsd[k], tsd[k]) for k in hsd if k.startswith(("backbone.", "smpl_head.transformer.")))
    te = make_engine(cfg, tsd, smpl, cuda_dev, 130, tokenizer=tok)
    he = make_engine(hcfg, hsd, smpl, cuda_dev, 130)
    ctx = torch.randn(130, 192, 1280, generator=torch.Generator().manual_seed(12)).to(cuda_dev)
    for B in (1, 2, 8, 64, 130):
        a = te.head_forward(ctx[:B], taps=True, want_probs=False)["token_out"].clone()
        b = he.head_forward(ctx[:B], taps=True)["token_out"].clone()
        assert torch.equal(a, b), B
        assert float(a.abs().max()) > 0
    te.status()
    he.status()
    te.close()
    he.close()


# ---------------------------------------------------------------------------------------------- forms and regimes
def test_forms_and_batch_regimes(built_lib, cuda_dev, monkeypatch):
    """Fused (persistent kernel + finish) vs the launch chain: within the bounds of the token head's fused-vs-chain test (token_out
    1e-4, vertices 1e-5).  THMR_CFG_NO_PERSISTENT gives the forced chain's bits.  A crop's result does not depend on its position in
    the batch or on the batch size inside one regime."""
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.engine import Engine
    cfg = HMRConfig(vit_depth=1, dec_depth=6, head="hmr2")
    sd, smpl = W.make_synthetic_state(cfg, 0), make_synthetic_smpl(cfg, 0)
    fused = make_engine(cfg, sd, smpl, cuda_dev, 130)
    nop = Engine(cfg, max_batch=130, device=cuda_dev, weight_arena=fused.weight_arena, persistent=False)
    nop.finalize(assume_all_loaded=True)
    monkeypatch.setenv("THMR_LEGACY_HEAD", "1")          # read once, at thmr_create, by the experiments build only
    chain = Engine(cfg, max_batch=130, device=cuda_dev, weight_arena=fused.weight_arena, experiments=True)
    chain.finalize(assume_all_loaded=True)
    monkeypatch.delenv("THMR_LEGACY_HEAD")
    ctx = torch.randn(130, 192, 1280, generator=torch.Generator().manual_seed(12))
    ctx[5] = ctx[0]
    ctx = ctx.to(cuda_dev)
    keys = ("token_out", "pose6d", "rotmat", "betas", "pred_cam", "pred_cam_t", "pred_vertices", "pred_keypoints_2d")
    for mode in ("split3", "f32"):
        for e in (fused, nop, chain):
            e.set_vit_gemm(mode)
        ref128 = {k: v.clone() for k, v in fused.head_forward(ctx[:128], taps=True).items()}
        ref2 = {k: v.clone() for k, v in fused.head_forward(ctx[:2], taps=True).items()}
        for k in keys:
            assert torch.equal(ref128[k][0], ref128[k][5]), (mode, k)                 # position 0 == position 5
        for B in (1, 2, 6, 8, 16, 17, 49, 64, 100, 128, 130):
            a = {k: v.clone() for k, v in fused.head_forward(ctx[:B], taps=True).items()}
            b = fused.head_forward(ctx[:B], taps=True)
            c = chain.head_forward(ctx[:B], taps=True)
            n = nop.head_forward(ctx[:B], taps=True)
            for k in keys:
                assert torch.equal(a[k], b[k]), (mode, B, k)                          # deterministic
                assert torch.equal(c[k], n[k]), (mode, B, k)                          # NO_PERSISTENT == the forced chain
                if B <= 128 and not (B <= 2 and mode == "split3"):                    # (one and two crops: exact-fp32 to_kv, own regime)
                    assert torch.equal(a[k], ref128[k][:B]), (mode, B, k)             # batch-invariant within the fused regime
                if B <= 2:
                    assert torch.equal(a[k], ref2[k][:B]), (mode, B, k)
            if B > 128:
                for k in keys:
                    assert torch.equal(a[k], c[k]), (mode, B, k)                      # above 128 crops the default IS the chain
            assert float((a["token_out"] - c["token_out"]).abs().max()) < 1e-4, (mode, B)
            assert float((a["pose6d"] - c["pose6d"]).abs().max()) < 1e-5, (mode, B)
            assert float((a["pred_vertices"] - c["pred_vertices"]).abs().max()) < 1e-5, (mode, B)
            if B >= 6:
                assert torch.equal(c["pose6d"][0], c["pose6d"][5]), (mode, B)
    for e in (fused, nop, chain):
        e.status()
        e.close()


# ---------------------------------------------------------------------------------------------- errors and graph capture
def test_refusals_leave_the_engine_usable_and_forward_is_graph_capturable(built_lib, cuda_dev):
    from tokenhmr_amd import _cabi
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.engine import _ptr, _stream_ptr
    cfg = HMRConfig(vit_depth=2, dec_depth=6, head="hmr2")
    eng = make_engine(cfg, W.make_synthetic_state(cfg, 0), make_synthetic_smpl(cfg, 0), cuda_dev, 40)
    lib = eng.lib
    img = torch.randn(2, 3, 256, 256, generator=torch.Generator().manual_seed(3)).to(cuda_dev)
    want = {k: v.clone() for k, v in eng.forward(img).items()}
    extra = {"cls_logits_softmax": torch.empty(2, 160, 2048, device=cuda_dev), "cls_logits": torch.empty(2, 160, 2048, device=cuda_dev),
             "token_idx": torch.empty(2, 160, dtype=torch.int32, device=cuda_dev)}
    ctx = torch.randn(2, 192, 1280, generator=torch.Generator().manual_seed(4)).to(cuda_dev)
    for field, buf in extra.items():
        o = eng._alloc_outputs(2)
        o[field] = buf
        st = eng._outputs_struct(o)
        for rc in (lib.thmr_forward(eng.h, _ptr(img), 2, C.byref(st), _stream_ptr(eng.device)),
                   lib.thmr_head_forward(eng.h, _ptr(ctx), 2, C.byref(st), _stream_ptr(eng.device))):
            assert rc < 0 and field in lib.thmr_last_error(eng.h).decode(), (field, rc, lib.thmr_last_error(eng.h))
    for call, name in ((lambda: eng.vq_argmin(torch.zeros(4, 256, device=cuda_dev)), "thmr_vq_argmin"),
                       (lambda: eng.vq_decode(torch.zeros(1, 160, 2048, device=cuda_dev)), "thmr_vq_decode"),
                       (lambda: eng.encode_tokens(torch.zeros(1, 21, 6, device=cuda_dev)), "thmr_encode_tokens")):
        with pytest.raises(_cabi.EngineError, match=name):
            call()
    with pytest.raises((KeyError, ValueError)):
        eng.load_state({}, {"quantizer.codebook": torch.zeros(2048, 256)})
    eng.status()                                                                   # thmr_engine_status == 0 after all of it
    again = eng.forward(img)
    for k in want:
        assert torch.equal(again[k], want[k]), k
    # capture + replay of thmr_forward, bit-identical to eager: 2 crops (exact-fp32 kernels) and 40 (split3 streams, persistent decoder)
    keys = ("pred_vertices", "pred_keypoints_2d", "pred_cam", "rotmat", "betas")
    for B in (2, 40):
        imgs = [torch.randn(B, 3, 256, 256, generator=torch.Generator().manual_seed(60 + B + i)).to(cuda_dev) for i in range(2)]
        wants = []
        for im in imgs:
            o = eng.forward(im, outputs=eng._alloc_outputs(B))
            wants.append({k: o[k].clone() for k in keys})
        eng.status()
        buf = imgs[0].clone()
        outs = eng._alloc_outputs(B)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eng.forward(buf, outputs=outs)                      # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            eng.forward(buf, outputs=outs)
        for rep in range(2):
            for im, w in zip(imgs, wants):
                buf.copy_(im)
                for k in keys:
                    outs[k].zero_()
                graph.replay()
                torch.cuda.synchronize()
                for k in keys:
                    assert torch.equal(outs[k], w[k]), (B, rep, k)
        eng.status()
        del graph
    eng.close()


# ---------------------------------------------------------------------------------------------- facade
def test_load_tokenhmr_eval_loop_render_and_records(built_lib, cuda_dev, tmp_path):
    """load_tokenhmr on HMR2.0-style files (no tokenizer): the reference's dict for this head, equal to the in-memory model bit for
    bit; max_batch chunking, .to(), .eval(), .smpl.faces, vit_gemm= and shared_gpu=; eval_dp.run_eval; demo.py's loop
    (Renderer.render_batch on pred_vertices); the packed records with zero token words."""
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W, dist as D, render as R
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.model import TokenHMR, load_tokenhmr
    from tokenhmr_amd.evaluator import Evaluator
    from tokenhmr_amd.eval_dp import run_eval

    cfg = HMRConfig(vit_depth=1, dec_depth=2, head="hmr2")
    sd, smpl = W.make_synthetic_state(cfg, 3, style="trained"), make_synthetic_smpl(cfg, 3)
    ck, yml = write_hmr2_reference_files(tmp_path, cfg, sd, smpl)
    model, mcfg = load_tokenhmr(ck, yml, max_batch=4, device=cuda_dev)
    assert model.engine.cfg.head == "hmr2" and model.engine.vit_gemm() == "split3" and mcfg.MODEL.SMPL_HEAD.TYPE == "transformer_decoder"
    assert model.to(cuda_dev) is model and model.eval() is model and np.asarray(model.smpl.faces).shape == (13776, 3)
    ref = TokenHMR.from_state(cfg, sd, None, smpl, max_batch=4, device=cuda_dev)
    n = 10
    img = torch.randn(n, 3, 256, 256, generator=torch.Generator().manual_seed(1)).to(cuda_dev)
    a, b = model({"img": img}), ref({"img": img})                         # 10 crops through max_batch = 4: chunks of 4, 4, 2
    assert set(a) == {"pred_cam", "pred_smpl_params", "pred_cam_t", "focal_length", "pred_keypoints_3d", "pred_vertices", "pred_keypoints_2d"}
    shapes = {"pred_cam": (n, 3), "pred_cam_t": (n, 3), "focal_length": (n, 2), "pred_keypoints_3d": (n, 44, 3), "pred_vertices": (n, 6890, 3),
              "pred_keypoints_2d": (n, 44, 2)}
    for k, s in shapes.items():
        assert tuple(a[k].shape) == s and a[k].dtype == torch.float32 and torch.equal(a[k], b[k]), k
    for k, s in {"global_orient": (n, 1, 3, 3), "body_pose": (n, 23, 3, 3), "betas": (n, 10)}.items():
        assert tuple(a["pred_smpl_params"][k].shape) == s and torch.equal(a["pred_smpl_params"][k], b["pred_smpl_params"][k]), k
    one = model({"img": img[:4]})
    assert torch.equal(one["pred_vertices"], a["pred_vertices"][:4])
    R9 = torch.cat([a["pred_smpl_params"]["global_orient"], a["pred_smpl_params"]["body_pose"]], 1)
    eye = torch.eye(3, device=cuda_dev).expand(n, 24, 3, 3)
    assert float((R9 @ R9.transpose(-1, -2) - eye).abs().max()) < 1e-5      # rotation matrices
    optout, _ = load_tokenhmr(ck, yml, max_batch=4, device=cuda_dev, vit_gemm="f32", shared_gpu=True)
    assert optout.engine.vit_gemm() == "f32" and not optout.engine.persistent
    c = optout({"img": img[:4]})
    assert float((c["pred_vertices"] - a["pred_vertices"][:4]).abs().max()) < 1e-4

    # eval.py's loop
    g = torch.Generator().manual_seed(17)
    kp3d = torch.cat([0.3 * torch.randn(n, 44, 3, generator=g), torch.ones(n, 44, 1)], -1)
    verts = 0.3 * torch.randn(n, 6890, 3, generator=g)
    imgs = img.cpu()

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return n

        def __getitem__(self, i):
            return {"img": imgs[i], "keypoints_3d": kp3d[i], "vertices": verts[i], "imgname": f"im{i:03d}", "idx": i}

    ev = Evaluator(int(1e6), KP, 39, metrics=["mode_re", "mode_mpjpe", "mode_pve"], dataset="3DPW-TEST")
    m = run_eval(model, DS(), ev, batch_size=4, device=cuda_dev)
    assert ev.counter == n and np.isfinite(list(m.values())).all() and m["mode_mpjpe"] > 0

    # demo.py's loop: the renderer on this model's vertices
    renderer = R.Renderer(mcfg, faces=model.smpl.faces, device=cuda_dev)
    cam_t = a["pred_cam_t"][:4].clone()
    cam_t[:, 2] = 2 * 5000 / (256 * 0.9)                                    # synthetic weights: a camera that frames the body
    out = renderer.render_batch(a["pred_vertices"][:4], cam_t, img[:4], mesh_base_color=(0.65, 0.74, 0.86), scene_bg_color=(1, 1, 1))
    out = out[0] if isinstance(out, tuple) else out
    assert tuple(out.shape[:3]) == (4, 256, 256) and bool(torch.isfinite(torch.as_tensor(out)).all())

    # records: same layout, zero token words; ShardedRunner (one process) hands them back
    eo = model.engine.forward(img[:4])
    assert "token_idx" not in eo
    rec = D.pack_records(eo)
    assert tuple(rec.shape) == (4, D.RECORD_WORDS) and not bool(rec[:, -160:].any())
    un = D.ShardedRunner(lambda x: model.engine.forward(x), gather=False)(img[:4])
    assert torch.equal(un["pred_vertices"], eo["pred_vertices"]) and torch.equal(un["rotmat"], eo["rotmat"])
    assert un["token_idx"].dtype == torch.int32 and not bool(un["token_idx"].any())
    cpu = D.pack_records({k: v.cpu() for k, v in eo.items()})
    assert torch.equal(cpu, rec.cpu())
    model.engine.status()
