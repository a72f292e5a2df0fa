"""The HMR2 head (MODEL.SMPL_HEAD.TYPE: transformer_decoder) without a GPU: the C contract (thmr_spec / thmr_arena_bytes with
THMR_CFG_HEAD_HMR2), the host side (HMRConfig.head, weights.spec, read_reference_files) and the restatement tests/hmr2_oracle.py,
pinned to tests/golden/hmr2_head.npz — what the reference's own SMPLTransformerDecoderHead computed (scripts/gen_golden_hmr2.py) —
and to that module live where the reference tree exists."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from _ref_files_hmr2 import write_hmr2_reference_files

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "scripts") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hmr2_head.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def c_spec(lib, vit_depth, dec_depth, flags, max_batch=4):
    from tokenhmr_amd import _cabi
    cfg = _cabi.Config(abi_version=_cabi.ABI_VERSION, vit_depth=vit_depth, dec_depth=dec_depth, max_batch=max_batch, device=0, flags=flags)
    n = lib.thmr_spec(C.byref(cfg), -1, None, None)
    assert n > 0, lib.thmr_last_error(None)
    out = []
    for i in range(n):
        name, numel = C.c_char_p(), C.c_int64()
        assert lib.thmr_spec(C.byref(cfg), i, C.byref(name), C.byref(numel)) == n
        out.append((name.value.decode(), numel.value))
    return out


def c_arena(lib, vit_depth, dec_depth, max_batch, flags):
    from tokenhmr_amd import _cabi
    cfg = _cabi.Config(abi_version=_cabi.ABI_VERSION, vit_depth=vit_depth, dec_depth=dec_depth, max_batch=max_batch, device=0, flags=flags)
    wb, sb = C.c_size_t(0), C.c_size_t(0)
    assert lib.thmr_arena_bytes(C.byref(cfg), C.byref(wb), C.byref(sb)) == 0
    return wb.value, sb.value


# ---------------------------------------------------------------------------------------------- the C contract
def test_spec_with_flag_is_the_reference_heads_state_dict(built_lib, golden):
    from tokenhmr_amd import _cabi
    keys = json.loads(str(golden["state_keys"]))                       # the reference module's own state_dict(): [name, shape]
    want = [("smpl_head." + k, int(np.prod(s))) for k, s in keys]
    got = c_spec(built_lib, 1, 6, _cabi.CFG_HEAD_HMR2)
    head = [(n, e) for n, e in got if n.startswith("smpl_head.")]
    assert sorted(head) == sorted(want)
    names = [n for n, _ in got]
    assert ("smpl_head.decpose.weight", 144 * 1024) in got and ("smpl_head.decpose.bias", 144) in got
    assert not any(n.startswith(("smpl_head.decpose_grot", "smpl_head.decpose_hands", "smpl_head.decpose.mixer", "decoder.", "quantizer.",
                                 "encoder.")) for n in names)
    # every backbone.* and smpl_head.transformer.* entry is the flag-less contract's, in its order
    plain = c_spec(built_lib, 1, 6, 0)
    shared = lambda s: [(n, e) for n, e in s if n.startswith(("backbone.", "smpl_head.transformer."))]
    assert shared(got) == shared(plain)
    assert {n for n, _ in got} - {n for n, _ in shared(got)} == {
        "smpl_head.decpose.weight", "smpl_head.decpose.bias", "smpl_head.decshape.weight", "smpl_head.decshape.bias",
        "smpl_head.deccam.weight", "smpl_head.deccam.bias", "smpl_head.init_body_pose", "smpl_head.init_betas", "smpl_head.init_cam"}


@pytest.mark.parametrize("vit_depth,dec_depth", [(1, 6), (2, 2), (32, 6)])
def test_python_spec_agrees_with_c_spec(built_lib, vit_depth, dec_depth):
    from tokenhmr_amd import _cabi, weights as W
    from tokenhmr_amd.config import HMRConfig
    cfg = HMRConfig(vit_depth=vit_depth, dec_depth=dec_depth, head="hmr2")
    py = [(n, int(np.prod(s))) for n, s, _, _ in W.spec(cfg)]
    assert py == c_spec(built_lib, vit_depth, dec_depth, _cabi.CFG_HEAD_HMR2)


# recorded from the parent commit's library: (vit_depth, dec_depth, max_batch, flags) -> (tensors, total elements, sha256 of
# "name:numel\n" lines [:16], weight arena bytes, scratch arena bytes)
PARENT = {
    (32, 6, 64, 0): (586, 688161282, "890f86205db53d15", 2868424704, 683887360),
    (2, 2, 4, 0): (158, 71582722, "0f3f7e8ea15ff586", 402110464, 64373248),
    (32, 6, 1, 2): (586, 688161282, "890f86205db53d15", 2868424704, 33791488),
    (1, 6, 130, 1): (214, 78160642, "9d6db048a62c8646", 428422144, 1356705536),
}


@pytest.mark.parametrize("key", sorted(PARENT))
def test_flagless_contract_is_the_parents(built_lib, key):
    vd, dd, mb, fl = key
    spec = c_spec(built_lib, vd, dd, fl, mb)
    h = hashlib.sha256()
    for n, e in spec:
        h.update(f"{n}:{e}\n".encode())
    assert (len(spec), sum(e for _, e in spec), h.hexdigest()[:16]) + c_arena(built_lib, vd, dd, mb, fl) == PARENT[key]


def test_hmr2_arenas_are_smaller_and_flags_compose(built_lib):
    from tokenhmr_amd import _cabi
    for mb in (1, 64, 130):
        w0, s0 = c_arena(built_lib, 32, 6, mb, 0)
        w1, s1 = c_arena(built_lib, 32, 6, mb, _cabi.CFG_HEAD_HMR2)
        assert w1 < w0 and s1 < s0
        assert c_arena(built_lib, 32, 6, mb, _cabi.CFG_HEAD_HMR2 | _cabi.CFG_NO_PERSISTENT | _cabi.CFG_VIT_GEMM_F32) == (w1, s1)
    # no mixer / VQ scratch: what is left of a crop's share beyond the ViT's and the SMPL stage's is below 64 KB
    _, s64 = c_arena(built_lib, 32, 6, 64, _cabi.CFG_HEAD_HMR2)
    _, t64 = c_arena(built_lib, 32, 6, 64, 0)
    assert t64 - s64 > 64 * 160 * 64 * 4 * 10           # ten (B, 160, 64) mixer buffers alone
    cfg = _cabi.Config(abi_version=_cabi.ABI_VERSION, vit_depth=1, dec_depth=1, max_batch=1, device=0, flags=16)
    assert built_lib.thmr_spec(C.byref(cfg), -1, None, None) < 0       # an unknown flag is still refused
    cfg.flags = 4
    assert built_lib.thmr_spec(C.byref(cfg), -1, None, None) < 0       # (the unassigned bit between the ABI 5 flags and this one, too)


# ---------------------------------------------------------------------------------------------- config / weights
def test_config_and_synthetic_state():
    from dataclasses import replace
    from tokenhmr_amd.config import HMRConfig, RELEASE
    from tokenhmr_amd import weights as W
    assert RELEASE.head == "token" and HMRConfig().head == "token"
    with pytest.raises(ValueError):
        HMRConfig(head="mlp")
    cfg = HMRConfig(vit_depth=1, dec_depth=2)
    for style in ("init", "trained"):
        tok_sd = W.make_synthetic_state(cfg, 5, style=style)
        sd = W.make_synthetic_state(cfg, 5, style=style, head="hmr2")
        assert list(sd) == [n for n, *_ in W.spec(replace(cfg, head="hmr2"))]
        shared = [k for k in sd if k.startswith(("backbone.", "smpl_head.transformer."))]
        assert shared == [k for k in tok_sd if k.startswith(("backbone.", "smpl_head.transformer."))]
        assert all(torch.equal(sd[k], tok_sd[k]) for k in shared)
        if style == "init":       # ("trained" draws its mean parameters behind the head-specific tensors)
            assert torch.equal(sd["smpl_head.init_body_pose"], tok_sd["smpl_head.init_body_pose"])
        assert sd["smpl_head.decpose.weight"].shape == (144, 1024)
        assert torch.equal(W.make_synthetic_state(replace(cfg, head="hmr2"), 5, style=style)["smpl_head.decpose.weight"], sd["smpl_head.decpose.weight"])
        W.validate_state(sd, replace(cfg, head="hmr2"), None)
        with pytest.raises(KeyError):
            W.validate_state(tok_sd, replace(cfg, head="hmr2"), None)
        with pytest.raises(ValueError):
            W.validate_state(sd, replace(cfg, head="hmr2"), {"quantizer.codebook": torch.zeros(1)})
    # the token state of a seed is what it was
    assert abs(W.checksum(W.make_synthetic_state(HMRConfig(vit_depth=2, dec_depth=2), 0)) -
               W.checksum(W.make_synthetic_state(HMRConfig(vit_depth=2, dec_depth=2), 0, head="token"))) == 0.0


# ---------------------------------------------------------------------------------------------- file readers
@pytest.fixture(scope="module")
def tiny():
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    cfg = HMRConfig(vit_depth=1, dec_depth=2, head="hmr2")
    return cfg, W.make_synthetic_state(cfg, 3, style="trained"), make_synthetic_smpl(cfg, 3)


def test_read_reference_files_transformer_decoder(tiny, tmp_path):
    from tokenhmr_amd.model import read_reference_files
    cfg, sd, smpl = tiny
    ck, yml = write_hmr2_reference_files(tmp_path, cfg, sd, smpl)
    assert not os.path.exists(tmp_path / "tokenizer.pth") and "TOKENIZER_CHECKPOINT_PATH" not in open(yml).read()
    hcfg, state, tok, sm, mcfg = read_reference_files(ck, yml)
    assert hcfg.head == "hmr2" and hcfg.vit_depth == 1 and hcfg.dec_depth == 2 and tok is None
    assert mcfg.MODEL.SMPL_HEAD.TYPE == "transformer_decoder"
    assert set(state) == set(sd) and all(torch.equal(state[k], sd[k]) for k in sd)      # init_cam comes from smpl_mean_params.npz
    assert torch.equal(sm["v_template"], smpl["v_template"])


def test_read_reference_files_strict_and_foreign_keys(tiny, tmp_path):
    from tokenhmr_amd.model import read_reference_files
    cfg, sd, smpl = tiny
    # discriminator.* and smpl.* are in every file the writer makes and are ignored; an unknown smpl_head.* key is strict's business
    ck, yml = write_hmr2_reference_files(tmp_path, cfg, sd, smpl, extra_state={"smpl_head.decpose_hands.weight": torch.zeros(12, 1024)})
    with pytest.raises(KeyError):
        read_reference_files(ck, yml)
    with pytest.warns(Warning):
        hcfg, state, *_ = read_reference_files(ck, yml, strict=False)
    assert hcfg.head == "hmr2" and "smpl_head.decpose_hands.weight" not in state


@pytest.mark.parametrize("key,val", [("IEF_ITERS", 3), ("TRANSFORMER_INPUT", "mean_shape"), ("JOINT_REP", "aa")])
def test_unsupported_head_keys_name_themselves(tiny, tmp_path, key, val):
    from tokenhmr_amd.model import read_reference_files
    cfg, sd, smpl = tiny
    ck, yml = write_hmr2_reference_files(tmp_path, cfg, sd, smpl, head_overrides={key: val})
    with pytest.raises(NotImplementedError, match=key):
        read_reference_files(ck, yml)


@pytest.mark.parametrize("key,val", [("dim_head", 32), ("heads", 4), ("mlp_dim", 2048), ("context_dim", 1024)])
def test_wrong_decoder_dimension_names_the_key(tiny, tmp_path, key, val):
    from tokenhmr_amd.model import read_reference_files
    cfg, sd, smpl = tiny
    ck, yml = write_hmr2_reference_files(tmp_path, cfg, sd, smpl, decoder_overrides={key: val})
    with pytest.raises(ValueError, match=key):
        read_reference_files(ck, yml)


def test_token_files_still_read_as_token(tmp_path):
    from _ref_files import write_reference_files
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.model import read_reference_files
    cfg = HMRConfig(vit_depth=1, dec_depth=2)
    ck, yml = write_reference_files(tmp_path, cfg, W.make_synthetic_state(cfg, 3), W.make_synthetic_tokenizer(cfg, 3), make_synthetic_smpl(cfg, 3))
    hcfg, _, tok, _, _ = read_reference_files(ck, yml)
    assert hcfg.head == "token" and "quantizer.codebook" in tok


# ---------------------------------------------------------------------------------------------- the restatement
def _cases(golden):
    import gen_golden_hmr2 as G
    assert json.loads(str(golden["cases"])) == [list(c) for c in G.CASES] and list(golden["batches"]) == list(G.BATCHES)
    return G


@pytest.mark.parametrize("case", [0, 1], ids=["init", "trained"])
def test_restatement_against_the_fixture(golden, case):
    """float64 restatement vs the reference's float32 outputs: within the reference's OWN recorded fp32-vs-fp64 distance (the
    restatement in fp64 is the reference in fp64 up to 1e-12); float32 restatement: the bounds the GPU path is held to."""
    from tests import hmr2_oracle as HO
    from tokenhmr_amd import weights as W
    G = _cases(golden)
    name, wseed, style, cseed = G.CASES[case]
    sd = W.make_synthetic_state(G.CFG, wseed, style=style, head="hmr2")
    assert abs(W.checksum(sd) - float(golden[f"{name}.weights_checksum"][0])) < 1e-6 * max(1.0, abs(W.checksum(sd)))
    sd64 = {k: v.double() for k, v in sd.items()}
    for B in G.BATCHES:
        ctx = G.make_context(cseed, B)
        assert np.array_equal(G.context_sample(ctx).numpy(), golden[f"{name}.b{B}.ctx_sample"])
        with torch.no_grad():
            r64 = HO.head_forward(ctx.double(), sd64, G.CFG)
            r32 = HO.head_forward(ctx, sd, G.CFG)
        for i, k in enumerate(G.OUTPUTS):
            ref = torch.from_numpy(golden[f"{name}.b{B}.{k}"])
            own = float(golden[f"{name}.b{B}.ref32_vs_f64"][i])
            d64 = float((r64[k].reshape(ref.shape) - ref.double()).abs().max())
            d32 = float((r32[k].reshape(ref.shape) - ref).abs().max())
            print(f"[{name}, {B} crops] {k}: fp64 restatement {d64:.3e} (reference's own {own:.3e}), fp32 restatement {d32:.3e}")
            assert d64 <= own * (1 + 1e-6) + 1e-9, (k, d64, own)
            assert d32 < (1e-3 if k == "token_out" else 1e-4), (k, d32)


def test_restatement_against_the_live_reference(golden):
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("reference tree not present (it is on the build machine only)")
    from tests import hmr2_oracle as HO
    from tokenhmr_amd import weights as W
    G = _cases(golden)
    name, wseed, style, cseed = G.CASES[1]
    sd = W.make_synthetic_state(G.CFG, wseed, style=style, head="hmr2")
    head = G.reference_head({k: v.double() for k, v in sd.items()}, dtype=torch.float64)
    assert G.state_keys(head) == json.loads(str(golden["state_keys"]))
    ctx = G.make_context(cseed + 50, 3)
    live = G.run_reference(head, ctx, dtype=torch.float64)
    with torch.no_grad():
        own = HO.head_forward(ctx.double(), {k: v.double() for k, v in sd.items()}, G.CFG)
    for k in G.OUTPUTS:
        assert float((own[k].reshape(live[k].shape) - live[k]).abs().max()) < 1e-10, k
    # and the fixture is what the generator produces today
    h32 = G.reference_head(sd, dtype=torch.float32)
    r32 = G.run_reference(h32, G.make_context(cseed, 2))
    for k in G.OUTPUTS:
        assert np.array_equal(r32[k].numpy(), golden[f"{name}.b2.{k}"]), k


def test_reference_raises_for_what_the_reader_refuses():
    """'aa' raises in the reference itself (smpl_head.py:61-62): the reader's NotImplementedError mirrors it."""
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("reference tree not present (it is on the build machine only)")
    import gen_golden_hmr2 as G
    from tokenhmr_amd import weights as W
    sd = W.make_synthetic_state(G.CFG, 0, head="hmr2")
    # 'aa' makes decpose 72 rows wide (smpl_head.py:18-19,32), so the 6D weights do not load: the module keeps its own initialisation
    head = G.reference_head(sd, head_extra={"JOINT_REP": "aa"}, load_weights=False)
    assert head.decpose.out_features == 72
    with pytest.raises(NotImplementedError):
        G.run_reference(head, G.make_context(1, 1))
