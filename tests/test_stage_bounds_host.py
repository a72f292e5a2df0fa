"""CPU (-m "not gpu"): the proof that the rule of tests/stage_bounds.py sees what the fixed stage bounds of tests/test_gpu_model.py
(vit < 2e-3, token_out < 1e-3, cls_logits < 1e-3) do not.  Three mistakes a fused kernel can make on its own — LayerNorm eps x10, the
tanh form of GELU in place of erf, every F.linear operand cut to two bf16 pieces instead of three — are applied to the fp32 oracle.
Each stage is fed the CORRECT fp32 oracle's upstream output, as tests/test_gpu_stage_fp64.py feeds a stage the device's own, so the
numbers here are per stage: the mistaken `token_out` and `cls_logits` must each exceed bound(ref32, ref64, mult) at the multiplier
those stages use in the GPU file, and on the default weights every mistake passes the old 1e-3 through the whole chain.

4 crops, vit_depth 2, dec_depth 6, both weight kinds.  Measured (distance / bound at mult 2, token_out / cls_logits): two bf16 pieces
9.3 / 9.0 (default) and 9.3 / 7.5 (trained-like); LayerNorm eps 44 / 325 and 19 / 85; tanh-GELU 144 / 192 and 94 / 147.  At the cap of
the GPU file's multipliers, 4, the two-piece product is still 3.8 to 4.7 times the bound — above 4 it would start to escape.  pred_cam, the
one stage that carries 4, is checked at its own read-out: the two-piece product is 5.6 (default) and 5.3 (trained-like) times its bound."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

import stage_bounds as SB
from oracle import tokenhmr_oracle as O
from tokenhmr_amd import weights as W
from tokenhmr_amd.config import HMRConfig

CFG = HMRConfig(vit_depth=2, dec_depth=6)
KINDS = {"default": (0, "init"), "trained": (3, "trained")}
OLD_BOUND = 1e-3           # tests/test_gpu_model.py::_check_against on token_out and cls_logits


def _two_pieces(x):
    hi = x.bfloat16().float()
    return hi + (x - hi).bfloat16().float()


@pytest.fixture(scope="module", params=list(KINDS))
def refs(request):
    """The correct oracle once per weight kind: fp32 chain, and per stage the fp64 value on the fp32 chain's own upstream output."""
    seed, style = KINDS[request.param]
    sd = W.make_synthetic_state(CFG, seed, style)
    sd64 = SB.to64(sd)
    img = torch.randn(4, 3, 256, 256, generator=torch.Generator().manual_seed(4000))
    with torch.no_grad():
        vit32 = O.vit_forward(img, sd, CFG)
        tok32 = O.decoder_forward(vit32, sd, CFG)
        log32 = O.classifier_logits(tok32, sd, CFG)
        tok64 = O.decoder_forward(vit32.double(), sd64, CFG)
        log64 = O.classifier_logits(tok32.double(), sd64, CFG)
    return dict(kind=request.param, sd=sd, img=img, vit32=vit32, tok32=tok32, log32=log32, tok64=tok64, log64=log64)


def _mistaken(name, monkeypatch):
    cfg = CFG
    if name == "ln_eps_x10":
        cfg = dataclasses.replace(CFG, vit_ln_eps=10 * CFG.vit_ln_eps, ln_eps=10 * CFG.ln_eps)
    elif name == "tanh_gelu":
        gelu = F.gelu
        monkeypatch.setattr(F, "gelu", lambda x: gelu(x, approximate="tanh"))
    elif name == "two_bf16_pieces":
        linear = F.linear
        monkeypatch.setattr(F, "linear", lambda x, w, b=None: linear(_two_pieces(x), _two_pieces(w), b))
    return cfg


@pytest.mark.parametrize("mistake", ["ln_eps_x10", "tanh_gelu", "two_bf16_pieces"])
def test_rule_sees_the_mistake_the_fixed_bound_passes(refs, mistake, monkeypatch):
    MULT = SB.MULT
    r = refs
    cfg = _mistaken(mistake, monkeypatch)
    with torch.no_grad():
        tok_stage = O.decoder_forward(r["vit32"], r["sd"], cfg)              # the stage alone, on the correct upstream output
        log_stage = O.classifier_logits(r["tok32"], r["sd"], cfg)
        vit = O.vit_forward(r["img"], r["sd"], cfg)                           # the whole chain, as the old bounds see it
        tok_chain = O.decoder_forward(vit, r["sd"], cfg)
        log_chain = O.classifier_logits(tok_chain, r["sd"], cfg)
    monkeypatch.undo()
    for stage, got, r32, r64 in (("token_out", tok_stage, r["tok32"], r["tok64"]), ("cls_logits", log_stage, r["log32"], r["log64"])):
        d, b = SB.dist(got, r64), SB.bound(r32, r64, MULT[stage])
        print(f"[{r['kind']}] {mistake}, {stage}: distance to fp64 {d:.3e}, reference's own {SB.dist(r32, r64):.3e}, "
              f"bound {b:.3e} (x{MULT[stage]:g}): {d / b:.1f} times the bound")
        assert d > b, (mistake, stage, d, b)
        assert not SB.check(f"[{r['kind']}] {mistake} {stage}", got, r32, r64, MULT[stage])[0]
    if mistake == "two_bf16_pieces":
        # pred_cam carries the largest multiplier of the GPU file (4): its read-out (token_head.py:99-105) with both operands cut to two pieces
        sd, t32 = r["sd"], r["tok32"]
        wc, bc, ic = sd["smpl_head.deccam.weight"], sd["smpl_head.deccam.bias"], sd["smpl_head.init_cam"]
        with torch.no_grad():
            c32, c64 = F.linear(t32, wc, bc) + ic, F.linear(t32.double(), wc.double(), bc.double()) + ic.double()
            got = F.linear(_two_pieces(t32), _two_pieces(wc), bc) + ic
        d, b = SB.dist(got, c64), SB.bound(c32, c64, MULT["pred_cam"])
        print(f"[{r['kind']}] {mistake}, pred_cam: distance to fp64 {d:.3e}, bound {b:.3e} (x{MULT['pred_cam']:g}): {d / b:.1f} times the bound")
        assert d > b, (mistake, "pred_cam", d, b)
    old = {k: SB.dist(a, b) for k, a, b in (("vit", vit, r["vit32"]), ("token_out", tok_chain, r["tok32"]), ("cls_logits", log_chain, r["log32"]))}
    print(f"[{r['kind']}] {mistake}, whole chain against the fp32 oracle (what the fixed bounds compare): " + " ".join(f"{k} {v:.2e}" for k, v in old.items()))
    if r["kind"] == "default":
        assert old["vit"] < 2e-3 and old["token_out"] < OLD_BOUND and old["cls_logits"] < OLD_BOUND, old


def test_bound_helpers():
    a64 = torch.tensor([[1.0, 100.0], [-2.0, 50.0]], dtype=torch.float64)
    a32 = (a64 + torch.tensor([[1e-6, 0.0], [0.0, -3e-5]], dtype=torch.float64)).float()
    own = (a32.double() - a64).abs()
    assert SB.bound(a32, a64) == max(2.0 ** -22 * 100.0, 2.0 * own.max().item())
    assert SB.bound(a32, a64, mult=4.0) == 4.0 * own.max().item()
    assert SB.bound(a64.float(), a64) == 2.0 ** -22 * 100.0                 # exact reference: the 4-ulp floor
    assert SB.bound(a64.float(), a64, floor=SB.FLOOR_M) == SB.FLOOR_M
    pc = SB.bound_per_channel(a32, a64)
    assert pc.shape == (2,) and pc[0].item() == max(2.0 ** -22 * 2.0, 2.0 * own[:, 0].max().item()) and pc[1].item() == 2.0 * own[:, 1].max().item()
    # an error in the quiet channel that the max-abs bound hides
    dev = a32.clone()
    dev[0, 0] += 2e-5
    assert SB.check("max-abs", dev, a32, a64)[0] and not SB.check_per_channel("quiet channel", dev, a32, a64)[0]
    s = SB.to64({"w": torch.ones(2), "i": torch.ones(2, dtype=torch.int32), "flag": True})
    assert s["w"].dtype == torch.float64 and s["i"].dtype == torch.int32 and s["flag"] is True
