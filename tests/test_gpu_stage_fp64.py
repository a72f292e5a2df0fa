"""Stage parity against float64 (-m gpu): the stages of the engine — ViT, decoder, mixer / classifier, VQ decoder and read-out within the
head call, camera and body, the encoder's quantiser — against the CPU oracle evaluated in float64, bounded by the oracle's OWN fp32 distance to float64 on the
same inputs (tests/stage_bounds.py: max(4 ulp of the largest element, MULT x that distance); metres: max(2e-6 m, ...)).  The fixed
bounds of tests/test_gpu_model.py (vit 2e-3, token_out 1e-3, cls_logits 1e-3, pose6d 1e-4) are several hundred times looser and pass a
LayerNorm eps x10, a tanh-GELU and a two-bf16-piece product (tests/test_stage_bounds_host.py).

How a stage is checked.  It is fed the DEVICE's own upstream output, and its float64 reference and the fp32 reference of the bound are
computed on exactly those bits, so no stage inherits another's error.  Inputs come from a pool of 11 distinct items, row b of a batch
being pool item b % 11 (11 is coprime to every tile, group and cluster size): rows b and b + 11 must be BIT-equal at every tap, which
leaves rows 0 ... 10 to compare with the references.  One engine per weight kind (default-init; "trained-like": LayerNorm gains in
[0.1, 10], x50 outlier channels), HMRConfig(vit_depth=2, dec_depth=6), max_batch 136; every stage in both ViT GEMM modes.

Batch sizes: the ViT at the regime edges of tokenhmr_amd/csrc/vit_plan.h (f32: 1, 3, 7, 17; split3: 1, 3, 5, 16, 32); the encoder at 1, 6, 7, 25; the head at 1, 2, 3 (exact-fp32
to_kv below 3 crops in split3 mode), 6, 7 (the VQ decoder's tiny-M GEMMs end at 6), 16, 17, 25, 26 (in-kernel mixer cluster of 10
workgroups per crop up to 25), 49, 128 (64 / 128 / 192 / 256-workgroup grids of the persistent kernel), 136 (the chain of GEMMs above
kFusedHeadMaxB).

Every check prints the device's distance, the reference's own distance, their ratio and the bound; the module prints the largest ratio
per stage, mode and weight kind when it ends.

Measured on an MI355X: device distance / the reference's own fp32 distance, the largest over the batch sizes, as
split3 default | split3 trained-like | f32 default | f32 trained-like.  The bound allows MULT (tests/stage_bounds.py: 2; pred_cam and the
ViT's per-channel rule 4); a ratio above it can still pass on the 4-ulp / 2e-6 m floor.
  vit_features                    1.02 | 3.03 | 1.10 | 3.03    (3.03: one crop alone; three crops and more <= 1.87)
  vit_features, worst channel     3.09 | 4.70 | 3.09 | 4.70    (one crop alone; three crops and more <= 2.28 | 3.11 | 2.71 | 3.85)
  token_out                       1.04 | 1.11 | 1.04 | 1.16    (randn context: 1.15 | 1.07 | 1.15 | 1.11)
  cls_logits                      1.25 | 1.12 | 1.19 | 1.20
  cls_logits_softmax              0.79 | 1.00 | 0.77 | 0.87
  pose6d / betas / pred_cam       1.78 / 0.79 / 2.12 | 1.70 / 1.57 / 2.56 | 1.38 / 0.78 / 1.95 | 1.16 / 1.57 / 2.56
  rotmat                          1.59 | 1.36 | 1.75 | 1.35
  vertices / joints               0.94 / 0.99 | 0.98 / 0.43 | 1.00 / 0.76 | 1.23 / 0.40    (all under the 2e-6 m floor: 1.5e-7 ... 6.7e-7 m)
  cam_t / kp2d                    1.00 (the device's bits are the fp32 oracle's)
Token and code indices: 0 differ from the float64 argmax / argmin, and the gap rule leaves out 0.00 % of the tokens, in every case.

NOT MET, ONE CASE: the ViT of ONE crop alone on the trained-like weights (3.03; 4.70 per channel) needs a multiplier above the cap of 4.
The fmaf-chain experiment at _VIT_ONE_CROP does not account for it and no other cause was found; its assertions stay in, unchanged, as
strict expected failures that wait for SB.OverBound only, behind plain ceilings (twice / per channel 4 x the reference's own distance over
the whole pool), so an error above those fails the suite.
LEFT OUT: the stand-alone VQ decoder and the encoder's latent (4.16 and 4.15; cause found in the tile GEMM's accumulation order, see the
note at VQ_CASES) — they wait for the kernel change that lets them meet the rule.
"""
import itertools

import pytest
import torch
import torch.nn.functional as F

import stage_bounds as SB
from stage_bounds import MULT, MULT_MAX
from oracle import tokenhmr_oracle as O
from tokenhmr_amd import weights as W
from tokenhmr_amd.config import HMRConfig

pytestmark = pytest.mark.gpu

CFG = HMRConfig(vit_depth=2, dec_depth=6)
POOL, MAX_BATCH = 11, 136
KINDS = {"default": (0, "init"), "trained": (3, "trained")}
MODES = ("split3", "f32")
VIT_BATCHES = {"f32": (1, 3, 7, 17), "split3": (1, 3, 5, 16, 32)}
HEAD_BATCHES = (1, 2, 3, 6, 7, 16, 17, 25, 26, 49, 128, 136)
VQ_BATCHES = (1, 6, 7, 25)
HEAD_TAPS = ("token_out", "cls_logits", "cls_logits_softmax", "token_idx", "pose6d", "rotmat", "betas", "pred_cam", "pred_cam_t",
             "pred_vertices", "pred_keypoints_3d", "pred_keypoints_2d")

_MEASURED = {}           # (stage, mode, kind) -> largest device / reference distance ratio seen in this run
_WORLDS = {}


def _sel(B):
    return torch.arange(B) % POOL


def _rows_repeat(t, what):
    """rows b and b + 11 hold the same input: bit-equal outputs (compared on the device)"""
    if t.shape[0] > POOL:
        assert torch.equal(t[POOL:], t[:-POOL]), f"{what}: rows b and b + {POOL} hold the same input but differ"


def _check(failures, stage, w, mode, B, dev, r32, r64, floor=None, note=""):
    tag = f"[{w.kind} {mode} B={B}] {stage}{note}"
    ok, line = SB.check(tag, dev, r32, r64, MULT[stage], floor)
    own = SB.dist(r32, r64)
    if own > 0:
        key = (stage + note, mode, w.kind)
        _MEASURED[key] = max(_MEASURED.get(key, 0.0), SB.dist(dev, r64) / own)
    if not ok:
        failures.append(line)


class World:
    """One weight kind: the engine, the pools, and the references that depend only on the pools (each computed once, on first use)."""

    def __init__(self, kind, dev):
        from tokenhmr_amd.engine import Engine
        from tokenhmr_amd.smpl_assets import make_synthetic_smpl
        seed, style = KINDS[kind]
        self.kind, self.dev = kind, dev
        self.sd = W.make_synthetic_state(CFG, seed, style)
        self.tok = dict(W.make_synthetic_tokenizer(CFG, seed))
        self.enc = dict(W.make_synthetic_encoder(CFG, seed))
        self.smpl = make_synthetic_smpl(CFG, seed)
        self.sd64, self.tok64, self.enc64, self.smpl64 = SB.to64(self.sd), SB.to64(self.tok), SB.to64(self.enc), SB.to64(self.smpl)
        self.eng = Engine(CFG, max_batch=MAX_BATCH, device=dev)
        self.eng.load_state(self.sd, dict(self.tok, **self.enc))
        self.eng.load_smpl(self.smpl)
        self.eng.finalize()
        g = torch.Generator().manual_seed(4100 + seed)
        self.img = torch.randn(POOL, 3, 256, 256, generator=g)
        self.ctx_randn = torch.randn(POOL, 192, 1280, generator=g)
        self._cache = {}

    def once(self, key, fn):
        if key not in self._cache:
            with torch.no_grad():
                self._cache[key] = fn()
        return self._cache[key]

    def vit_refs(self):
        return self.once("vit", lambda: (O.vit_forward(self.img, self.sd, CFG), O.vit_forward(self.img.double(), self.sd64, CFG)))

    def ctx_pool(self, name):
        """(11, 192, 1280) on the host: "vit" = the DEVICE's ViT features of the image pool (split3 mode, one call of 11), "randn"."""
        if name == "randn":
            return self.ctx_randn

        def run():
            self.eng.set_vit_gemm("split3")
            out = self.eng.vit_forward(self.img.to(self.dev)).cpu()
            self.eng.status()
            return out
        return self.once("ctx_vit", run)

    def decoder_refs(self, name):
        ctx = self.ctx_pool(name)
        return self.once("dec_" + name, lambda: (O.decoder_forward(ctx, self.sd, CFG), O.decoder_forward(ctx.double(), self.sd64, CFG)))

    def head(self, mode, B, ctx_name="vit", taps=HEAD_TAPS):
        """One head call of B crops on ctx pool rows b % 11: every tap's rows b / b + 11 compared on the device, rows 0 ... 10 returned
        on the host; "dev" keeps the full device tensors the camera-and-body stage is fed."""
        ctx = self.ctx_pool(ctx_name)[_sel(B)].to(self.dev)
        self.eng.set_vit_gemm(mode)
        o = self.eng.head_forward(ctx, taps=True)
        self.eng.status()
        for k in taps:
            _rows_repeat(o[k], f"[{self.kind} {mode} B={B} ctx={ctx_name}] {k}")
        n = min(B, POOL)
        out = {k: o[k][:n].cpu() for k in taps}
        out["dev"] = {k: o[k] for k in ("rotmat", "betas", "pred_cam")}
        return out

    def seed_head(self):
        """The pool of the encoder: the device's own body pose of the 11 pool items."""
        def run():
            o = self.head("split3", POOL)
            return dict(pose=o["pose6d"][:, 6:132].reshape(POOL, 21, 6).contiguous())
        return self.once("seed_head", run)


def _world(kind, dev):
    if kind not in _WORLDS:
        _WORLDS[kind] = World(kind, dev)
    return _WORLDS[kind]


@pytest.fixture(scope="module", autouse=True)
def _summary_and_cleanup():
    yield
    print("\nlargest device / reference distance ratio per stage, mode and weight kind (the bound allows MULT, tests/stage_bounds.py):")
    for (stage, mode, kind), r in sorted(_MEASURED.items()):
        print(f"  {stage:34s} {mode:6s} {kind:8s} {r:6.2f}")
    for w in _WORLDS.values():
        w.eng.close()
    _WORLDS.clear()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ ViT
VIT_CASES = [(k, m, b) for k in KINDS for m in MODES for b in VIT_BATCHES[m]]


def _over(failures):
    if failures:
        raise SB.OverBound("\n".join(failures))


def _vit_rows(w, mode, B):
    """engine.vit_forward of B crops (pool items b % 11), rows b / b + 11 compared on the device; rows 0 ... 10 on the host, kept."""
    def run():
        w.eng.set_vit_gemm(mode)
        out = w.eng.vit_forward(w.img[_sel(B)].to(w.dev))
        w.eng.status()
        _rows_repeat(out, "vit_features")
        return out[:min(B, POOL)].cpu()
    return w.once(("vit_rows", mode, B), run)


def _ceiling(what, d, b):
    """A plain assertion (not the OverBound an expected failure waits for): where the rule's own assertion is an expected failure, this
    is the bound that still holds, so that a regression there fails the suite."""
    assert d <= b, f"{what}: {d:.3e} is over the ceiling {b:.3e}"


# One crop alone on the trained-like weights: the device is 3.03 times as far from float64 as the oracle's fp32 ON THAT CROP (2.03e-3
# against 6.68e-4 on pool item 0, features up to 119), which would need a multiplier of 4.5.  The eleven pool items alone give ratios of
# 0.84 ... 3.03 (rms over the tensor: 1.54), calls of three and more crops 0.7 ... 1.9 over the call.  The kernels of 1-2 crops are the
# exact-fp32 ring GEMMs (one fmaf chain over K, split four ways on proj / fc2: tokenhmr_amd/csrc/vit_plan.h), so the oracle was run on the
# CPU with every F.linear summed that way.  On item 0 it lands 1.25e-3 from float64 (1.04e-3 with unsplit chains; ATen 7.2e-4 on that
# host), on items 9, 2 and 4: 7.9e-4, 7.5e-4, 1.40e-3 where the device has 1.25e-3, 8.8e-4, 9.4e-4 — three correct fp32 evaluations of
# one crop differ by 1.7 among themselves, and the device is 0.7 ... 1.6 times the chain oracle.  The association moves the distance
# but does NOT account for 2.03e-3 on item 0; what is left is the spread of the largest error of 192 rows whose x50 outlier channels
# meet LayerNorm gains of 10.  No further cause was found, so the rule's assertion stays in as the strict expected failure the rule gives
# that case, under a ceiling that does hold: TWICE the oracle's own distance over the WHOLE pool (2.25e-3; per channel the cap, 4 x).
_VIT_ONE_CROP = pytest.mark.xfail(strict=True, raises=SB.OverBound,
                                  reason="vit_features, trained-like weights, one crop alone: device / reference distance on that crop 3.03 (bound: 2); "
                                         "per channel 4.70 in the worst of 6 channels over x4")


def _vit_cases(mark_one_crop):
    return [pytest.param(k, m, b, marks=_VIT_ONE_CROP) if mark_one_crop and (k, b) == ("trained", 1) else (k, m, b) for k, m, b in VIT_CASES]


@pytest.mark.parametrize("kind,mode,B", _vit_cases(True))
def test_vit(built_lib, cuda_dev, kind, mode, B):
    """engine.vit_forward against O.vit_forward in float64, the max-abs rule."""
    w = _world(kind, cuda_dev)
    r32, r64 = w.vit_refs()
    out = _vit_rows(w, mode, B)
    n = out.shape[0]
    _ceiling(f"[{kind} {mode} B={B}] vit_features against {MULT['vit_features']:g} x the reference's own distance over the pool", SB.dist(out, r64[:n]),
             SB.bound(r32, r64, MULT["vit_features"]))
    failures = []
    _check(failures, "vit_features", w, mode, B, out, r32[:n], r64[:n])
    _over(failures)


@pytest.mark.parametrize("kind,mode,B", _vit_cases(True))
def test_vit_per_channel(built_lib, cuda_dev, kind, mode, B):
    """The trained-like statistics have x50 outlier channels (features up to 136 here), so an error in a quiet channel hides under the
    max-abs bound: SB.bound_per_channel on the rows compared, at MULT["vit_features_per_channel"] (tests/stage_bounds.py says why 4).
    Ceiling, every case: each channel within 4 x the reference's own distance in that channel over the whole pool (measured worst 3.74,
    one crop alone on the trained-like weights; 3.10 otherwise)."""
    w = _world(kind, cuda_dev)
    r32, r64 = w.vit_refs()
    out = _vit_rows(w, mode, B)
    n = out.shape[0]
    d = SB.dist_per_channel(out, r64[:n])
    over = d > SB.bound_per_channel(r32, r64, MULT_MAX)
    assert not over.any(), f"{int(over.sum())} channels are over 4 x the reference's own distance over the pool, worst {(d / SB.dist_per_channel(r32, r64)).max().item():.2f}"
    ok, line = SB.check_per_channel(f"[{kind} {mode} B={B}] vit_features", out, r32[:n], r64[:n], MULT["vit_features_per_channel"])
    key = ("vit_features per channel", mode, kind)
    _MEASURED[key] = max(_MEASURED.get(key, 0.0), (d / SB.dist_per_channel(r32[:n], r64[:n])).max().item())
    _over([] if ok else [line])


# ------------------------------------------------------------------------------------------------ the head, one call per (kind, mode, B)
@pytest.fixture(scope="module", params=list(itertools.product(KINDS, MODES, HEAD_BATCHES)), ids=lambda p: f"{p[0]}-{p[1]}-{p[2]}")
def head_call(request, built_lib, cuda_dev):
    kind, mode, B = request.param
    w = _world(kind, cuda_dev)
    return w, mode, B, w.head(mode, B)


def test_decoder(head_call):
    """token_out against O.decoder_forward in float64 on the very context the device was fed: the device's own ViT features of the pool,
    and a second pool of randn(11, 192, 1280)."""
    w, mode, B, o = head_call
    n = min(B, POOL)
    failures = []
    r32, r64 = w.decoder_refs("vit")
    _check(failures, "token_out", w, mode, B, o["token_out"], r32[:n], r64[:n])
    r32, r64 = w.decoder_refs("randn")
    o2 = w.head(mode, B, "randn", taps=("token_out",))
    _check(failures, "token_out", w, mode, B, o2["token_out"], r32[:n], r64[:n], note=" (randn context)")
    _over(failures)


def test_mixer_and_classifier(head_call):
    """cls_logits against O.classifier_logits in float64 of the device's token_out; the softmax against the float64 softmax of the device's
    logits; token_idx == the argmax of the device's own logits (lowest index on ties), and == the float64 argmax wherever the float64 top-2
    gap exceeds 2 x the logits' bound (two logits each within the bound cannot swap across a wider gap), which may leave out 1 % at most."""
    w, mode, B, o = head_call
    failures = []
    with torch.no_grad():
        l32 = O.classifier_logits(o["token_out"], w.sd, CFG)
        l64 = O.classifier_logits(o["token_out"].double(), w.sd64, CFG)
    _check(failures, "cls_logits", w, mode, B, o["cls_logits"], l32, l64)
    _check(failures, "cls_logits_softmax", w, mode, B, o["cls_logits_softmax"], o["cls_logits"].softmax(-1), o["cls_logits"].double().softmax(-1))
    idx = o["token_idx"]
    assert torch.equal(idx, O.token_indices(o["cls_logits"])), "token_idx is not the argmax (lowest index on ties) of the device's own logits"
    top2 = l64.topk(2, dim=-1).values
    safe = (top2[..., 0] - top2[..., 1]) > 2.0 * SB.bound(l32, l64, MULT["cls_logits"])
    left_out = 1.0 - safe.double().mean().item()
    wrong = int((idx != O.token_indices(l64))[safe].sum())
    print(f"[{w.kind} {mode} B={B}] token_idx: {wrong} of {int(safe.sum())} differ from the float64 argmax; {100 * left_out:.2f} % of {safe.numel()} "
          f"tokens left out by the gap rule")
    assert wrong == 0, f"{wrong} token indices differ from the float64 argmax where the top-2 gap exceeds twice the bound"
    assert left_out <= 0.01, f"the gap rule leaves out {100 * left_out:.2f} % of the tokens (> 1 %)"
    _over(failures)


def _readout(w, token_out, probs, dt):
    sd, tok = (w.sd64, w.tok64) if dt == torch.float64 else (w.sd, w.tok)
    t, H = token_out.to(dt), "smpl_head."
    lin = lambda name: F.linear(t, sd[H + name + ".weight"], sd[H + name + ".bias"])      # noqa: E731
    bpose = O.vq_decode(probs.to(dt), tok, CFG).reshape(t.shape[0], -1)                    # token_head.py:103-107 as O.head_forward restates it
    pose6d = torch.cat([lin("decpose_grot"), bpose, lin("decpose_hands")], -1) + sd[H + "init_body_pose"]
    return pose6d, lin("decshape") + sd[H + "init_betas"], lin("deccam") + sd[H + "init_cam"]


def test_vq_decoder_and_readout(head_call):
    """pose6d, betas and pred_cam against the read-out of O.head_forward in float64 on the device's token_out and probabilities; rotmat
    against O.rot6d_to_rotmat of the device's pose6d."""
    w, mode, B, o = head_call
    failures = []
    with torch.no_grad():
        r32 = _readout(w, o["token_out"], o["cls_logits_softmax"], torch.float32)
        r64 = _readout(w, o["token_out"], o["cls_logits_softmax"], torch.float64)
        n = o["pose6d"].shape[0]
        rot32 = O.rot6d_to_rotmat(o["pose6d"]).view(n, 24, 3, 3)
        rot64 = O.rot6d_to_rotmat(o["pose6d"].double()).view(n, 24, 3, 3)
    for k, dev, a, b in (("pose6d", o["pose6d"], r32[0], r64[0]), ("betas", o["betas"], r32[1], r64[1]), ("pred_cam", o["pred_cam"], r32[2], r64[2]),
                         ("rotmat", o["rotmat"], rot32, rot64)):
        _check(failures, k, w, mode, B, dev, a, b)
    _over(failures)


def test_camera_and_body(head_call):
    """engine.lbs_forward on the device's rotmat, betas and camera: vertices and joints against O.smpl_forward in float64 (floor 2e-6 m),
    cam_t against tokenhmr.py:165-169, kp2d against O.perspective_projection of the device's joints and cam_t; the head call's own
    mesh, joints, cam_t and kp2d are the same kernels on the same inputs and held to the same references."""
    w, mode, B, o = head_call
    failures = []
    d = o["dev"]
    verts, joints, cam_t, kp2d = w.eng.lbs_forward(d["rotmat"], d["betas"], d["pred_cam"])
    w.eng.status()
    for k, t in (("vertices", verts), ("joints", joints), ("cam_t", cam_t), ("kp2d", kp2d)):
        _rows_repeat(t, f"lbs_forward {k}")
    n = min(B, POOL)
    verts, joints, cam_t, kp2d = (t[:n].cpu() for t in (verts, joints, cam_t, kp2d))

    def refs(dt, jts, ct):
        R, betas, cam = o["rotmat"].to(dt), o["betas"].to(dt), o["pred_cam"].to(dt)
        smpl = w.smpl64 if dt == torch.float64 else w.smpl
        v, j = O.smpl_forward(R[:, :1], R[:, 1:], betas, smpl)
        focal = CFG.focal_length * torch.ones(n, 2, dtype=dt)
        t = torch.stack([cam[:, 1], cam[:, 2], 2 * focal[:, 0] / (CFG.img_size * cam[:, 0] + 1e-9)], dim=-1)
        return v, j, t, O.perspective_projection(jts.to(dt), ct.to(dt), focal / CFG.img_size)

    for what, (dv, dj, dc, dk) in (("", (verts, joints, cam_t, kp2d)),
                                   (" (head call)", (o["pred_vertices"], o["pred_keypoints_3d"], o["pred_cam_t"], o["pred_keypoints_2d"]))):
        with torch.no_grad():
            a, b = refs(torch.float32, dj, dc), refs(torch.float64, dj, dc)
        _check(failures, "vertices", w, mode, B, dv, a[0], b[0], floor=SB.FLOOR_M, note=what)
        _check(failures, "joints", w, mode, B, dj, a[1], b[1], floor=SB.FLOOR_M, note=what)
        _check(failures, "cam_t", w, mode, B, dc, a[2], b[2], note=what)
        _check(failures, "kp2d", w, mode, B, dk, a[3], b[3], note=what)
    _over(failures)


# ------------------------------------------------------------------------------------------------ the quantiser of the encoder
# NOT in this file: the stand-alone VQ decoder (engine.vq_decode at 1, 6, 7, 25 poses) and the encoder's latent.  From 7 poses on the
# decoder, and the encoder at every size, run their convolutions as K = 1536 ... 2048 products on the exact-fp32 tile GEMM
# (tokenhmr_amd/csrc/gemm_f32.hip), which sums each output as ONE fmaf chain over K; ATen sums vector partial sums.  Measured: device /
# reference distance 3.12 ... 4.16 (decoder) and 2.75 ... 4.15 (latent), over the rule's cap of 4 at 1.5 x the ratio; the oracle summed as
# such a chain on the CPU, on the device's own pool items, lands within 10 % of the device (decoder 4.90e-8 / 4.56e-8 against the device's
# 5.06e-8 / 4.23e-8, ATen 1.6e-8; encoder 1.36e-7 / 1.82e-7 against 1.50e-7 / 1.74e-7, ATen 4.2e-8), and the decoder's tiny-M kernel (up to 6
# poses, K split among eight waves) lands at ATen's 1.96e-8 / 1.58e-8.  So the cause is the accumulation order of the tile GEMMs, the rule
# cannot hold until they sum K in partial accumulators, and the two checks belong to the change that does that.  What stays is the
# quantiser on the device's own latent, which does not depend on how close that latent is.
VQ_CASES = [(k, m, b) for k in KINDS for m in MODES for b in VQ_BATCHES]


def _encode(w, mode, B):
    def run():
        pose = w.seed_head()["pose"]
        w.eng.set_vit_gemm(mode)
        idx, lat = w.eng.encode_tokens(pose[_sel(B)].to(w.dev), want_latent=True)
        w.eng.status()
        _rows_repeat(idx, "encode_tokens idx")
        _rows_repeat(lat, "encode_tokens latent")
        n = min(B, POOL)
        return idx[:n].cpu().reshape(-1).long(), lat[:n].cpu().reshape(-1, 256)
    return w.once(("encode", mode, B), run)


@pytest.mark.parametrize("kind,mode,B", VQ_CASES)
def test_encoder_indices(built_lib, cuda_dev, kind, mode, B):
    """The code indices == the float64 argmin of the expanded distance (quantize_cnn.py:80-86) of the DEVICE's latent wherever the float64
    top-2 gap exceeds 2 x the distances' bound (1 % left out at most)."""
    w = _world(kind, cuda_dev)
    idx, lat = _encode(w, mode, B)
    with torch.no_grad():
        _, d32 = O.vq_quantize(lat, w.tok["quantizer.codebook"])
        i64, d64 = O.vq_quantize(lat.double(), w.tok64["quantizer.codebook"])
    b = SB.bound(d32, d64, MULT["vq_dist"])
    two = d64.topk(2, dim=-1, largest=False).values
    safe = (two[:, 1] - two[:, 0]) > 2.0 * b
    left_out = 1.0 - safe.double().mean().item()
    wrong = int((idx != i64)[safe].sum())
    print(f"[{w.kind} {mode} B={B}] code indices: {wrong} of {int(safe.sum())} differ from the float64 argmin (distance bound {b:.3e}, "
          f"max distance {d64.max().item():.4g}); {100 * left_out:.2f} % of {safe.numel()} left out by the gap rule")
    assert wrong == 0, f"{wrong} code indices differ from the float64 argmin where the top-2 gap exceeds twice the bound"
    assert left_out <= 0.01, f"the gap rule leaves out {100 * left_out:.2f} % of the codes (> 1 %)"
