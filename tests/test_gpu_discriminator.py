"""thmr_disc_forward / thmr_disc_backward, tokenhmr_amd.discriminator.Discriminator and the adversarial term of the loss surfaces on the
device.

Truth is the reference's own record at B = 8 (tests/golden/discriminator.npz: its class in float32 and float64 under autograd) and the torch
restatement tests/discriminator_oracle.py at the other sizes (pinned to the reference in tests/test_discriminator_host.py).  The bound is
the project's rule (tests/stage_bounds.py): the device may be MULT x as far from float64 as torch float32 on the CPU is on the same inputs,
with the 4-ulp floor; every check prints the measured ratio.  The seeds are accepted by discriminator_oracle.accept (no ReLU
pre-activation close enough to 0 for a precision to flip it; asserted for these shapes in the host test).

Both entry points take their outputs as a host table (`float** bufs_host`), so tests/test_gpu_guard_bands.py::CASES cannot list them:
their guard-band cases are test_guard_bands below."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

import discriminator_oracle as DO
import stage_bounds as SB
from tests import guarded as G
from tokenhmr_amd import _cabi, ops
from tokenhmr_amd import weights as W
from tokenhmr_amd.discriminator import Discriminator

pytestmark = pytest.mark.gpu

MULT = 2.0
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _inputs(B):
    return DO.make_inputs(B, DO.GPU_SEED[B])


@functools.lru_cache(maxsize=None)
def _truth(B):
    """({key: float32 tensor}, {key: float64 tensor}): the fixture at B = 8, the oracle elsewhere; computed once per size."""
    if B == DO.BATCH:
        g = np.load(os.path.join(GOLDEN_DIR, "discriminator.npz"))
        assert all(np.array_equal(g["in." + k], v) for k, v in _inputs(B).items())
        return tuple({k[4:]: torch.from_numpy(np.atleast_1d(g[k])) for k in g.files if k.startswith(p)} for p in ("f32.", "f64."))
    return tuple({k: torch.from_numpy(np.atleast_1d(v)) for k, v in DO.run(_inputs(B), dt).items()} for dt in (torch.float32, torch.float64))


@pytest.fixture(scope="module")
def disc(built_lib, cuda_dev):
    return Discriminator(cuda_dev).load_state_dict(W.make_synthetic_discriminator(DO.WEIGHT_SEED))


def _dev(B, dev):
    return {k: torch.from_numpy(v).to(dev) for k, v in _inputs(B).items()}


def _ws(B, dev):
    """A workspace of exactly the documented size, poisoned: it needs no initialisation, the pad columns of fc1's operand included."""
    return torch.full((_cabi.DISC_WS_PER_ITEM * B,), NAN, device=dev)


def _forward(D, t, B, target=None, poses=None, stride=207):
    out, loss = torch.full((B, 25), NAN, device=D.device), torch.full((), NAN, device=D.device)
    D.forward_raw(t["poses"] if poses is None else poses, stride, t["betas"], B, out, loss=None if target is None else loss,
                  target=0.0 if target is None else target, workspace=_ws(B, D.device))
    return out, loss


def _backward(D, t, B, target=1.0, grad_out=None, want=("poses", "betas"), poses=None, stride=207, value=True):
    f = lambda *s: torch.full(s, NAN, device=D.device)      # noqa: E731
    out, loss = (f(B, 25), f()) if value else (None, None)
    gp, gb = f(B, 23, 3, 3) if "poses" in want else None, f(B, 10) if "betas" in want else None
    D.backward_raw(t["poses"] if poses is None else poses, stride, t["betas"], B, grad_out=grad_out, target=target, out=out,
                   loss=loss if grad_out is None else None, grad_poses=gp, grad_betas=gb, workspace=_ws(B, D.device))
    return out, loss, gp, gb


def _check(fails, tag, got, r32, r64, per_column=False):
    assert torch.isfinite(got).all(), f"{tag}: an element was left unwritten or is not finite"
    ok, line = SB.check(tag, got.detach().cpu().reshape(r64.shape), r32, r64, MULT)
    fails += [] if ok else [line]
    if per_column:
        # Column by column against the TENSOR's bound, so that a failure names its column.  The 25 columns share one scale — each is an
        # O(1) sum of O(0.1 ... 1) terms, and where the terms cancel the error does not shrink with the value — so the rule's 4-ulp floor
        # is that of the tensor's largest element, and at B = 1 a column's own float32 distance is a single draw, not a scale.  A swapped
        # or mis-paired column is off by the columns' distance, O(0.1) (the host test holds the 25 values apart): 10^5 bounds.
        b = SB.bound(r32, r64, MULT)
        d = (got.detach().cpu().double() - r64).abs().max(dim=0).values
        own = (r32.double() - r64).abs().max(dim=0).values
        print(f"{tag}, per column device / reference's own fp32: " + " ".join(f"{x / y if y > 0 else float('inf'):.2f}" for x, y in zip(d.tolist(), own.tolist())))
        fails += [f"{tag}: column {c}: device {d[c].item():.3e}, bound {b:.3e}" for c in range(d.numel()) if d[c].item() > b]


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("B", DO.GPU_BATCHES)
def test_forward_and_the_two_losses(disc, B):
    """out column by column (a wrong joint -> head pairing, a j * 32 + c flatten or swapped columns 23 / 24 move single columns), L(0) and
    L(1); the stride-216 view of a (B,24,3,3) buffer whose joint 0 is NaN; two runs."""
    t, (r32, r64) = _dev(B, disc.device), _truth(B)
    out0, l0 = _forward(disc, t, B, target=0.0)
    out1, l1 = _forward(disc, t, B, target=1.0)
    plain, _ = _forward(disc, t, B)
    joined = torch.full((B, 24, 3, 3), NAN, device=disc.device)
    joined[:, 1:] = t["poses"]
    view = joined[:, 1:]
    assert view.stride(0) == 216 and view.data_ptr() == joined.data_ptr() + 36
    outv, lv = _forward(disc, t, B, target=1.0, poses=view, stride=216)
    torch.cuda.synchronize()
    assert torch.equal(out0, out1) and torch.equal(out0, plain) and torch.equal(outv, out1) and torch.equal(lv, l1)
    fails = []
    _check(fails, f"B = {B}: out", out1, r32["out"], r64["out"], per_column=True)
    _check(fails, f"B = {B}: L(0)", l0, r32["loss_fake"], r64["loss_fake"])
    _check(fails, f"B = {B}: L(1)", l1, r32["loss_adv"], r64["loss_adv"])
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("B", DO.GPU_BATCHES)
def test_backward_against_float64_autograd(disc, B):
    """The gradient of L(1) and of sum(out * grad_out) by poses and betas; every call on a poisoned workspace and without a preceding
    forward; a call's own out and loss are the forward's; a NULL gradient changes nothing of the other."""
    t, (r32, r64) = _dev(B, disc.device), _truth(B)
    fout, floss = _forward(disc, t, B, target=1.0)
    out, loss, gp, gb = _backward(disc, t, B, target=1.0)
    again = _backward(disc, t, B, target=1.0)
    _, _, vp, vb = _backward(disc, t, B, grad_out=t["grad_out"])
    _, _, gp_only, none_b = _backward(disc, t, B, target=1.0, want=("poses",), value=False)
    _, _, none_p, gb_only = _backward(disc, t, B, target=1.0, want=("betas",), value=False)
    joined = torch.full((B, 24, 3, 3), NAN, device=disc.device)
    joined[:, 1:] = t["poses"]
    _, _, gpv, gbv = _backward(disc, t, B, target=1.0, poses=joined[:, 1:], stride=216)
    torch.cuda.synchronize()
    assert torch.equal(out, fout) and torch.equal(loss, floss)
    for a, b in zip((out, loss, gp, gb), again):
        assert torch.equal(a, b), "two runs differ"
    assert none_b is None and none_p is None and torch.equal(gp_only, gp) and torch.equal(gb_only, gb)
    assert torch.equal(gpv, gp) and torch.equal(gbv, gb)
    fails = []
    _check(fails, f"B = {B}: d L(1) / d poses", gp, r32["grad_poses"], r64["grad_poses"])
    _check(fails, f"B = {B}: d L(1) / d betas", gb, r32["grad_betas"], r64["grad_betas"])
    _check(fails, f"B = {B}: grad_out's product by poses", vp, r32["vjp_poses"], r64["vjp_poses"])
    _check(fails, f"B = {B}: grad_out's product by betas", vb, r32["vjp_betas"], r64["vjp_betas"])
    assert not fails, "\n".join(fails)


def test_captured_forward_and_backward(disc):
    """A forward and a backward captured in one graph on one stream, replayed on changed input contents: bit-equal to eager."""
    B = 3
    cases = [{k: torch.from_numpy(v).to(disc.device) for k, v in DO.make_inputs(B, 1000 + 7 * k).items()} for k in range(3)]
    t = {k: v.clone() for k, v in cases[0].items()}
    f = lambda *s: torch.full(s, NAN, device=disc.device)      # noqa: E731
    out, loss, bout, bloss, gp, gb, ws = f(B, 25), f(), f(B, 25), f(), f(B, 23, 3, 3), f(B, 10), _ws(B, disc.device)

    def run():
        disc.forward_raw(t["poses"], 207, t["betas"], B, out, loss=loss, target=0.0, workspace=ws)
        disc.backward_raw(t["poses"], 207, t["betas"], B, target=1.0, out=bout, loss=bloss, grad_poses=gp, grad_betas=gb, workspace=ws)

    eager = []
    for k in range(3):
        for key in t:
            t[key].copy_(cases[k][key])
        run()
        torch.cuda.synchronize()
        eager.append([x.clone() for x in (out, loss, bout, bloss, gp, gb)])
    assert not torch.equal(eager[1][4], eager[2][4])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for k in (1, 2):
        for key in t:
            t[key].copy_(cases[k][key])
        for x in (out, loss, bout, bloss, gp, gb, ws):
            x.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((out, loss, bout, bloss, gp, gb), eager[k]):
            assert torch.equal(got, want), k
    del graph


# ------------------------------------------------------------------------------------------------ the Python surface
def test_autograd_surface(disc):
    B = 8
    t, (r32, r64) = _dev(B, disc.device), _truth(B)
    out_c, loss_c, gp_c, gb_c = _backward(disc, t, B, target=1.0)
    _, _, vp_c, vb_c = _backward(disc, t, B, grad_out=t["grad_out"])
    # __call__ under autograd
    p, b = t["poses"].clone().requires_grad_(True), t["betas"].clone().requires_grad_(True)
    out = disc(p, b)
    assert out.grad_fn is not None and torch.equal(out.detach(), out_c)
    out.backward(t["grad_out"])
    assert torch.equal(p.grad, vp_c) and torch.equal(b.grad, vb_c)
    # adversarial_loss(...).backward() is the C ABI's gradient, bit for bit
    p, b = t["poses"].clone().requires_grad_(True), t["betas"].clone().requires_grad_(True)
    adv = disc.adversarial_loss(p, b)
    assert adv.dim() == 0 and torch.equal(adv.detach(), loss_c)
    adv.backward()
    assert torch.equal(p.grad, gp_c) and torch.equal(b.grad, gb_c)
    # an input that asks for no gradient gets None; without grad, the plain path
    p = t["poses"].clone().requires_grad_(True)
    disc.adversarial_loss(p, t["betas"]).backward()
    assert torch.equal(p.grad, gp_c)
    with torch.no_grad():
        assert disc(p, t["betas"]).grad_fn is None
    assert torch.equal(disc(t["poses"].reshape(B, -1), t["betas"]), out_c)           # tokenhmr.py:392 hands (B,207)
    out2, loss2, gp2, gb2 = disc.value_and_grad(t["poses"], t["betas"], target=1.0)
    assert torch.equal(out2, out_c) and torch.equal(loss2, loss_c) and torch.equal(gp2, gp_c) and torch.equal(gb2, gb_c)
    # discriminator_loss: the fake branch against 0, the real branch from axis-angle against 1
    real = disc.loss(ops.aa_to_rotmat(t["gt_body_pose_aa"].reshape(-1, 3).contiguous()).view(B, 23, 3, 3), t["gt_betas"], 1.0)
    p = t["poses"].clone().requires_grad_(True)
    ld = disc.discriminator_loss(p, t["betas"], t["gt_body_pose_aa"], t["gt_betas"])
    torch.cuda.synchronize()
    assert ld.grad_fn is None                                                        # the fake branch is detached by construction
    fails = []
    _check(fails, "loss_real from axis-angle", real, r32["loss_real"], r64["loss_real"])
    _check(fails, "loss_disc", ld, r32["loss_disc"], r64["loss_disc"])
    assert not fails, "\n".join(fails)


def test_batches_above_the_maximum_are_chunked(built_lib, cuda_dev):
    B = 17
    t = _dev(B, cuda_dev)
    whole = Discriminator(cuda_dev).load_state_dict(W.make_synthetic_discriminator(DO.WEIGHT_SEED))
    small = Discriminator(cuda_dev).load_state_dict(W.make_synthetic_discriminator(DO.WEIGHT_SEED))
    small.max_batch = 8                                                              # 8 + 8 + 1
    a, b = whole.value_and_grad(t["poses"], t["betas"]), small.value_and_grad(t["poses"], t["betas"])
    torch.cuda.synchronize()
    for x, y, name in zip(a, b, ("out", "loss", "grad_poses", "grad_betas")):
        if name == "loss":                                                           # three fp64 sums added in fp32 instead of one
            assert abs(float(x) - float(y)) <= 4 * 2.0 ** -23 * abs(float(x))
        else:
            assert torch.equal(x, y), name
    with pytest.raises(_cabi.EngineError, match="THMR_DISC_MAX_BATCH"):
        small.forward_raw(torch.zeros(257, 23, 3, 3, device=cuda_dev), 207, torch.zeros(257, 10, device=cuda_dev), 257,
                          torch.zeros(257, 25, device=cuda_dev))


# ------------------------------------------------------------------------------------------------ the loss surfaces
W_ADV = 0.0005


def _loss_case(dev, B=5):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_golden_val_loss as GV
    import gen_golden_val_loss_grad as GG
    from tokenhmr_amd.model import ConfigNode
    g = np.load(os.path.join(GOLDEN_DIR, "val_loss_grad.npz"))
    th = {k[7:]: g[k] for k in g.files if k.startswith("thresh.")}
    inp = GG.make_inputs(B, 4200, thresholds=th)
    batch, output = GV.to_batch(inp, torch.float32)
    mv = lambda d: {k: (mv(v) if isinstance(v, dict) else v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}      # noqa: E731
    flags = batch.pop("smpl_params_is_axis_angle")
    batch, output = mv(batch), mv(output)
    batch["smpl_params_is_axis_angle"] = flags
    output["pred_cam"] = torch.from_numpy(inp["pred_cam"]).to(dev)
    cfg = lambda adv: ConfigNode({"MODEL": {"LOOSE_SUP": False, "LOOSE_WEIGHT": GV.LOOSE_WEIGHT, "IMAGE_SIZE": GG.IMAGE_SIZE},      # noqa: E731
                                  "LOSS_WEIGHTS": dict(GV.LOSS_WEIGHTS, **({"ADVERSARIAL": adv} if adv is not None else {})),
                                  "EXTRA": {"FOCAL_LENGTH": GG.FOCAL_LENGTH}})
    return inp, batch, output, cfg


def _adv_truth(inp):
    """(float32, float64) of loss_gen and its gradient by body_pose and betas: the oracle on the loss case's prediction."""
    d = {"poses": inp["pred_rotmat"][:, 1:].copy(), "betas": inp["pred_betas"], "gt_body_pose_aa": np.zeros((len(inp["pred_betas"]), 69), np.float32),
         "gt_betas": inp["pred_betas"], "grad_out": np.zeros((len(inp["pred_betas"]), 25), np.float32)}
    DO.accept(d)
    return tuple({k: torch.from_numpy(np.atleast_1d(v)) for k, v in DO.run(d, dt).items()} for dt in (torch.float32, torch.float64))


@pytest.mark.parametrize("with_body", [False, True])
def test_value_and_grad_with_the_adversarial_term(disc, with_body):
    """loss and the gradients = the existing result + w x the separately computed term; without a discriminator, the existing bits."""
    from tokenhmr_amd.losses import LOSS_KEYS, ValidationLoss
    dev = disc.device
    inp, batch, output, cfg = _loss_case(dev)
    B = len(inp["pred_betas"])
    body = None
    if with_body:
        from tokenhmr_amd.smpl import SMPL
        from tokenhmr_amd.smpl_assets import make_synthetic_smpl
        body = SMPL(make_synthetic_smpl(seed=0), max_batch=8, device=dev).enable_grad()
    kw = dict(body_model=body)
    base_l, base_g = ValidationLoss(cfg(None)).value_and_grad(batch, dict(output), **kw)
    base_l, base_g = {k: v.clone() for k, v in base_l.items()}, {k: v.clone() for k, v in base_g.items()}
    vl = ValidationLoss(cfg(W_ADV))
    assert vl.adversarial_weight == W_ADV and ValidationLoss(cfg(None)).adversarial_weight == 0.0
    # without a discriminator: the existing result, bit for bit, whatever the config's weight
    same_l, same_g = vl.value_and_grad(batch, dict(output), **kw)
    assert list(same_l) == list(LOSS_KEYS) and all(torch.equal(same_l[k], base_l[k]) for k in base_l)
    assert all(torch.equal(same_g[k], base_g[k]) for k in base_g)
    out_d = dict(output)
    losses, grads = vl.value_and_grad(batch, out_d, discriminator=disc, **kw)
    losses, grads = {k: v.clone() for k, v in losses.items()}, {k: v.clone() for k, v in grads.items()}
    explicit_l, explicit_g = ValidationLoss(cfg(None)).value_and_grad(batch, dict(output), discriminator=disc, adversarial_weight=W_ADV, **kw)
    assert all(torch.equal(explicit_l[k], losses[k]) for k in losses) and all(torch.equal(explicit_g[k], grads[k]) for k in grads)
    _, lg, gp, gb = disc.value_and_grad(output["pred_smpl_params"]["body_pose"], output["pred_smpl_params"]["betas"], target=1.0)
    torch.cuda.synchronize()
    assert list(losses) == list(LOSS_KEYS) + ["loss_gen"] and out_d["losses"]["loss_gen"] is not None
    assert torch.equal(losses["loss_gen"], lg) and losses["loss"].dim() == 0
    for k in LOSS_KEYS[1:]:
        assert torch.equal(losses[k], base_l[k]), k
    # the separately computed term, added by hand
    assert torch.equal(losses["loss"], torch.add(base_l["loss"], lg, alpha=W_ADV))
    assert torch.equal(grads["body_pose"], torch.add(base_g["body_pose"], gp, alpha=W_ADV))
    assert torch.equal(grads["betas"], torch.add(base_g["betas"], gb, alpha=W_ADV))
    untouched = ("global_orient", "pred_cam") if with_body else ("global_orient", "pred_keypoints_2d", "pred_keypoints_3d")
    for k in untouched:
        assert torch.equal(grads[k], base_g[k]), k
    # and to the rule: the existing result + w x the float32 / float64 truth of the term
    a32, a64 = _adv_truth(inp)
    fails = []
    for name, got, base, key in (("loss", losses["loss"], base_l["loss"], "loss_adv"), ("body_pose", grads["body_pose"], base_g["body_pose"], "grad_poses"),
                                 ("betas", grads["betas"], base_g["betas"], "grad_betas")):
        b = base.cpu()
        want32, want64 = b + W_ADV * a32[key].reshape(b.shape), b.double() + W_ADV * a64[key].reshape(b.shape)
        _check(fails, f"value_and_grad with the adversarial term ({'body model' if with_body else 'direct'}): {name}", got, want32, want64)
    _check(fails, "loss_gen", losses["loss_gen"], a32["loss_adv"], a64["loss_adv"])
    if body is not None:
        body.close()
    assert not fails, "\n".join(fails)


def test_model_surfaces_with_the_adversarial_term(disc):
    """TokenHMR.loss_value_and_grad and head_loss hand the discriminator through: the same numbers as ValidationLoss's, under autograd too."""
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd.model import TokenHMR
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    dev = disc.device
    inp, batch, _, cfg_of = _loss_case(dev, B=3)
    cfg, B = HMRConfig(vit_depth=2, dec_depth=2), 3
    model = TokenHMR.from_state(cfg, W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0), make_synthetic_smpl(cfg, 0),
                                max_batch=4, device=dev, model_cfg=cfg_of(W_ADV))
    p = {"global_orient": torch.from_numpy(inp["pred_rotmat"][:, :1]).to(dev), "body_pose": torch.from_numpy(inp["pred_rotmat"][:, 1:].copy()).to(dev),
         "betas": torch.from_numpy(inp["pred_betas"]).to(dev)}
    cam = torch.from_numpy(inp["pred_cam"]).to(dev)
    tail = model._head_output(p, cam)
    base_l, base_g = model.loss_value_and_grad(batch, dict(tail))
    base_l, base_g = {k: v.clone() for k, v in base_l.items()}, {k: v.clone() for k, v in base_g.items()}
    losses, grads = model.loss_value_and_grad(batch, dict(tail), discriminator=disc)
    want_l, want_g = {k: v.clone() for k, v in losses.items()}, {k: v.clone() for k, v in grads.items()}
    _, lg, gp, gb = disc.value_and_grad(p["body_pose"], p["betas"], target=1.0)
    assert torch.equal(want_l["loss"], torch.add(base_l["loss"], lg, alpha=W_ADV)) and torch.equal(want_l["loss_gen"], lg)
    assert torch.equal(want_g["body_pose"], torch.add(base_g["body_pose"], gp, alpha=W_ADV))
    assert torch.equal(want_g["betas"], torch.add(base_g["betas"], gb, alpha=W_ADV))
    assert torch.equal(want_g["global_orient"], base_g["global_orient"]) and torch.equal(want_g["pred_cam"], base_g["pred_cam"])
    # head_loss: without a discriminator the existing total; with one, value and gradients of loss_value_and_grad
    assert torch.equal(model.head_loss(batch, p, cam), base_l["loss"])
    assert torch.equal(model.head_loss(batch, p, cam, discriminator=disc), want_l["loss"])
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    cam_leaf = cam.clone().requires_grad_(True)
    total = model.head_loss(batch, leaves, cam_leaf, discriminator=disc)
    assert total.grad_fn is not None and torch.equal(total.detach(), want_l["loss"])
    total.backward()
    torch.cuda.synchronize()
    for k in ("global_orient", "body_pose", "betas"):
        assert torch.equal(leaves[k].grad, want_g[k]), k
    assert torch.equal(cam_leaf.grad, want_g["pred_cam"])
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    model.head_loss(batch, leaves, cam).backward()                                   # no discriminator: the existing gradient
    assert torch.equal(leaves["body_pose"].grad, base_g["body_pose"]) and torch.equal(leaves["betas"].grad, base_g["betas"])
    model.engine.status()
    model.body_model.close()
    model.engine.close()


# ------------------------------------------------------------------------------------------------ the C calls: guard bands, refusals
def _p(t):
    return None if t is None else t.data_ptr()


def _c_forward(lib, D, poses, stride, betas, B, out, loss, ws, div=0, target=0.0, weights=0, table=True):
    tb = (C.c_void_p * _cabi.DISC_SLOTS)(_p(out), _p(loss), None, None, _p(ws))
    rc = lib.thmr_disc_forward(D.weights.data_ptr() if weights == 0 else weights, _p(poses), stride, _p(betas), B, div, target,
                               tb if table else None, None)
    return rc, (lib.thmr_last_error(None) or b"").decode()


def _c_backward(lib, D, poses, stride, betas, grad_out, B, out, loss, gp, gb, ws, div=0, target=1.0, weights=0, table=True):
    tb = (C.c_void_p * _cabi.DISC_SLOTS)(_p(out), _p(loss), _p(gp), _p(gb), _p(ws))
    rc = lib.thmr_disc_backward(D.weights.data_ptr() if weights == 0 else weights, _p(poses), stride, _p(betas), _p(grad_out), B, div, target,
                                tb if table else None, None)
    return rc, (lib.thmr_last_error(None) or b"").decode()


@pytest.mark.parametrize("B", [1, 5])
def test_guard_bands(disc, built_lib, B):
    """Every input, output and the workspace is a window of a canary buffer (poses: the stride-216 rows of one): nothing outside a window
    is written, no input changes, every output element is written, and the outputs equal the plain call's bit for bit."""
    dev = disc.device
    t = {k: torch.from_numpy(v).to(dev) for k, v in DO.make_inputs(B, 1000).items()}
    want_f = _forward(disc, t, B, target=0.0)
    want_b = _backward(disc, t, B, target=1.0)
    want_v = _backward(disc, t, B, grad_out=t["grad_out"])
    torch.cuda.synchronize()
    for mode in ("forward", "backward", "grad_out"):
        checks, ins = [], {}
        rows, chk = G.guarded(B, 207, 216, col0=9, device=dev, fill=t["poses"].reshape(B, 207))
        ins["poses"] = rows
        checks.append(("poses", chk))
        for k in ("betas", "grad_out"):
            ins[k], chk = G.guarded_like(tuple(t[k].shape), device=dev, fill=t[k])
            checks.append((k, chk))
        outs = {}
        for k, shape in (("out", (B, 25)), ("loss", ()), ("gp", (B, 23, 3, 3)), ("gb", (B, 10)), ("ws", (_cabi.DISC_WS_PER_ITEM * B,))):
            outs[k], chk = G.guarded_like(shape, device=dev)
            checks.append((k, chk))
        if mode == "forward":
            rc, msg = _c_forward(built_lib, disc, ins["poses"], 216, ins["betas"], B, outs["out"], outs["loss"], outs["ws"])
            want = dict(out=want_f[0], loss=want_f[1])
        else:
            go = ins["grad_out"] if mode == "grad_out" else None
            rc, msg = _c_backward(built_lib, disc, ins["poses"], 216, ins["betas"], go, B, outs["out"], None if go is not None else outs["loss"],
                                  outs["gp"], outs["gb"], outs["ws"])
            w = want_v if go is not None else want_b
            want = dict(out=w[0], gp=w[2], gb=w[3], **({} if go is not None else {"loss": w[1]}))
        assert rc == 0, msg
        torch.cuda.synchronize()
        for k, chk in checks:
            try:
                chk()
            except AssertionError as e:
                raise AssertionError(f"{mode}, {k}: {e}") from None
        assert torch.equal(ins["poses"], t["poses"].reshape(B, 207)) and torch.equal(ins["betas"], t["betas"]), "an input was written"
        assert torch.equal(ins["grad_out"], t["grad_out"])
        for k, v in want.items():
            assert not bool(G.holds_canary(outs[k]).any()), f"{mode}, {k}: an element was never written"
            assert torch.equal(outs[k], v), (mode, k)
        for k in set(outs) - set(want) - {"ws"}:
            assert bool(G.holds_canary(outs[k]).all()), f"{mode}: {k} was written although it was not passed"


def test_refusals(disc, built_lib):
    """Everything the header lists: THMR_ERR_INVALID with a message, before any HIP call — the outputs stay as they were."""
    dev, B = disc.device, 5
    t = {k: torch.from_numpy(v).to(dev) for k, v in DO.make_inputs(B, 1000).items()}
    f = lambda *s: torch.full(s, -3.0, device=dev)      # noqa: E731
    out, loss, gp, gb, ws = f(B, 25), f(), f(B, 23, 3, 3), f(B, 10), f(_cabi.DISC_WS_PER_ITEM * B + 4)
    inf = float("inf")
    fwd = dict(poses=t["poses"], stride=207, betas=t["betas"], B=B, out=out, loss=loss, ws=ws)
    bwd = dict(poses=t["poses"], stride=207, betas=t["betas"], grad_out=None, B=B, out=out, loss=loss, gp=gp, gb=gb, ws=ws)
    shared = [dict(weights=None), dict(poses=None), dict(betas=None), dict(table=False), dict(ws=None), dict(B=0), dict(B=-1),
              dict(B=_cabi.DISC_MAX_BATCH + 1), dict(B=2 ** 31 - 1), dict(stride=206), dict(stride=0), dict(stride=-216), dict(div=-1),
              dict(weights=disc.weights.data_ptr() + 4), dict(ws=ws[1:]), dict(target=NAN), dict(target=inf), dict(target=-inf)]
    for kw in shared + [dict(out=None)]:
        rc, msg = _c_forward(built_lib, disc, **{**fwd, **kw})
        assert rc == _cabi.ERR_INVALID and "disc_forward" in msg, (kw, rc, msg)
    for kw in shared + [dict(gp=None, gb=None), dict(grad_out=t["grad_out"], target=NAN)]:         # the last: LOSS still reads the target
        rc, msg = _c_backward(built_lib, disc, **{**bwd, **kw})
        assert rc == _cabi.ERR_INVALID and "disc_backward" in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    for name, x in (("out", out), ("loss", loss), ("grad_poses", gp), ("grad_betas", gb), ("workspace", ws)):
        assert (x == -3.0).all(), f"a refused call wrote {name}"
    # a target that is not read is not checked: no LOSS in the forward; grad_out and no LOSS in the backward
    rc, msg = _c_forward(built_lib, disc, **{**fwd, "loss": None, "target": NAN})
    assert rc == 0, msg
    rc, msg = _c_backward(built_lib, disc, **{**bwd, "loss": None, "grad_out": t["grad_out"], "target": NAN})
    assert rc == 0, msg
    torch.cuda.synchronize()
    want = _backward(disc, t, B, grad_out=t["grad_out"])
    assert torch.equal(out, want[0]) and torch.equal(gp, want[2]) and torch.equal(gb, want[3]) and (loss == -3.0).all()
    with pytest.raises(RuntimeError, match="load_state_dict"):
        Discriminator(dev)(t["poses"], t["betas"])
