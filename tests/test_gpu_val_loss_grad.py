"""thmr_val_loss_grad, ValidationLoss.value_and_grad and TokenHMR.loss_value_and_grad / head_loss on the device.

Truth is float64 torch autograd of a restatement of compute_loss (tests/val_loss_grad_oracle.py::torch_grads, pinned to the reference's own
float64 autograd in tests/test_val_loss_grad_host.py).  The bound is the project's rule (tests/stage_bounds.py): the device may be MULT x
as far from float64 as the same torch computation in float32 on the CPU is on the same inputs, with the 4-ulp floor.  Every check prints
the measured ratio.  The inputs' conditions (no difference or threshold close enough for a precision to flip a sign or a mask) are
asserted for these seeds and shapes in tests/test_val_loss_grad_host.py.

The entry point takes its outputs as a host table (`float** grads_host`), so tests/test_gpu_guard_bands.py::CASES cannot list it; its
guard-band cases are test_guard_bands below."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

import lbs_backward_numpy as LB
import stage_bounds as SB
import val_loss_grad_oracle as GO
from tests import guarded as G
from tokenhmr_amd import _cabi, ops
from tokenhmr_amd.losses import LOSS_KEYS, ValidationLoss
from tokenhmr_amd.model import ConfigNode

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_golden_val_loss as GV              # noqa: E402
import gen_golden_val_loss_grad as GG         # noqa: E402

pytestmark = pytest.mark.gpu

MULT = 2.0
WEIGHTS = [GV.LOSS_WEIGHTS[k] for k in ("KEYPOINTS_2D", "KEYPOINTS_3D", "GLOBAL_ORIENT", "BODY_POSE", "BETAS")]
IN_KEYS = ("pred_keypoints_2d", "pred_keypoints_3d", "pred_rotmat", "pred_betas", "gt_keypoints_2d", "gt_keypoints_3d", "gt_pose", "gt_betas",
           "has_global_orient", "has_body_pose", "has_betas")
SHAPES = {"kp2d": (44, 2), "kp3d": (44, 3), "joints": (44, 3), "cam": (3,), "rotmat": (24, 3, 3), "betas": (10,)}
F, S = GG.FOCAL_LENGTH, GG.IMAGE_SIZE


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@functools.lru_cache(maxsize=None)
def _thresholds():
    g = np.load(os.path.join(GOLDEN_DIR, "val_loss_grad.npz"))
    return {k[7:]: g[k] for k in g.files if k.startswith("thresh.")}


@functools.lru_cache(maxsize=None)
def _inputs(B, pelvis_id):
    return GG.make_inputs(B, GO.gpu_seed(B, pelvis_id), pelvis_id=pelvis_id, thresholds=_thresholds())


@functools.lru_cache(maxsize=None)
def _truth(B, pelvis_id, mode, gt):
    """(float32, float64) torch autograd of the six slots, once per case."""
    inp = _inputs(B, pelvis_id)
    kw = dict(loose=mode == "loose", loose_weight=GV.LOOSE_WEIGHT, thresholds=_thresholds(), valid_3d=GG.valid_3d(inp), pelvis_id=pelvis_id,
              gt_is_axis_angle=gt == "aa", focal_length=F, image_size=S)
    return GO.torch_grads(inp, WEIGHTS, torch.float32, **kw), GO.torch_grads(inp, WEIGHTS, torch.float64, **kw)


def _device_inputs(inp, dev, gt):
    th = _thresholds()
    t = {k: torch.from_numpy(np.ascontiguousarray(inp[k], dtype=np.float32)).to(dev) for k in IN_KEYS if k != "gt_pose"}
    t["gt_pose"] = torch.from_numpy(np.ascontiguousarray(inp["gt_pose_aa" if gt == "aa" else "gt_pose_rotmat"], dtype=np.float32)).to(dev)
    t["valid_3d"] = torch.from_numpy(GG.valid_3d(inp)).to(dev)
    t["kp2d_thresh"] = torch.from_numpy(th["kp2d"]).to(dev)
    t["angle_thresh"] = torch.from_numpy(np.concatenate([th["global_orient"], th["body_pose"]])).to(dev)
    t["pred_cam"] = torch.from_numpy(inp["pred_cam"]).to(dev)
    return t


def _grad(t, mode, pelvis_id=39, cam=True, **kw):
    loose = mode == "loose"
    extra = dict(valid_3d=t["valid_3d"], kp2d_thresh=t["kp2d_thresh"], angle_thresh=t["angle_thresh"]) if loose else {}
    return ops.val_loss_grad(*[t[k] for k in IN_KEYS], WEIGHTS, loose=loose, loose_weight=GV.LOOSE_WEIGHT, pelvis_id=pelvis_id,
                             pred_cam=t["pred_cam"] if cam else None, focal_length=F, image_size=S, **extra, **kw)


# ------------------------------------------------------------------------------------------------ parity of the six slots
@pytest.mark.parametrize("mode,gt", GG.CASES)
@pytest.mark.parametrize("B,pelvis_id", GO.GPU_SHAPES)
def test_parity_of_the_six_slots(built_lib, cuda_dev, B, pelvis_id, mode, gt):
    inp = _inputs(B, pelvis_id)
    r32, r64 = _truth(B, pelvis_id, mode, gt)
    t = _device_inputs(inp, cuda_dev, gt)
    out = {k: torch.full((B,) + SHAPES[k], float("nan"), device=cuda_dev) for k in GO.SLOTS}
    got = _grad(t, mode, pelvis_id, out=out)
    again = _grad(t, mode, pelvis_id)
    torch.cuda.synchronize()
    fails = []
    for k in GO.SLOTS:
        assert got[k].data_ptr() == out[k].data_ptr() and torch.isfinite(got[k]).all(), f"{k}: an element was left unwritten or is not finite"
        assert torch.equal(got[k], again[k]), f"{k}: two runs differ"
        ok, line = SB.check(f"B = {B}, pelvis {pelvis_id}, {mode} {gt}: {k}", got[k].cpu(), r32[k], r64[k], MULT)
        fails += [] if ok else [line]
    # sign(0) = 0 at the planted keypoint: an exact zero in the 2D and the 3D slot
    assert (got["kp2d"][0, GG.PLANT] == 0).all() and (got["kp3d"][0, GG.PLANT] == 0).all()
    assert (r64["kp2d"][0, GG.PLANT] == 0).all() and (r64["kp3d"][0, GG.PLANT] == 0).all()
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ slot selection
@pytest.mark.parametrize("mode,gt", [("plain", "mat"), ("loose", "aa")])
def test_slot_selection(built_lib, cuda_dev, mode, gt):
    t = _device_inputs(_inputs(5, 39), cuda_dev, gt)
    full = _grad(t, mode)
    assert list(full) == list(GO.SLOTS)
    for k in GO.SLOTS:
        one = _grad(t, mode, want=[k])
        assert list(one) == [k] and torch.equal(one[k], full[k]), k
    direct = _grad(t, mode, cam=False)
    assert list(direct) == ["kp2d", "kp3d", "rotmat", "betas"]
    for k in direct:
        assert torch.equal(direct[k], full[k]), k
    with pytest.raises(ValueError, match="pred_cam"):
        _grad(t, mode, cam=False, want=["joints"])
    with pytest.raises(ValueError):
        _grad(t, mode, want=[])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ composition with the body model
def _cfg(loose):
    return ConfigNode({"MODEL": {"LOOSE_SUP": loose, "LOOSE_WEIGHT": GV.LOOSE_WEIGHT, "IMAGE_SIZE": S}, "LOSS_WEIGHTS": dict(GV.LOSS_WEIGHTS),
                       "EXTRA": {"FOCAL_LENGTH": F}})


def _dicts(inp, dev):
    """The reference's batch and output dicts on the device, with output['pred_cam']."""
    batch, output = GV.to_batch(inp, torch.float32)
    mv = lambda d: {k: (mv(v) if isinstance(v, dict) else v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}      # noqa: E731
    flags = batch.pop("smpl_params_is_axis_angle")          # host flags: read without a synchronisation
    batch, output = mv(batch), mv(output)
    batch["smpl_params_is_axis_angle"] = flags
    output["pred_cam"] = torch.from_numpy(inp["pred_cam"]).to(dev)
    return batch, output


@pytest.fixture(scope="module")
def body(cuda_dev):
    from tokenhmr_amd.smpl import SMPL
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    smpl = make_synthetic_smpl(seed=0)
    m = SMPL(smpl, max_batch=64, device=cuda_dev).enable_grad()
    yield smpl, m
    m.close()


def _smpl_truth32(smpl, R, betas, gJ):
    """float32 torch autograd through the oracle's body model: (grad_R, grad_betas) of sum(joints * gJ)."""
    from oracle import tokenhmr_oracle as O
    R, betas = R.float().clone().requires_grad_(True), betas.float().clone().requires_grad_(True)
    _, j = O.smpl_forward(R[:, :1], R[:, 1:], betas, smpl)
    return torch.autograd.grad((j * gJ.float()).sum(), (R, betas))


@pytest.mark.parametrize("B,mode", [(5, "plain"), (5, "loose"), (67, "loose")])
def test_value_and_grad_composes_with_the_body_model(built_lib, cuda_dev, body, B, mode):
    """67 items through a handle of max_batch 64: the chunk loop."""
    from tokenhmr_amd.smpl import SMPL
    smpl, m = body
    loose = mode == "loose"
    inp = _inputs(B, 39)
    batch, output = _dicts(inp, cuda_dev)
    vl = ValidationLoss(_cfg(loose), thresholds=_thresholds())
    losses, grads = vl.value_and_grad(batch, output, body_model=m, train=loose, focal_length=F, image_size=S)
    assert list(losses) == list(LOSS_KEYS) and sorted(grads) == ["betas", "body_pose", "global_orient", "pred_cam"]
    assert grads["global_orient"].shape == (B, 1, 3, 3) and grads["body_pose"].shape == (B, 23, 3, 3) and grads["betas"].shape == (B, 10)
    assert grads["pred_cam"].shape == (B, 3)
    # the value: what __call__ sets, bit for bit
    plain_out = {k: output[k] for k in ("pred_smpl_params", "pred_keypoints_2d", "pred_keypoints_3d")}
    ValidationLoss(_cfg(loose), thresholds=_thresholds())(batch, plain_out, train=loose)
    for k in LOSS_KEYS:
        assert torch.equal(losses[k], plain_out["losses"][k]) and losses[k].dim() == 0, k
    assert torch.equal(output["loss_per_item"], plain_out["loss_per_item"])
    # the gradient, assembled by hand: thmr_smpl_backward(JOINTS) of ALL items in one call + the direct terms
    t = _device_inputs(inp, cuda_dev, "aa")
    slots = _grad(t, mode)
    whole = m if B <= m.max_batch else SMPL(smpl, max_batch=B, device=cuda_dev).enable_grad()
    gR, gb = torch.empty(B, 24, 3, 3, device=cuda_dev), torch.empty(B, 10, device=cuda_dev)
    whole._backward(t["pred_rotmat"], False, t["pred_betas"], B, None, slots["joints"], gR, gb)
    hand_R, hand_b = gR + slots["rotmat"], gb + slots["betas"]
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([grads["global_orient"], grads["body_pose"]], 1), hand_R)
    assert torch.equal(grads["betas"], hand_b) and torch.equal(grads["pred_cam"], slots["cam"])
    if whole is not m:
        whole.close()
    # against float64: tests/lbs_backward_numpy.py fed the float64 truth of JOINTS, plus the direct terms
    r32, r64 = _truth(B, 39, mode, "aa")
    R64, b64 = inp["pred_rotmat"].astype(np.float64), inp["pred_betas"].astype(np.float64)
    bR, bb = LB.smpl_backward(R64, b64, None, r64["joints"].numpy(), smpl)
    want64 = (torch.from_numpy(bR) + r64["rotmat"], torch.from_numpy(bb) + r64["betas"])
    sR, sb = _smpl_truth32(smpl, torch.from_numpy(inp["pred_rotmat"]), torch.from_numpy(inp["pred_betas"]), r32["joints"])
    want32 = (sR + r32["rotmat"], sb + r32["betas"])
    fails = []
    for name, got, a, b in (("rotation matrices", hand_R, want32[0], want64[0]), ("betas", hand_b, want32[1], want64[1]),
                            ("pred_cam", grads["pred_cam"], r32["cam"], r64["cam"])):
        ok, line = SB.check(f"value_and_grad, B = {B}, {mode}: total gradient by the {name}", got.cpu(), a, b, MULT)
        fails += [] if ok else [line]
    # without a body model: the five plain partial derivatives
    _, direct = vl.value_and_grad(batch, output, train=loose)
    assert sorted(direct) == ["betas", "body_pose", "global_orient", "pred_keypoints_2d", "pred_keypoints_3d"]
    for k, s in (("pred_keypoints_2d", "kp2d"), ("pred_keypoints_3d", "kp3d"), ("betas", "betas")):
        assert torch.equal(direct[k], slots[s]), k
    assert torch.equal(torch.cat([direct["global_orient"], direct["body_pose"]], 1), slots["rotmat"])
    with pytest.raises(ValueError, match="pred_cam"):
        vl.value_and_grad(batch, {k: v for k, v in output.items() if k != "pred_cam"}, body_model=m, train=loose)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ the autograd surface
def test_head_loss_is_loss_value_and_grad_under_autograd(built_lib, cuda_dev):
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd.model import TokenHMR
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    cfg, B = HMRConfig(vit_depth=2, dec_depth=2), 3
    model = TokenHMR.from_state(cfg, W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0), make_synthetic_smpl(cfg, 0),
                                max_batch=4, device=cuda_dev, model_cfg=_cfg(False))
    assert model.body_model is None                                   # built on first use only
    batch, _ = _dicts(GG.make_inputs(B, 700, thresholds=_thresholds()), cuda_dev)
    batch["img"] = torch.randn(B, 3, 256, 256, generator=torch.Generator().manual_seed(1)).to(cuda_dev)
    out = model.forward(batch)
    p = {k: v.clone() for k, v in out["pred_smpl_params"].items()}
    cam = out["pred_cam"].clone()
    # the reference: loss_value_and_grad on the engine's own tail of these head outputs
    tail = model._head_output(p, cam)
    losses, grads = model.loss_value_and_grad(batch, tail)
    assert model.body_model is not None
    want = {k: v.clone() for k, v in grads.items()}
    want_loss = losses["loss"].clone()
    same_tail = all(torch.equal(tail[k], out[k]) for k in ("pred_keypoints_2d", "pred_keypoints_3d"))
    print(f"Engine.lbs_forward on the head's outputs {'equals' if same_tail else 'differs from'} forward()'s keypoints bit for bit")
    leaves = {k: v.clone().requires_grad_(k != "betas") for k, v in p.items()}
    cam_leaf = cam.clone().requires_grad_(True)
    total = model.head_loss(batch, leaves, cam_leaf)
    assert total.dim() == 0 and total.grad_fn is not None and torch.equal(total.detach(), want_loss)
    g_cam, = torch.autograd.grad(total, cam_leaf, create_graph=True, retain_graph=True)
    with pytest.raises(RuntimeError):                                 # once differentiable
        g_cam.sum().backward()
    total.backward()
    torch.cuda.synchronize()
    assert torch.equal(leaves["global_orient"].grad, want["global_orient"]) and torch.equal(leaves["body_pose"].grad, want["body_pose"])
    assert torch.equal(cam_leaf.grad, want["pred_cam"]) and torch.equal(g_cam.detach(), want["pred_cam"])
    assert leaves["betas"].grad is None                               # an input that asks for no gradient gets None
    assert torch.isfinite(cam_leaf.grad).all() and cam_leaf.grad.abs().max() > 0
    with torch.no_grad():
        quiet = model.head_loss(batch, leaves, cam_leaf)
    assert quiet.grad_fn is None and torch.equal(quiet, want_loss)
    assert model.head_loss(batch, p, cam).grad_fn is None             # no input requires grad: the plain path
    bare = TokenHMR.from_engine(model.engine, model_cfg=_cfg(False))
    with pytest.raises(ValueError, match="body_model="):
        bare.loss_value_and_grad(batch, tail)
    _, g2 = bare.loss_value_and_grad(batch, tail, body_model=model.body_model)
    assert torch.equal(g2["pred_cam"], want["pred_cam"])
    model.engine.status()
    model.body_model.close()
    model.engine.close()


# ------------------------------------------------------------------------------------------------ capture
def test_value_and_grad_captured(built_lib, cuda_dev, body):
    """value_and_grad with a body model captured in one graph on one stream, replayed twice on changed input contents: bit-equal to eager."""
    _, m = body
    B = 5
    cases = [_dicts(GG.make_inputs(B, 5000 + k, thresholds=_thresholds()), cuda_dev) for k in range(3)]
    batch, output = _dicts(GG.make_inputs(B, 5000, thresholds=_thresholds()), cuda_dev)
    vl = ValidationLoss(_cfg(False))

    def load(k):
        for dst, src in ((batch, cases[k][0]), (output, cases[k][1])):
            for key, v in src.items():
                if isinstance(v, dict):
                    for kk, vv in v.items():
                        dst[key][kk].copy_(vv)
                elif torch.is_tensor(v):
                    dst[key].copy_(v)

    order = ("global_orient", "body_pose", "betas", "pred_cam")
    eager = []
    for k in range(3):
        load(k)
        losses, grads = vl.value_and_grad(batch, output, body_model=m, focal_length=F, image_size=S)
        torch.cuda.synchronize()
        eager.append((torch.stack([losses[n] for n in LOSS_KEYS]).clone(), [grads[n].clone() for n in order]))
    assert not torch.equal(eager[1][1][3], eager[2][1][3])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        losses, grads = vl.value_and_grad(batch, output, body_model=m, focal_length=F, image_size=S)
    for k in (1, 2):
        load(k)
        for n in order:
            grads[n].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(torch.stack([losses[n] for n in LOSS_KEYS]), eager[k][0]), k
        for n, e in zip(order, eager[k][1]):
            assert torch.equal(grads[n], e), (k, n)
    del graph


# ------------------------------------------------------------------------------------------------ the C call: guard bands, refusals
def _c_call(lib, ins, slots, mode, gt, B, cam=True, desc_kw=None, in_kw=None, focal=F, size=S, desc_null=False, in_null=False, table_null=False):
    d = dict(pelvis_id=39, mode=_cabi.VAL_LOSS_LOOSE if mode == "loose" else _cabi.VAL_LOSS_PLAIN, gt_pose_is_rotmat=0 if gt == "aa" else 1)
    d.update(desc_kw or {})
    desc = _cabi.ValLossDesc(*WEIGHTS, GV.LOOSE_WEIGHT, d["pelvis_id"], d["mode"], d["gt_pose_is_rotmat"], 0)
    fields = dict(zip(_cabi.VAL_LOSS_IN_FIELDS, IN_KEYS + ("valid_3d", "kp2d_thresh", "angle_thresh")))
    ptrs = {f: ins[k].data_ptr() if (mode == "loose" or f not in ("valid_3d", "kp2d_thresh", "angle_thresh")) else None for f, k in fields.items()}
    ptrs.update(in_kw or {})
    cin = _cabi.ValLossIn(**ptrs)
    table = (C.c_void_p * _cabi.LOSS_GRAD_SLOTS)(*[slots[k].data_ptr() if slots.get(k) is not None else None for k in GO.SLOTS])
    rc = lib.thmr_val_loss_grad(None if desc_null else C.byref(desc), None if in_null else C.byref(cin), _p(ins["pred_cam"]) if cam else None,
                                focal, size, B, None if table_null else table, None)
    return rc, (lib.thmr_last_error(None) or b"").decode()


@pytest.mark.parametrize("mode", ["plain", "loose"])
@pytest.mark.parametrize("B", [1, 5])
def test_guard_bands(built_lib, cuda_dev, B, mode):
    """Every input and every slot is a window of a canary buffer: nothing outside a window is written, no input changes, every output
    element is written, and the outputs equal the plain call's bit for bit."""
    plain_in = _device_inputs(_inputs(B, 39), cuda_dev, "aa")
    want = _grad(plain_in, mode)
    ins, checks = {}, []
    for k, v in plain_in.items():
        ins[k], chk = G.guarded_like(tuple(v.shape), device=cuda_dev, fill=v)
        checks.append((k, chk))
    slots = {}
    for k in GO.SLOTS:
        slots[k], chk = G.guarded_like((B,) + SHAPES[k], device=cuda_dev)
        checks.append((k, chk))
    rc, msg = _c_call(built_lib, ins, slots, mode, "aa", B)
    assert rc == 0, msg
    torch.cuda.synchronize()
    for k, chk in checks:
        try:
            chk()
        except AssertionError as e:
            raise AssertionError(f"{k}: {e}") from None
    for k, v in plain_in.items():
        assert torch.equal(ins[k].view(torch.int32), v.view(torch.int32)), f"input {k} was written"
    for k in GO.SLOTS:
        assert not bool(G.holds_canary(slots[k]).any()), f"{k}: an element was never written"
        assert torch.equal(slots[k], want[k]), k


def test_refusals(built_lib, cuda_dev):
    """Everything the header lists: THMR_ERR_INVALID with a message, before any launch — the outputs stay as they were."""
    B = 5
    ins = _device_inputs(_inputs(B, 39), cuda_dev, "aa")
    slots = {k: torch.full((B,) + SHAPES[k], -3.0, device=cuda_dev) for k in GO.SLOTS}
    call = functools.partial(_c_call, built_lib, ins, slots, "loose", "aa")
    inf, nan = float("inf"), float("nan")
    cases = [dict(desc_null=True), dict(in_null=True), dict(table_null=True), dict(B=0), dict(B=-1), dict(B=2 ** 24 + 1), dict(B=2 ** 31 - 1),
             dict(desc_kw={"mode": 2}), dict(desc_kw={"mode": -1}), dict(desc_kw={"pelvis_id": 44}), dict(desc_kw={"pelvis_id": -1}),
             dict(desc_kw={"gt_pose_is_rotmat": 2}), dict(in_kw={"valid_3d": None}), dict(in_kw={"kp2d_thresh": None}),
             dict(in_kw={"angle_thresh": None}), dict(in_kw={"gt_keypoints_3d": ins["gt_keypoints_3d"].data_ptr() + 4}),
             dict(in_kw={"pred_keypoints_2d": ins["pred_keypoints_2d"].data_ptr() + 4}),
             dict(focal=0.0), dict(focal=-1.0), dict(focal=inf), dict(focal=nan), dict(size=0.0), dict(size=-256.0), dict(size=inf), dict(size=nan)]
    cases += [dict(in_kw={f: None}) for f in _cabi.VAL_LOSS_IN_FIELDS[:11]]
    for kw in cases:
        kw = dict(kw)
        rc, msg = call(kw.pop("B", B), **kw)
        assert rc == _cabi.ERR_INVALID and "val_loss_grad" in msg, (kw, rc, msg)
    # the three it adds
    empty = {k: None for k in GO.SLOTS}
    rc, msg = _c_call(built_lib, ins, empty, "loose", "aa", B)
    assert rc == _cabi.ERR_INVALID and "every slot" in msg, (rc, msg)
    for k in ("joints", "cam"):
        rc, msg = _c_call(built_lib, ins, {k: slots[k]}, "loose", "aa", B, cam=False)
        assert rc == _cabi.ERR_INVALID and "pred_cam" in msg, (k, rc, msg)
    torch.cuda.synchronize()
    for k in GO.SLOTS:
        assert (slots[k] == -3.0).all(), f"a refused call wrote {k}"
    # without pred_cam the projection's scalars are not read; the plain mode needs neither thresholds nor valid_3d
    direct = {k: slots[k] for k in ("kp2d", "kp3d", "rotmat", "betas")}
    rc, msg = _c_call(built_lib, ins, direct, "plain", "aa", B, cam=False, focal=nan, size=-1.0)
    assert rc == 0, msg
    torch.cuda.synchronize()
    want = _grad(ins, "plain", cam=False)
    for k in direct:
        assert torch.equal(slots[k], want[k]), k
    assert (slots["joints"] == -3.0).all() and (slots["cam"] == -3.0).all()
    with pytest.raises(ValueError, match="loose"):
        ops.val_loss_grad(*[ins[k] for k in IN_KEYS], WEIGHTS, loose=True)
