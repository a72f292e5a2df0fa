"""The forward value of the reference's loss on the device: TokenHMR.compute_loss (tokenhmr/lib/models/tokenhmr.py:190-277)
as validation_step (:421-440) runs it, and TokenLoss (losses.py:230-252).

    vloss = ValidationLoss(cfg)                        # cfg.LOSS_WEIGHTS, cfg.MODEL.LOOSE_SUP, cfg.MODEL.LOOSE_WEIGHT
    loss = vloss(batch, output)                        # a 0-dim device tensor; output['losses'] holds the reference's six keys
    means = vloss.get_metrics_dict()                   # the one synchronisation: the mean of every term over the batches so far

One call enqueues the two launches of `thmr_val_loss` (plus one concatenation of the ground-truth pose) and leaves every result on the
device.  The loss is the number the reference selects checkpoints by (best_validation_loss, :101).  Its gradient is built as far as the
head's outputs:

    losses, grads = vloss.value_and_grad(batch, output, body_model=smpl_model)      # d loss / d (global_orient, body_pose, betas, pred_cam)

With a tokenhmr_amd.discriminator.Discriminator the generator's adversarial term (tokenhmr.py:392-394) joins both:

    losses, grads = vloss.value_and_grad(batch, output, body_model=smpl_model, discriminator=D)      # + losses['loss_gen']

There is no backward above the head, no gradient by the discriminator's own weights, and the optimisers are not built.

Deliberate departure: the reference's LOOSE_SUP branch writes into the batch (keypoints_2d[:, :, -1], keypoints_3d[:, :, -1],
has_smpl_params['betas']; :223, :227, :240).  Nothing in `batch` is modified here; what the reference would have written is returned in
output['loss_masks'] as conf2d_used, conf3d_used and has_betas_used.

The per-joint thresholds of the LOOSE_SUP branch (losses.py:7-20) are an INPUT, `thresholds`: a mapping with 'kp2d' (44), 'body_pose' (23)
and 'global_orient' (1), or the path of an .npz with those keys.  None are shipped.
"""
import os

import numpy as np
import torch

from . import ops

LOSS_KEYS = ("loss", "loss_keypoints_2d", "loss_keypoints_3d", "loss_global_orient", "loss_body_pose", "loss_betas")
_WEIGHT_KEYS = ("KEYPOINTS_2D", "KEYPOINTS_3D", "GLOBAL_ORIENT", "BODY_POSE", "BETAS")
_THRESH_SHAPES = {"kp2d": 44, "body_pose": 23, "global_orient": 1}


def _node(cfg, key):
    """cfg.KEY or cfg['KEY'] (yacs CfgNode, ConfigNode, dict, namespace)."""
    if isinstance(cfg, dict):
        if key in cfg:
            return cfg[key]
    elif hasattr(cfg, key):
        return getattr(cfg, key)
    raise KeyError(f"the config has no {key}")


def load_thresholds(thresholds):
    """-> {'kp2d': (44) float32, 'angle': (24) float32, [0] = global_orient}, validated."""
    if isinstance(thresholds, (str, os.PathLike)):
        with np.load(thresholds) as f:
            thresholds = {k: f[k] for k in f.files}
    out = {}
    for k, n in _THRESH_SHAPES.items():
        if k not in thresholds:
            raise ValueError(f"thresholds lacks '{k}' ({n} values)")
        v = torch.as_tensor(np.asarray(thresholds[k], dtype=np.float32)).reshape(-1)
        if v.numel() != n:
            raise ValueError(f"thresholds['{k}'] holds {v.numel()} values, {n} are expected")
        out[k] = v
    return {"kp2d": out["kp2d"].contiguous(), "angle": torch.cat([out["global_orient"], out["body_pose"]]).contiguous()}


class ValidationLoss:
    def __init__(self, cfg, thresholds=None, trusted_3d_datasets=("H36M-TRAIN-WMASK", "BEDLAM"), pelvis_id=25 + 14, strict_flags=False):
        """strict_flags: also read `smpl_params_is_axis_angle` flags that live on the device (one synchronisation per call); by default
        only host-resident flags are checked and the pose tensor's shape decides."""
        lw = _node(cfg, "LOSS_WEIGHTS")
        missing = [k for k in _WEIGHT_KEYS if k not in lw]
        if missing:
            raise KeyError(f"cfg.LOSS_WEIGHTS lacks {missing}")
        self.weights = [float(lw[k]) for k in _WEIGHT_KEYS]
        self.adversarial_weight = float(lw["ADVERSARIAL"]) if "ADVERSARIAL" in lw else 0.0      # tokenhmr.py:394; read by value_and_grad only
        model = _node(cfg, "MODEL")
        get = model.get if hasattr(model, "get") else (lambda k, d=None: getattr(model, k, d))
        self.loose_sup = bool(get("LOOSE_SUP", False))
        self.loose_weight = float(get("LOOSE_WEIGHT", 0.0) or 0.0)
        self.thresholds = load_thresholds(thresholds) if thresholds is not None else None
        self.trusted_3d_datasets = tuple(trusted_3d_datasets)
        self.pelvis_id = int(pelvis_id)
        self.strict_flags = bool(strict_flags)
        self._dev = {}                      # device -> (kp2d_thresh, angle_thresh, running, workspace)
        self._grad = {}                     # (device, B) -> the buffers of value_and_grad

    # ---- argument handling: everything up to the launch, on whatever device the tensors live ----
    def prepare(self, batch, output, train=False):
        """The launch's arguments from the reference's dicts -> a dict (tensors float32 and contiguous, on the inputs' device)."""
        loose = bool(self.loose_sup and train)                          # tokenhmr.py:214
        if loose and self.thresholds is None:
            raise ValueError("MODEL.LOOSE_SUP with train=True needs the per-joint thresholds: pass `thresholds` to ValidationLoss "
                             "(a mapping with 'kp2d', 'body_pose', 'global_orient', or the path of an .npz)")
        pred = output["pred_smpl_params"]
        kp2 = output["pred_keypoints_2d"]
        dev, B = kp2.device, kp2.shape[0]
        f = lambda t: t.to(dev).float().contiguous()      # noqa: E731
        gt, has, flags = batch["smpl_params"], batch["has_smpl_params"], batch["smpl_params_is_axis_angle"]
        is_aa = {}
        for k, n in (("global_orient", 1), ("body_pose", 23)):
            numel = gt[k].numel() // B
            if numel not in (3 * n, 9 * n):
                raise ValueError(f"batch['smpl_params']['{k}'] holds {numel} values per item: {3 * n} (axis-angle) or {9 * n} (matrices)")
            is_aa[k] = numel == 3 * n
            fl = flags[k]
            # the flag is checked where that costs no synchronisation (host values); a device tensor is read back only under
            # strict_flags: otherwise the shape decides
            if self.strict_flags or not (torch.is_tensor(fl) and fl.is_cuda):
                fl = torch.as_tensor(fl).reshape(-1).bool().cpu()
                if fl.any() and not fl.all():
                    raise ValueError(f"batch['smpl_params_is_axis_angle']['{k}'] mixes axis-angle and matrix items in one batch "
                                     "(the reference's .all() would silently take the matrix branch)")
                if bool(fl.all()) != is_aa[k]:
                    raise ValueError(f"batch['smpl_params_is_axis_angle']['{k}'] says {'axis-angle' if fl.all() else 'matrices'}, "
                                     f"the tensor holds {numel} values per item")
        if is_aa["global_orient"] != is_aa["body_pose"]:
            raise ValueError("batch['smpl_params']: 'global_orient' and 'body_pose' must both be axis-angle or both be matrices")
        gt_pose = torch.cat([f(gt["global_orient"]).reshape(B, -1), f(gt["body_pose"]).reshape(B, -1)], 1)
        gt_pose = gt_pose if is_aa["body_pose"] else gt_pose.view(B, 24, 3, 3)
        a = {
            "pred_kp2d": f(kp2).reshape(B, 44, 2), "pred_kp3d": f(output["pred_keypoints_3d"]).reshape(B, 44, 3),
            "pred_rotmat": _joined_rotmat(pred["global_orient"], pred["body_pose"], B), "pred_betas": f(pred["betas"]).reshape(B, 10),
            "gt_kp2d": f(batch["keypoints_2d"]), "gt_kp3d": f(batch["keypoints_3d"]), "gt_pose": gt_pose, "gt_betas": f(gt["betas"]).reshape(B, 10),
            "has_global_orient": f(has["global_orient"]).reshape(B), "has_body_pose": f(has["body_pose"]).reshape(B),
            "has_betas": f(has["betas"]).reshape(B), "loose": loose, "valid_3d": None,
        }
        if loose:                                                       # :226
            names = batch["dataset"]
            if len(names) != B:
                raise ValueError(f"batch['dataset'] names {len(names)} items, the batch holds {B}")
            a["valid_3d"] = torch.tensor([float(n in self.trusted_3d_datasets) for n in names], dtype=torch.float32).to(dev)
        return a

    def _device_state(self, dev, B):
        st = self._dev.get(dev)
        if st is None:
            th = self.thresholds
            st = self._dev[dev] = {"kp2d": th["kp2d"].to(dev) if th else None, "angle": th["angle"].to(dev) if th else None,
                                   "running": torch.zeros(7, device=dev, dtype=torch.float64), "ws": None}
        if st["ws"] is None or st["ws"].numel() < 5 * B:
            st["ws"] = torch.empty(5 * max(B, 64), device=dev, dtype=torch.float32)
        return st

    def _value(self, a, loose, output, running, losses=None, out=None):
        """The thmr_val_loss call of prepare()'s arguments; sets output['losses'], 'loss_per_item' and (loose) 'loss_masks'."""
        st = self._device_state(a["pred_kp2d"].device, a["pred_kp2d"].shape[0])
        res = ops.val_loss(a["pred_kp2d"], a["pred_kp3d"], a["pred_rotmat"], a["pred_betas"], a["gt_kp2d"], a["gt_kp3d"], a["gt_pose"],
                           a["gt_betas"], a["has_global_orient"], a["has_body_pose"], a["has_betas"], self.weights, loose=loose,
                           loose_weight=self.loose_weight, valid_3d=a["valid_3d"], kp2d_thresh=st["kp2d"] if loose else None,
                           angle_thresh=st["angle"] if loose else None, pelvis_id=self.pelvis_id, taps=True,
                           running=st["running"] if running else None, workspace=st["ws"], losses=losses, out=out)
        losses = res.pop("losses")
        output["losses"] = {k: losses[i] for i, k in enumerate(LOSS_KEYS)}       # tokenhmr.py:268-275
        output["loss_per_item"] = res.pop("per_item")
        if loose:
            output["loss_masks"] = res
        return output["losses"]

    def __call__(self, batch, output, train=False):
        a = self.prepare(batch, output, train)
        loose = a.pop("loose")
        return self._value(a, loose, output, running=True)["loss"]      # a fresh buffer per call: earlier batches' values stay valid

    # ---- value and gradient ----
    def _grad_buffers(self, dev, B, loose):
        """The buffers of one (device, batch size): the value's outputs, the six slots, the body model's gradients and the two sums."""
        f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)      # noqa: E731
        b = self._grad.get((dev, B))
        if b is None:
            b = self._grad[(dev, B)] = dict(losses=f(6), value={"per_item": f(B, 5)}, kp2d=f(B, 44, 2), kp3d=f(B, 44, 3), joints=f(B, 44, 3),
                                            cam=f(B, 3), rotmat=f(B, 24, 3, 3), betas=f(B, 10), bm_rotmat=f(B, 24, 3, 3), bm_betas=f(B, 10),
                                            total_rotmat=f(B, 24, 3, 3), total_betas=f(B, 10))
        if loose and "valid2d" not in b["value"]:          # the loose branch's taps, on its first call at this size
            b["value"].update({k: f(B) if k == "has_betas_used" else f(B, 44 if "2d" in k or "3d" in k else 24) for k in ops.VAL_LOSS_TAPS})
        return b

    def value_and_grad(self, batch, output, body_model=None, train=False, focal_length=5000.0, image_size=256.0, discriminator=None,
                       adversarial_weight=None):
        """-> (losses, grads).  `losses` is what __call__ sets as output['losses'], from the same thmr_val_loss call on the same arguments
        (bit-equal to it); the running means of get_metrics_dict() count __call__ only.  The total is a SUM over the items, as the
        reference's: nothing is divided by the batch size.
        Without body_model, grads holds the plain partial derivatives by the five tensors compute_loss reads: 'pred_keypoints_2d'
        (B,44,2), 'pred_keypoints_3d' (B,44,3), 'global_orient' (B,1,3,3), 'body_pose' (B,23,3,3), 'betas' (B,10).
        With a tokenhmr_amd.smpl.SMPL and output['pred_cam'], grads holds the total derivative by the head's outputs, through the projection
        (focal_length = EXTRA.FOCAL_LENGTH, image_size = MODEL.IMAGE_SIZE) and the body model: 'global_orient', 'body_pose', 'betas' and
        'pred_cam' (B,3).  The chain: thmr_val_loss_grad, thmr_smpl_backward on its JOINTS slot in chunks of body_model.max_batch, one
        torch.add per summed tensor; on the current stream, without synchronisation, and after the first call at a batch size without
        allocations beyond prepare()'s own copies (capturable once body_model.enable_grad() has run; prepare() uploads valid_3d from
        the host in the loose branch, which a capture refuses).  The returned tensors are buffers of this object, overwritten by the
        next call at that batch size on that device.
        discriminator (a tokenhmr_amd.discriminator.Discriminator; default None: not a launch or a bit changes): the generator's term of
        training_step (tokenhmr.py:392-394).  `losses` then also holds 'loss_gen' = ((D(body_pose, betas) - 1)^2).sum() / B, 'loss' is
        compute_loss + w loss_gen, and w d loss_gen is added into the 'body_pose' and 'betas' gradients ('global_orient' and 'pred_cam'
        get none); w = adversarial_weight, by default cfg.LOSS_WEIGHTS.ADVERSARIAL where the config has it, else 0.  One
        thmr_disc_backward call per chunk of the discriminator's max_batch, on body_pose as the stride-216 view of the joined
        rotation matrices (no copy), and three torch.add."""
        a = self.prepare(batch, output, train)
        loose = a.pop("loose")
        dev, B = a["pred_kp2d"].device, a["pred_kp2d"].shape[0]
        b = self._grad_buffers(dev, B, loose)
        losses = self._value(a, loose, output, running=False, losses=b["losses"], out=b["value"])
        st = self._device_state(dev, B)
        cam = None
        if body_model is not None:
            if output.get("pred_cam") is None:
                raise ValueError("value_and_grad with a body model differentiates through the projection: output['pred_cam'] is needed")
            if body_model.device != dev:
                raise ValueError(f"the body model lives on {body_model.device}, the loss's inputs on {dev}")
            cam = output["pred_cam"].detach().to(dev).float().reshape(B, 3).contiguous()
            body_model.enable_grad()
        want = ("joints", "cam", "rotmat", "betas") if body_model is not None else ("kp2d", "kp3d", "rotmat", "betas")
        ops.val_loss_grad(a["pred_kp2d"], a["pred_kp3d"], a["pred_rotmat"], a["pred_betas"], a["gt_kp2d"], a["gt_kp3d"], a["gt_pose"],
                          a["gt_betas"], a["has_global_orient"], a["has_body_pose"], a["has_betas"], self.weights, loose=loose,
                          loose_weight=self.loose_weight, valid_3d=a["valid_3d"], kp2d_thresh=st["kp2d"] if loose else None,
                          angle_thresh=st["angle"] if loose else None, pelvis_id=self.pelvis_id, pred_cam=cam, focal_length=focal_length,
                          image_size=image_size, want=want, out=b)
        if discriminator is not None:
            losses = self._adversarial(discriminator, adversarial_weight, a, b, losses, output)
        if body_model is None:
            if discriminator is not None:
                b["rotmat"][:, 1:].add_(b["adv_poses"], alpha=b["adv_w"])
                b["betas"].add_(b["adv_betas"], alpha=b["adv_w"])
            return losses, {"pred_keypoints_2d": b["kp2d"], "pred_keypoints_3d": b["kp3d"], "global_orient": b["rotmat"][:, :1],
                            "body_pose": b["rotmat"][:, 1:], "betas": b["betas"]}
        with torch.no_grad():
            for i in range(0, B, body_model.max_batch):
                n = min(body_model.max_batch, B - i)
                body_model._backward(a["pred_rotmat"][i:i + n], False, a["pred_betas"][i:i + n], n, None, b["joints"][i:i + n],
                                     b["bm_rotmat"][i:i + n], b["bm_betas"][i:i + n])
            torch.add(b["bm_rotmat"], b["rotmat"], out=b["total_rotmat"])
            torch.add(b["bm_betas"], b["betas"], out=b["total_betas"])
            if discriminator is not None:
                b["total_rotmat"][:, 1:].add_(b["adv_poses"], alpha=b["adv_w"])
                b["total_betas"].add_(b["adv_betas"], alpha=b["adv_w"])
        return losses, {"global_orient": b["total_rotmat"][:, :1], "body_pose": b["total_rotmat"][:, 1:], "betas": b["total_betas"],
                        "pred_cam": b["cam"]}

    def _adversarial(self, discriminator, weight, a, b, losses, output):
        """loss_gen and its gradient by body_pose and betas into b['adv_*']; -> the losses dict with 'loss_gen' and the new total."""
        dev, B = a["pred_betas"].device, a["pred_betas"].shape[0]
        if discriminator.device != dev:
            raise ValueError(f"the discriminator lives on {discriminator.device}, the loss's inputs on {dev}")
        w = self.adversarial_weight if weight is None else float(weight)
        if "adv_poses" not in b:
            f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)      # noqa: E731
            b.update(adv_poses=f(B, 23, 3, 3), adv_betas=f(B, 10), adv_loss=f(()), adv_chunk=f(()), adv_total=f(()))
        b["adv_w"] = w
        with torch.no_grad():
            discriminator._chunks(a["pred_rotmat"][:, 1:], a["pred_betas"], target=1.0, want_loss=True, want_poses=True, want_betas=True,
                                  bufs={"loss": b["adv_loss"], "chunk_loss": b["adv_chunk"], "grad_poses": b["adv_poses"],
                                        "grad_betas": b["adv_betas"]})
            torch.add(losses["loss"], b["adv_loss"], alpha=w, out=b["adv_total"])          # tokenhmr.py:394
        losses = dict(losses, loss=b["adv_total"], loss_gen=b["adv_loss"])
        output["losses"] = losses
        return losses

    def reset(self):
        for st in self._dev.values():
            st["running"].zero_()

    def get_metrics_dict(self):
        """The mean over the batches seen since reset() of each of the six terms — what averaging validation_step_outputs gives.
        Synchronises once."""
        tot = None
        for st in self._dev.values():
            r = st["running"].cpu()
            tot = r if tot is None else tot + r
        if tot is None or float(tot[6]) == 0.0:
            raise ValueError("no batch was evaluated")
        return {k: float(tot[i] / tot[6]) for i, k in enumerate(LOSS_KEYS)}


def _joined_rotmat(go, bp, B):
    """global_orient (B,1,3,3) + body_pose (B,23,3,3) -> (B,24,3,3) contiguous; no copy when they are the two views of one (B,24,3,3)
    buffer the facade hands out."""
    go, bp = go.reshape(B, 1, 3, 3), bp.reshape(B, 23, 3, 3)
    if (go.dtype == torch.float32 and bp.dtype == torch.float32 and go.device == bp.device and go.stride() == (216, 9, 3, 1)
            and bp.stride() == (216, 9, 3, 1) and bp.data_ptr() == go.data_ptr() + 36
            and go.untyped_storage().data_ptr() == bp.untyped_storage().data_ptr()
            and (go.storage_offset() + B * 216) * 4 <= go.untyped_storage().nbytes()):
        return go.as_strided((B, 24, 3, 3), (216, 9, 3, 1))
    return torch.cat([go.float(), bp.to(go.device).float()], 1).contiguous()


def token_loss(probs, gt_tokens):
    """TokenLoss.forward (losses.py:239-252): probs (B, 160, 2048) — the reference passes cls_logits_softmax — and gt_tokens (B, 160)
    -> the mean cross-entropy as a 0-dim device tensor."""
    x = probs.float().reshape(-1, probs.shape[-1]).contiguous()
    return ops.token_ce(x, gt_tokens.to(x.device).reshape(-1).to(torch.int32).contiguous())
