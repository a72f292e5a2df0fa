"""The HMR pose and shape discriminator on the device: the reference's Discriminator
(tokenhmr/lib/models/discriminator.py:4-99) and the adversarial terms tokenhmr.py builds on it.

    D = Discriminator(device="cuda:0").load_state_dict(sd)           # the reference's key names; or Discriminator.from_checkpoint(path)
    out = D(body_pose, betas)                                        # (B,25); differentiable by both inputs under torch autograd
    loss_adv = D.adversarial_loss(body_pose, betas)                  # tokenhmr.py:392-394, ((D(.) - 1)^2).sum() / B
    loss_disc = D.discriminator_loss(body_pose, betas, gt_aa, gt_betas)      # :357-362, loss_fake + loss_real
    out, loss, g_pose, g_betas = D.value_and_grad(body_pose, betas, target=1.0)      # one thmr_disc_backward call per chunk

The C side is stateless (thmr_disc_forward / thmr_disc_backward, csrc/discriminator.hip): this object holds the weight block that
pack_weights() lays out — once, at load — and the workspaces.  There is no gradient by the discriminator's own weights and no optimiser;
every tensor stays on the device and no call synchronises.  Batches above max_batch (THMR_DISC_MAX_BATCH) are served in chunks."""
import ctypes as C

import torch

from . import _cabi
from .weights import discriminator_spec

N_JOINTS, N_OUT = 23, 25


def _up(x):
    return (x + 63) & ~63


def weight_layout():
    """[(block name, float offset, shape)] of the device weight block, in the order include/tokenhmr_hip.h lists; every block starts
    at a multiple of 64 floats.  The last offset + size, rounded up, is THMR_DISC_WEIGHT_FLOATS."""
    blocks = [("conv1_t", (9, 32)), ("conv1_b", (32,)), ("conv2_t", (32, 32)), ("conv2", (32, 32)), ("conv2_b", (32,)), ("conv1", (32, 9)),
              ("pose_out_w", (23, 32)), ("pose_out_b", (23,)), ("betas_fc1_w", (10, 10)), ("betas_fc1_b", (10,)), ("betas_fc2_w", (5, 10)),
              ("betas_fc2_b", (5,)), ("betas_out_w", (5,)), ("betas_out_b", (1,)), ("fc1", (1024, _cabi.DISC_KPAD)), ("fc1_b", (1024,)),
              ("fc1_t", (736, 1024)), ("fc2", (1024, 1024)), ("fc2_b", (1024,)), ("fc2_t", (1024, 1024)), ("out_w", (1024,)), ("out_b", (1,))]
    out, off = [], 0
    for name, shape in blocks:
        out.append((name, off, shape))
        n = 1
        for s in shape:
            n *= s
        off = _up(off + n)
    assert off == _cabi.DISC_WEIGHT_FLOATS, (off, _cabi.DISC_WEIGHT_FLOATS)
    return out


def check_state_dict(sd, prefix=""):
    """{name without prefix: float32 CPU tensor} of exactly the reference's keys under `prefix`, shapes checked: a missing, an unexpected
    or a mis-shaped tensor raises, as load_state_dict(strict=True) does."""
    spec = dict(discriminator_spec())
    have = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    missing, unexpected = [k for k in spec if k not in have], [k for k in have if k not in spec]
    if missing or unexpected:
        raise KeyError(f"Discriminator.load_state_dict: missing {missing[:6]}{' ...' if len(missing) > 6 else ''}, "
                       f"unexpected {[prefix + k for k in unexpected[:6]]}{' ...' if len(unexpected) > 6 else ''}")
    out = {}
    for k, shape in spec.items():
        if tuple(have[k].shape) != shape:
            raise ValueError(f"Discriminator.load_state_dict: '{prefix + k}' is {tuple(have[k].shape)}, expected {shape}")
        out[k] = have[k].detach().to("cpu", torch.float32)
    return out


def pack_weights(sd, prefix=""):
    """The reference's state_dict -> the float32 CPU block of THMR_DISC_WEIGHT_FLOATS floats (weight_layout()).  The 4-D conv weights are
    taken as they are.  fc1's columns are permuted from the reference's channel-major flatten (c * 23 + j, discriminator.py:91) to
    j * 32 + c, the order the front kernel writes, and padded with zero columns to K = 768."""
    s = check_state_dict(sd, prefix)
    c1, c2 = s["D_conv1.weight"].reshape(32, 9), s["D_conv2.weight"].reshape(32, 32)
    fc1 = torch.zeros(1024, _cabi.DISC_KPAD)
    fc1[:, :736] = s["D_alljoints_fc1.weight"].reshape(1024, 32, N_JOINTS).permute(0, 2, 1).reshape(1024, 736)
    fc2 = s["D_alljoints_fc2.weight"]
    t = {"conv1_t": c1.t(), "conv1_b": s["D_conv1.bias"], "conv2_t": c2.t(), "conv2": c2, "conv2_b": s["D_conv2.bias"], "conv1": c1,
         "pose_out_w": torch.cat([s[f"pose_out.{j}.weight"] for j in range(N_JOINTS)], 0),
         "pose_out_b": torch.cat([s[f"pose_out.{j}.bias"] for j in range(N_JOINTS)], 0),
         "betas_fc1_w": s["betas_fc1.weight"], "betas_fc1_b": s["betas_fc1.bias"], "betas_fc2_w": s["betas_fc2.weight"],
         "betas_fc2_b": s["betas_fc2.bias"], "betas_out_w": s["betas_out.weight"].reshape(5), "betas_out_b": s["betas_out.bias"],
         "fc1": fc1, "fc1_b": s["D_alljoints_fc1.bias"], "fc1_t": fc1[:, :736].t(), "fc2": fc2, "fc2_b": s["D_alljoints_fc2.bias"],
         "fc2_t": fc2.t(), "out_w": s["D_alljoints_out.weight"].reshape(1024), "out_b": s["D_alljoints_out.bias"]}
    block = torch.zeros(_cabi.DISC_WEIGHT_FLOATS, dtype=torch.float32)
    for name, off, shape in weight_layout():
        v = t[name].contiguous().reshape(-1)
        assert tuple(t[name].shape) == shape, (name, tuple(t[name].shape), shape)
        block[off:off + v.numel()] = v
    return block


class _DiscFn(torch.autograd.Function):
    """Discriminator.__call__ with a graph: forward = thmr_disc_forward (the launches and bits of the plain path), backward =
    thmr_disc_backward with the incoming gradient as grad_out.  Once differentiable."""

    @staticmethod
    def forward(ctx, model, poses, betas):
        ctx.model = model
        ctx.save_for_backward(poses, betas)
        return model._chunks(poses, betas, want_out=True)[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        poses, betas = ctx.saved_tensors
        m = ctx.model
        g_out = g_out.to(m.device, torch.float32).contiguous()
        _, _, gp, gb = m._chunks(poses, betas, grad_out=g_out, want_poses=ctx.needs_input_grad[1], want_betas=ctx.needs_input_grad[2])
        return None, None if gp is None else gp.reshape(poses.shape), None if gb is None else gb.reshape(betas.shape)


class _LossFn(torch.autograd.Function):
    """L(target) with a graph: the value and the gradients come out of one thmr_disc_backward call per chunk in forward()."""

    @staticmethod
    def forward(ctx, model, target, poses, betas):
        ctx.set_materialize_grads(False)
        _, loss, gp, gb = model._chunks(poses, betas, target=target, want_loss=True, want_poses=ctx.needs_input_grad[2],
                                        want_betas=ctx.needs_input_grad[3])
        keep = [None if g is None else g.reshape(t.shape) for g, t in ((gp, poses), (gb, betas))]
        ctx.which = [g is not None for g in keep]
        ctx.save_for_backward(*[g for g in keep if g is not None])
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_total):
        saved = iter(ctx.saved_tensors)
        grads = [next(saved) if have else None for have in ctx.which]
        if g_total is None:
            return None, None, None, None
        return (None, None) + tuple(None if g is None else g * g_total for g in grads)


class Discriminator:
    max_batch = _cabi.DISC_MAX_BATCH

    def __init__(self, device="cuda:0"):
        self.device = _cabi.Handle.cuda_device(device, "tokenhmr_amd.discriminator.Discriminator runs on a HIP device only", resolve=True)
        self.lib = _cabi.load()
        self.weights = None
        self._ws = None

    # ---- weights ----
    def load_state_dict(self, sd, prefix=""):
        """The reference's Discriminator.state_dict() (keys 'D_conv1.weight' ... 'pose_out.22.bias' ... 'D_alljoints_out.bias' under
        `prefix`); strict: a missing or an unexpected key under the prefix raises KeyError, a wrong shape ValueError."""
        self.weights = pack_weights(sd, prefix).to(self.device)
        return self

    @staticmethod
    def state_from_checkpoint(path, strict=True):
        """The 'discriminator.*' tensors of a reference Lightning checkpoint (tokenhmr.py:58: self.discriminator), read through ckpt_io
        (host only).  strict=False skips, with a warning, tensors under 'discriminator.' that the module does not have."""
        from . import ckpt_io
        full = ckpt_io.load_checkpoint(path)
        full = full.get("state_dict", full)
        known = {"discriminator." + k for k, _ in discriminator_spec()}
        sd = ckpt_io.select_state(full, ("discriminator.",), known, strict=strict, what="discriminator checkpoint")
        if not sd:
            raise KeyError(f"{path} holds no 'discriminator.*' tensor of the reference's Discriminator")
        return sd

    @classmethod
    def from_checkpoint(cls, path, device="cuda:0", strict=True):
        """state_from_checkpoint(path) loaded into a Discriminator on `device`."""
        return cls(device).load_state_dict(cls.state_from_checkpoint(path, strict), prefix="discriminator.")

    # ---- the C calls ----
    def _workspace(self, B):
        need = _cabi.DISC_WS_PER_ITEM * B
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(_cabi.DISC_WS_PER_ITEM * max(B, 64), device=self.device, dtype=torch.float32)
        return self._ws

    def _inputs(self, poses, betas):
        """-> (poses (B,23,3,3) float32 on the device whose items are contiguous, its item stride in floats, betas (B,10) contiguous).
        The body_pose view of a (B,24,3,3) buffer (stride 216) is taken as it is."""
        if self.weights is None:
            raise RuntimeError("Discriminator: load_state_dict() first")
        betas = betas.detach().to(self.device, torch.float32)
        B = betas.shape[0] if betas.dim() > 1 else 1
        betas = betas.reshape(B, 10).contiguous()
        poses = poses.detach().to(self.device, torch.float32)
        if poses.numel() != B * 207:
            raise ValueError(f"Discriminator: poses holds {poses.numel()} values for {B} items, (B,23,3,3) is expected")
        if not (poses.dim() == 4 and tuple(poses.shape) == (B, N_JOINTS, 3, 3) and poses.stride()[1:] == (9, 3, 1)
                and (B == 1 or poses.stride(0) >= 207)):
            poses = poses.reshape(B, N_JOINTS, 3, 3).contiguous()
        return poses, (poses.stride(0) if B > 1 else 207), betas, B

    def _table(self, out=None, loss=None, grad_poses=None, grad_betas=None, ws=None):
        return (C.c_void_p * _cabi.DISC_SLOTS)(*[None if t is None else t.data_ptr() for t in (out, loss, grad_poses, grad_betas, ws)])

    def forward_raw(self, poses, stride, betas, B, out, loss=None, target=0.0, loss_div=0, workspace=None):
        """thmr_disc_forward on prepared arguments (see _inputs); writes `out` (B,25) and, when given, `loss` (one float)."""
        ws = workspace if workspace is not None else self._workspace(B)
        with torch.cuda.device(self.device):
            rc = self.lib.thmr_disc_forward(self.weights.data_ptr(), poses.data_ptr(), stride, betas.data_ptr(), B, loss_div, float(target),
                                            self._table(out=out, loss=loss, ws=ws), torch.cuda.current_stream(self.device).cuda_stream)
        _cabi.check(rc, None, self.lib)

    def backward_raw(self, poses, stride, betas, B, grad_out=None, target=1.0, loss_div=0, out=None, loss=None, grad_poses=None,
                     grad_betas=None, workspace=None):
        """thmr_disc_backward on prepared arguments: the gradient of sum(out * grad_out), or of L(target) without grad_out."""
        ws = workspace if workspace is not None else self._workspace(B)
        with torch.cuda.device(self.device):
            rc = self.lib.thmr_disc_backward(self.weights.data_ptr(), poses.data_ptr(), stride, betas.data_ptr(),
                                             None if grad_out is None else grad_out.data_ptr(), B, loss_div, float(target),
                                             self._table(out, loss, grad_poses, grad_betas, ws),
                                             torch.cuda.current_stream(self.device).cuda_stream)
        _cabi.check(rc, None, self.lib)

    def _chunks(self, poses, betas, target=None, grad_out=None, want_out=False, want_loss=False, want_poses=False, want_betas=False,
                bufs=None):
        """One C call per chunk of max_batch items -> (out, loss, grad_poses, grad_betas), None where not asked for.  A forward when no
        gradient is wanted.  The loss of a chunked batch: every chunk divides by the whole batch's size, the chunks' values are added.
        bufs: a dict of preallocated 'out', 'loss', 'grad_poses', 'grad_betas' (and 'chunk_loss') to write into."""
        poses, stride, betas, B = self._inputs(poses, betas)
        bufs = bufs or {}
        f = lambda k, *s: bufs[k] if k in bufs else torch.empty(*s, device=self.device, dtype=torch.float32)      # noqa: E731
        grad = want_poses or want_betas
        out = f("out", B, N_OUT) if want_out or not grad else None
        loss = f("loss", ()) if want_loss else None
        gp = f("grad_poses", B, N_JOINTS, 3, 3) if want_poses else None
        gb = f("grad_betas", B, 10) if want_betas else None
        tgt = 0.0 if target is None else target
        for i in range(0, B, self.max_batch):
            n = min(self.max_batch, B - i)
            sl = slice(i, i + n)
            l_i = loss if loss is None or i == 0 else f("chunk_loss", ())
            kw = dict(out=None if out is None else out[sl], loss=l_i, target=tgt, loss_div=B)
            if grad:
                self.backward_raw(poses[sl], stride, betas[sl], n, grad_out=None if grad_out is None else grad_out[sl],
                                  grad_poses=None if gp is None else gp[sl], grad_betas=None if gb is None else gb[sl], **kw)
            else:
                self.forward_raw(poses[sl], stride, betas[sl], n, **kw)
            if loss is not None and i > 0:
                torch.add(loss, l_i, out=loss)
        return out, loss, gp, gb

    # ---- the reference's surface ----
    def __call__(self, poses, betas):
        """discriminator.py:52-99: poses (B,23,3,3) (any shape of B x 207 values), betas (B,10) -> (B,25)."""
        if torch.is_grad_enabled() and (poses.requires_grad or betas.requires_grad):
            return _DiscFn.apply(self, poses, betas)
        return self._chunks(poses, betas, want_out=True)[0]

    forward = __call__

    def loss(self, poses, betas, target):
        """L(target) = ((D(poses, betas) - target)^2).sum() / B as a 0-dim device tensor; differentiable by both inputs."""
        if torch.is_grad_enabled() and (poses.requires_grad or betas.requires_grad):
            return _LossFn.apply(self, float(target), poses, betas)
        return self._chunks(poses, betas, target=float(target), want_out=True, want_loss=True)[1]

    def value_and_grad(self, poses, betas, target=1.0, bufs=None):
        """-> (out (B,25), L(target), d L / d poses (B,23,3,3), d L / d betas (B,10)) from one thmr_disc_backward call per chunk."""
        return self._chunks(poses, betas, target=float(target), want_out=True, want_loss=True, want_poses=True, want_betas=True, bufs=bufs)

    def adversarial_loss(self, body_pose, betas):
        """loss_adv, the generator's term (tokenhmr.py:392-393)."""
        return self.loss(body_pose, betas, 1.0)

    def discriminator_loss(self, body_pose, betas, gt_body_pose_aa, gt_betas):
        """loss_disc = loss_fake + loss_real (tokenhmr.py:354-362): the prediction against 0 — detached, as there — and the mocap batch,
        (B,69) axis-angle through aa_to_rotmat, against 1.  -> a 0-dim device tensor without a graph."""
        from . import ops
        with torch.no_grad():
            B = betas.shape[0]
            loss_fake = self.loss(body_pose.detach(), betas.detach(), 0.0)
            aa = gt_body_pose_aa.detach().to(self.device, torch.float32).reshape(-1, 3).contiguous()
            gt_rotmat = ops.aa_to_rotmat(aa).view(B, N_JOINTS, 3, 3)
            loss_real = self.loss(gt_rotmat, gt_betas, 1.0)
            return loss_fake + loss_real
