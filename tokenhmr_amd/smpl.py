"""Stand-alone SMPL model on the GPU.

Mirrors what the reference's dataset code does per sample on the CPU with `smplx.SMPL(gender=...)`
(tokenhmr/lib/datasets/image_dataset.py:151-164,254-270; emdb_dataset.py:184-199): axis-angle
`global_orient` (B,3) + `body_pose` (B,69) + `betas` (B,10) -> GT vertices — but batched, through the same LBS
kernels as the hot path, with the male / female constants held in their own `thmr_smpl` handle.
"""
import ctypes as C
import types

import torch

from . import _cabi


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class _SmplFn(torch.autograd.Function):
    """forward = thmr_smpl_forward (the launches and bits of the plain path), backward = thmr_smpl_backward on the current stream: the
    body model's own vector-Jacobian product.  Once differentiable: a double backward raises."""

    @staticmethod
    def forward(ctx, model, pose, betas, pose2rot):
        ctx.model, ctx.pose2rot = model, pose2rot
        ctx.save_for_backward(pose, betas)
        ctx.set_materialize_grads(False)            # an unused output's gradient stays None and becomes a NULL pointer, not a zero tensor
        return model._forward(pose, betas, pose2rot)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_verts, g_joints):
        pose, betas = ctx.saved_tensors
        if g_verts is None and g_joints is None:
            return None, None, None, None
        m, B = ctx.model, betas.shape[0]
        g_verts, g_joints = (None if g is None else g.to(m.device, torch.float32).contiguous() for g in (g_verts, g_joints))
        g_pose = torch.empty_like(pose) if ctx.needs_input_grad[1] else None
        g_betas = torch.empty_like(betas) if ctx.needs_input_grad[2] else None
        m._backward(pose, ctx.pose2rot, betas, B, g_verts, g_joints, g_pose, g_betas)
        return None, g_pose, g_betas, None


class SMPL(_cabi.Handle):
    no_gpu_error = _cabi.EngineError

    def __init__(self, constants, max_batch=64, device="cuda:0"):
        super().__init__(device, "thmr_smpl", "tokenhmr_amd.smpl.SMPL runs on a HIP device only", last_error="thmr_last_error")
        self.max_batch = int(max_batch)
        keys = ["v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights", "J19_regressor"]
        ikeys = ["parents", "extra_verts", "joint_map"]
        ts = {k: constants[k].detach().float().contiguous().cpu() for k in keys}
        ts.update({k: constants[k].detach().to(torch.int32).contiguous().cpu() for k in ikeys})
        d = _cabi.SmplDesc(**{k: ts[k].data_ptr() for k in keys + ikeys}, on_device=0,
                           update_hips=1 if constants.get("update_hips", False) else 0)
        self._open(C.byref(d), self.max_batch, self._index())
        self.faces = constants.get("faces")
        self._grad_ready = False

    def enable_grad(self):
        """Reserves the backward's workspace (thmr_smpl_grad_reserve: allocates and synchronises once; forward() does it on first need).
        Call it before capturing a differentiable forward + backward in a graph."""
        if not self._grad_ready:
            with torch.cuda.device(self.device):
                self._check(self.lib.thmr_smpl_grad_reserve(self.h), "thmr_smpl_grad_reserve")
            self._grad_ready = True
        return self

    def forward(self, global_orient, body_pose, betas, pose2rot=True):
        """pose2rot=True: axis-angle (B,3)+(B,69) (smplx.SMPL); False: rotation matrices (B,1,3,3)+(B,23,3,3) (SMPLLayer).
        Differentiable like the class it stands in for: under torch.is_grad_enabled(), if global_orient, body_pose or betas requires
        grad, vertices and joints carry a graph whose backward is the device's own (thmr_smpl_backward); the gradient by a rotation
        matrix is the plain derivative by its nine entries, as autograd gives it.  Otherwise exactly the plain path."""
        B = betas.shape[0]
        if pose2rot:
            pose = torch.cat([global_orient.reshape(B, 3), body_pose.reshape(B, 69)], dim=1)
        else:
            pose = torch.cat([global_orient.reshape(B, 1, 3, 3), body_pose.reshape(B, 23, 3, 3)], dim=1)
        pose = pose.to(self.device, torch.float32).contiguous()
        betas = betas.to(self.device, torch.float32).contiguous()
        if torch.is_grad_enabled() and (pose.requires_grad or betas.requires_grad):
            self.enable_grad()
            verts, joints = _SmplFn.apply(self, pose, betas, bool(pose2rot))
        else:
            verts, joints = self._forward(pose, betas, pose2rot)
        return types.SimpleNamespace(vertices=verts, joints=joints)

    def _forward(self, pose, betas, pose2rot):
        B = betas.shape[0]
        verts = torch.empty(B, 6890, 3, device=self.device, dtype=torch.float32)
        joints = torch.empty(B, 44, 3, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            self._check(self.lib.thmr_smpl_forward(self.h, _p(pose), 1 if pose2rot else 0, _p(betas), B, _p(verts), _p(joints), st),
                        "thmr_smpl_forward")
        return verts, joints

    def _backward(self, pose, pose2rot, betas, B, g_verts, g_joints, g_pose, g_betas):
        """One thmr_smpl_backward call on the current stream (B <= max_batch, contiguous float32 tensors of this device, enable_grad()
        done): a None gradient input is zeros, a None output is not computed."""
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            self._check(self.lib.thmr_smpl_backward(self.h, _p(pose), 1 if pose2rot else 0, _p(betas), B, _p(g_verts), _p(g_joints),
                                                    _p(g_pose), _p(g_betas), st), "thmr_smpl_backward")

    __call__ = forward
