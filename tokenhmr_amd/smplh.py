"""SMPL-H body model on the GPU: drop-ins for the two smplx classes the tokenizer workflow uses.

    from tokenhmr_amd.smplh import SMPLHLayer      # was: from smplx import SMPLHLayer   tokenization/models/vanilla_pose_vqvae.py:10-17
    from tokenhmr_amd.smplh import SMPLH           # was: from smplx import SMPLH        tokenization/dataset/dataset_poseVQ.py:5,81

    body_model = SMPLHLayer(body_model_path, num_betas=10, ext='pkl')             # a directory holding SMPLH_NEUTRAL.pkl, a file, or a dict
    mesh = body_model(body_pose=pred_pose_rotmat)                                 # (B,21,3,3) -> .vertices (B,6890,3), .joints (B,73,3)
    gt = SMPLH('../data/body_models/smplh', num_betas=10, ext='pkl')(body_pose=pose_body_aa.view(-1, 63))

smplx is installed nowhere this package is built or tested, so the semantics below are RESTATED from its published source, not
pinned against it:
  * SMPLHLayer takes rotation matrices; whatever is omitted is the identity; no hand mean is added.  Omitted hands select the folded
    22-joint path of the kernels (`thmr_smplh_forward(body_only=1)`, csrc/body_model.hip); `folded_calls` / `full_calls` count which ran.
  * SMPLH takes axis-angle; an omitted body_pose / global_orient is zeros.  With use_pca=True hands arrive as `num_pca_comps`
    coefficients (omitted: zeros) and are expanded by hands_components{l,r}[:num_pca_comps]; with use_pca=False as 45 values.  Then
    pose_mean is added — zeros except hands_mean{l,r} when flat_hand_mean=False — and the full 52-joint path runs.
  * joints = the 52 posed chain joints, then the 21 vertices of config.SMPL_EXTRA_VERTS (VertexJointSelector order).
Both classes are differentiable like the ones they stand in for: under torch.is_grad_enabled(), if any pose part, betas
or transl requires grad, `vertices` and `joints` carry a graph whose backward is the device's own (`thmr_smplh_backward`, either path);
SMPLH's PCA hands and mean pose are torch ops above the call and differentiate by themselves.  Otherwise exactly the plain path: the
same launches and the same bits.  `enable_grad(paths=...)` reserves the backward's workspace ahead of a graph capture.
One reference quirk follows and is reproduced, not corrected: the dataset's SMPLH(flat_hand_mean=False) gives the ground-truth mesh
relaxed hands while the decoder's SMPLHLayer gives the predicted mesh flat hands, so the reference's mesh error carries a constant
hand term.
"""
import ctypes as C
import os
import types

import torch

from . import _cabi
from .smpl_assets import load_smplh_pkl

_KEYS = ["v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights"]
_IKEYS = ["parents", "extra_verts"]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _constants(model, num_betas, ext, gender):
    if isinstance(model, dict):
        return model
    path = os.fspath(model)
    if os.path.isdir(path):
        path = os.path.join(path, f"SMPLH_{gender.upper()}.{ext}")      # smplx's file naming inside a model directory
    return load_smplh_pkl(path, num_betas)


GRAD_FOLDED, GRAD_FULL = 1, 2       # header: THMR_SMPLH_GRAD_*


class _SmplhFn(torch.autograd.Function):
    """forward = thmr_smplh_forward (the launches and bits of the plain path), backward = thmr_smplh_backward on the current stream.  Saves
    the inputs only: the backward recomputes the forward's intermediates.  Once differentiable: a double backward raises."""

    @staticmethod
    def forward(ctx, model, pose, betas, transl, pose2rot, body_only):
        ctx.model, ctx.pose2rot, ctx.body_only = model, pose2rot, body_only
        ctx.save_for_backward(pose, betas, transl)
        ctx.set_materialize_grads(False)            # an unused output's gradient stays None and becomes a NULL pointer, not a zero tensor
        return model._launch(pose, pose2rot, betas, transl, body_only, pose.shape[0])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_verts, g_joints):
        pose, betas, transl = ctx.saved_tensors
        if g_verts is None and g_joints is None:
            return None, None, None, None, None, None
        m, B = ctx.model, pose.shape[0]
        g_verts, g_joints = (None if g is None else g.to(m.device, torch.float32).contiguous() for g in (g_verts, g_joints))
        g_pose = torch.empty_like(pose) if ctx.needs_input_grad[1] else None
        g_betas = torch.empty_like(betas) if betas is not None and ctx.needs_input_grad[2] else None
        g_transl = torch.empty_like(transl) if transl is not None and ctx.needs_input_grad[3] else None
        m._backward(pose, ctx.pose2rot, betas, transl, ctx.body_only, B, g_verts, g_joints, g_pose, g_betas, g_transl)
        return None, g_pose, g_betas, g_transl, None, None


class _SMPLHBase(_cabi.Handle):
    no_gpu_error = _cabi.EngineError

    def __init__(self, model_path_or_constants, num_betas=10, ext="pkl", gender="neutral", use_pca=True, num_pca_comps=6,
                 flat_hand_mean=False, *, max_batch=64, device="cuda:0"):
        if num_betas != 10:
            raise ValueError(f"the SMPL-H kernels are built for 10 betas, got num_betas = {num_betas}")
        if int(max_batch) < 1:
            raise ValueError(f"max_batch must be at least 1, got {max_batch}")
        self.use_pca, self.num_pca_comps, self.flat_hand_mean = bool(use_pca), int(num_pca_comps), bool(flat_hand_mean)
        if self.use_pca and not 1 <= self.num_pca_comps <= 45:
            raise ValueError(f"num_pca_comps must be in [1, 45], got {num_pca_comps}")
        constants = _constants(model_path_or_constants, num_betas, ext, gender)
        missing = [k for k in _KEYS + _IKEYS if k not in constants]
        if missing:
            raise KeyError(f"SMPL-H constants lack {missing}")
        shapes = {"v_template": (6890, 3), "shapedirs": (6890, 3, 10), "posedirs": (459, 20670), "J_regressor": (52, 6890),
                  "lbs_weights": (6890, 52), "parents": (52,), "extra_verts": (21,)}
        for k, s in shapes.items():
            if tuple(constants[k].shape) != s:
                raise ValueError(f"SMPL-H constant '{k}' has shape {tuple(constants[k].shape)}, the kernels are built for {s}")
        super().__init__(device, "thmr_smplh", "tokenhmr_amd.smplh runs on a HIP device only", last_error="thmr_last_error")
        self.max_batch = int(max_batch)
        self.faces = constants.get("faces")
        self.folded_calls = self.full_calls = 0
        self._host = constants
        self._grad_paths = 0

    def _handle(self):
        """The device handle, created by the first forward: construction and every argument check need no GPU."""
        if self.h is None:
            c = self._host
            ts = {k: c[k].detach().float().contiguous().cpu() for k in _KEYS}
            ts.update({k: c[k].detach().to(torch.int32).contiguous().cpu() for k in _IKEYS})
            d = _cabi.SmplhDesc(**{k: ts[k].data_ptr() for k in _KEYS + _IKEYS}, on_device=0)
            self._open(C.byref(d), self.max_batch, self._index())
            self._on_device()
        return self.h

    def _on_device(self):
        pass

    # nn.Module surface the callers touch
    def cuda(self, device=None):
        return self

    def eval(self):
        return self

    def _batch(self, *tensors):
        sizes = {int(t.shape[0]) for t in tensors if t is not None}
        if len(sizes) > 1:
            raise ValueError(f"inputs disagree on the batch size: {sorted(sizes)}")
        B = sizes.pop() if sizes else 1
        if not 1 <= B <= self.max_batch:
            raise ValueError(f"batch size {B} is outside [1, max_batch = {self.max_batch}]")
        return B

    @staticmethod
    def _sized(t, B, n, name):
        if t is not None and t.numel() != B * n:
            raise ValueError(f"{name} expects {n} values per item, got shape {tuple(t.shape)}")

    def _opt(self, t, B, n):
        return None if t is None else t.reshape(B, n).to(self.device, torch.float32).contiguous()

    def enable_grad(self, paths=("folded", "full")):
        """Reserves the backward's workspace for the named paths (thmr_smplh_grad_reserve: allocates and synchronises once per path; a
        differentiable forward does it on first need for the path it runs).  'folded' is SMPLHLayer without hands, the tokenizer's call;
        'full' is everything else and costs 40 MB more.  Call it before capturing a differentiable forward + backward in a graph."""
        names = {"folded": GRAD_FOLDED, "full": GRAD_FULL}
        mask = 0
        for p in ((paths,) if isinstance(paths, str) else paths):
            if p not in names:
                raise ValueError(f"enable_grad(paths=...) takes 'folded' and / or 'full', got {p!r}")
            mask |= names[p]
        if mask & ~self._grad_paths:
            with torch.cuda.device(self.device):
                self._check(self.lib.thmr_smplh_grad_reserve(self._handle(), mask), "thmr_smplh_grad_reserve")
            self._grad_paths |= mask
        return self

    def _run(self, pose, pose2rot, betas, transl, body_only, B):
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (pose, betas, transl)):
            self.enable_grad("folded" if body_only else "full")
            return _SmplhFn.apply(self, pose, betas, transl, bool(pose2rot), bool(body_only))
        with torch.no_grad():
            return self._launch(pose, pose2rot, betas, transl, body_only, B)

    def _backward(self, pose, pose2rot, betas, transl, body_only, B, g_verts, g_joints, g_pose, g_betas, g_transl):
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            self._check(self.lib.thmr_smplh_backward(self._handle(), _p(pose), 1 if pose2rot else 0, _p(betas), _p(transl), 1 if body_only else 0,
                                                     B, _p(g_verts), _p(g_joints), _p(g_pose), _p(g_betas), _p(g_transl), st),
                        "thmr_smplh_backward")

    def _launch(self, pose, pose2rot, betas, transl, body_only, B):
        verts = torch.empty(B, 6890, 3, device=self.device, dtype=torch.float32)
        joints = torch.empty(B, 73, 3, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            self._check(self.lib.thmr_smplh_forward(self._handle(), _p(pose), 1 if pose2rot else 0, _p(betas), _p(transl), 1 if body_only else 0, B,
                                                    _p(verts), _p(joints), st), "thmr_smplh_forward")
        if body_only:
            self.folded_calls += 1
        else:
            self.full_calls += 1
        return verts, joints

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)


class SMPLHLayer(_SMPLHBase):
    """smplx.SMPLHLayer as vanilla_pose_vqvae.py:182-191 calls it: rotation matrices in, identity for whatever is omitted."""

    def forward(self, betas=None, global_orient=None, body_pose=None, left_hand_pose=None, right_hand_pose=None, transl=None):
        B = self._batch(betas, global_orient, body_pose, left_hand_pose, right_hand_pose, transl)
        for t, n, name in ((global_orient, 9, "global_orient"), (body_pose, 21 * 9, "body_pose"), (left_hand_pose, 15 * 9, "left_hand_pose"),
                           (right_hand_pose, 15 * 9, "right_hand_pose"), (betas, 10, "betas"), (transl, 3, "transl")):
            self._sized(t, B, n, name)
        self._handle()

        def rot(t, n):
            if t is None:
                return torch.eye(3, device=self.device, dtype=torch.float32).expand(B, n, 3, 3)
            return t.reshape(B, n, 3, 3).to(self.device, torch.float32)

        parts = [rot(global_orient, 1), rot(body_pose, 21)]
        body_only = left_hand_pose is None and right_hand_pose is None
        if not body_only:
            parts += [rot(left_hand_pose, 15), rot(right_hand_pose, 15)]
        full = torch.cat(parts, dim=1).contiguous()
        betas_d, transl_d = self._opt(betas, B, 10), self._opt(transl, B, 3)
        verts, joints = self._run(full, False, betas_d, transl_d, body_only, B)
        if body_only:
            full = torch.cat([full, torch.eye(3, device=self.device, dtype=torch.float32).expand(B, 30, 3, 3)], dim=1)
        return types.SimpleNamespace(vertices=verts, joints=joints, full_pose=full,
                                     betas=betas_d if betas_d is not None else torch.zeros(B, 10, device=self.device),
                                     body_pose=full[:, 1:22], global_orient=full[:, :1], transl=transl_d)


class SMPLH(_SMPLHBase):
    """smplx.SMPLH as dataset/dataset_poseVQ.py:81,111-113 calls it: axis-angle in, PCA hands, the hand pose mean added."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        c = self._host
        for k in ("hands_meanl", "hands_meanr") + (("hands_componentsl", "hands_componentsr") if self.use_pca else ()):
            if k not in c:
                raise KeyError(f"SMPL-H constants lack '{k}' (needed by SMPLH's hand parameterisation)")

    def _on_device(self):
        c = self._host
        dev = lambda t: t.detach().float().to(self.device).contiguous()     # noqa: E731
        mean = torch.zeros(156, device=self.device)
        if not self.flat_hand_mean:
            mean[66:111], mean[111:156] = dev(c["hands_meanl"]).reshape(45), dev(c["hands_meanr"]).reshape(45)
        self.pose_mean = mean
        if self.use_pca:
            self.left_hand_components = dev(c["hands_componentsl"])[:self.num_pca_comps]
            self.right_hand_components = dev(c["hands_componentsr"])[:self.num_pca_comps]

    def forward(self, betas=None, global_orient=None, body_pose=None, left_hand_pose=None, right_hand_pose=None, transl=None):
        B = self._batch(betas, global_orient, body_pose, left_hand_pose, right_hand_pose, transl)
        nh = self.num_pca_comps if self.use_pca else 45
        for t, n, name in ((global_orient, 3, "global_orient"), (body_pose, 63, "body_pose"), (left_hand_pose, nh, "left_hand_pose"),
                           (right_hand_pose, nh, "right_hand_pose"), (betas, 10, "betas"), (transl, 3, "transl")):
            self._sized(t, B, n, name)
        self._handle()
        zeros = lambda n: torch.zeros(B, n, device=self.device, dtype=torch.float32)      # noqa: E731
        go, bp = self._opt(global_orient, B, 3), self._opt(body_pose, B, 63)
        lh, rh = self._opt(left_hand_pose, B, nh), self._opt(right_hand_pose, B, nh)
        go, bp = go if go is not None else zeros(3), bp if bp is not None else zeros(63)
        lh, rh = lh if lh is not None else zeros(nh), rh if rh is not None else zeros(nh)
        if self.use_pca:
            lh, rh = lh @ self.left_hand_components, rh @ self.right_hand_components
        full = (torch.cat([go, bp, lh, rh], dim=1) + self.pose_mean).contiguous()
        betas_d, transl_d = self._opt(betas, B, 10), self._opt(transl, B, 3)
        verts, joints = self._run(full, True, betas_d, transl_d, False, B)
        return types.SimpleNamespace(vertices=verts, joints=joints, full_pose=full,
                                     betas=betas_d if betas_d is not None else zeros(10),
                                     body_pose=bp, global_orient=go, transl=transl_d)
