"""The tokenizer's reconstruction objective on the device: a drop-in for tokenization/utils/losses.py::PoseReConsLoss,
and the value and gradient of the training total of tokenization/train_poseVQ.py:152-156 in one fused entry.

    from tokenhmr_amd.tokenizer_loss import PoseReConsLoss          # was: from utils.losses import PoseReConsLoss
    Loss = PoseReConsLoss(hparams.LOSS, hparams.ARCH.NB_JOINTS, hparams.ARCH.ROT_TYPE, hparams.ARCH.SMPL_TYPE, body_model=smplh_constants)
    loss_pose = Loss.forward_pose(gt_rotmat, output)               # 0-dim device tensors, differentiable by the output_batch entry
    losses, grad6d = Loss.value_and_grad(batch, output, loss_commit)

`loss_params` is the reference's hparams.LOSS node (or a dict): POSE_LOSS / MESH_LOSS / JNT_LOSS name a kind — 'l1', 'l2', 'l1_smooth',
'wt_l2' — and ONLY_VALID_JNT keeps joints 1..21; the five weights POSE_LOSS_WT, MESH_LOSS_WT, JNT_LOSS_WT, COMMIT_LOSS_WT, LOSS_WT (1 when
absent) enter value_and_grad only.  'geodesic' and 'rotdist' raise NotImplementedError by name: acos at their clamp has no finite
gradient.  A name the reference does not know becomes 'l2', as there (losses.py:103-104).

`body_model`: SMPL-H constants (a dict, a model file or directory) or a tokenhmr_amd.smplh.SMPLHLayer.  It is needed by 'wt_l2' on the mesh
(the vertex weights) and by value_and_grad (the backward through the body model); the three forward_* methods work without it.

value_and_grad's chain runs on the device in the current stream, with no synchronisation and no allocation after the first call at a
batch size: thmr_tok_recon_loss -> thmr_smplh_backward (the folded path) -> plus the pose term's rotation-matrix gradient ->
thmr_op_rot6d_backward.  The tensors it returns are buffers of this object and are overwritten by the next call at that batch size.
"""
import ctypes as C

import numpy as np
import torch

from . import _cabi

KINDS = {"l1": 0, "l2": 1, "l1_smooth": 2, "wt_l2": 3}          # header: THMR_RECON_*
WS_BASE, WS_PER_ITEM = 3, 21                                    # header: THMR_TOK_RECON_WS_*: workspace floats
_REFUSED = ("geodesic", "rotdist")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _field(node, key, default=None):
    if isinstance(node, dict):
        return node.get(key, default)
    return getattr(node, key, default)


def calculate_vertex_weights(vertices, faces):
    """losses.py:106-119 as a host function: the min-max normalised area of every triangle of `vertices` (V,3) added to its three
    corners in face-major order (np.add.at keeps that order), repeated to (V,3).  float64.  Raises ValueError by name for faces that are
    missing, out of range or degenerate (every triangle of one area: the normalisation divides by zero)."""
    if faces is None:
        raise ValueError("calculate_vertex_weights: the SMPL-H constants carry no 'faces'")
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1:
        raise ValueError(f"calculate_vertex_weights: 'faces' must be (F,3), got {f.shape}")
    if f.min() < 0 or f.max() >= v.shape[0]:
        raise ValueError(f"calculate_vertex_weights: 'faces' name vertices outside [0, {v.shape[0]})")
    p, q, r = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(q - p, r - p), axis=1)
    lo, hi = area.min(), area.max()
    if not hi > lo:
        raise ValueError("calculate_vertex_weights: 'faces' are degenerate (every triangle has the same area; the synthetic asset's "
                         "placeholder topology is all zeros): bring a real topology")
    area = (area - lo) / (hi - lo)
    w = np.zeros((v.shape[0], 1))
    np.add.at(w[:, 0], f.reshape(-1), np.repeat(area, 3))
    return np.repeat(w, 3, axis=1)


def _recon(lib, B, pred, gt, kinds, jrange, weights, vert_w, commit, losses, grads, ws, device):
    """One thmr_tok_recon_loss call on the current stream.  pred, gt, grads: (rotmat, vertices, joints), absent terms None."""
    with torch.cuda.device(device):
        st = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        rc = lib.thmr_tok_recon_loss(_p(pred[0]), _p(gt[0]), _p(pred[1]), _p(gt[1]), _p(pred[2]), _p(gt[2]), _p(vert_w), _p(commit),
                                     kinds[0], kinds[1], kinds[2], jrange[0], jrange[1], *[float(w) for w in weights], B, _p(losses),
                                     _p(grads[0]), _p(grads[1]), _p(grads[2]), _p(ws), st)
    if rc != 0:
        _cabi.raise_error(rc, "thmr_tok_recon_loss", lib.thmr_last_error(None))


class _TermFn(torch.autograd.Function):
    """One term's mean under autograd: value and gradient come out of the same thmr_tok_recon_loss call; once differentiable."""

    @staticmethod
    def forward(ctx, loss, term, pred, gt):
        B = pred.shape[0]
        out = torch.empty(4, device=pred.device, dtype=torch.float32)
        g = torch.empty_like(pred)
        ws = torch.empty(WS_BASE + WS_PER_ITEM * B, device=pred.device, dtype=torch.float32)
        preds, gts, grads, w = [None] * 3, [None] * 3, [None] * 3, [0.0, 0.0, 0.0, 0.0, 1.0]
        preds[term], gts[term], grads[term], w[term] = pred, gt, g, 1.0
        _recon(loss.lib, B, preds, gts, loss.kinds, loss.joint_range, w, loss._vert_w(pred.device) if term == 1 else None, None, out, grads, ws,
               pred.device)
        ctx.save_for_backward(g)
        return out[term]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        g, = ctx.saved_tensors
        return None, None, g * g_out, None


class PoseReConsLoss:
    _SHAPES = ((21 * 9, "pred_pose_body_rotmat"), (6890 * 3, "pred_body_vertices"), (73 * 3, "pred_body_joints"))

    def __init__(self, loss_params, nb_joints=21, rot_type="rotmat", smpl_type="smplh", *, body_model=None, device="cuda:0", max_batch=64):
        if int(nb_joints) != 21:
            raise ValueError(f"the tokenizer's kernels are built for 21 body joints, got nb_joints = {nb_joints}")
        if str(smpl_type).lower() != "smplh":
            raise ValueError(f"the body model on the device is SMPL-H, got smpl_type = {smpl_type!r}")
        self.nb_joints, self.rot_type, self.smpl_type = int(nb_joints), rot_type, smpl_type
        self.device = torch.device(device)
        self.max_batch = int(max_batch)
        self.names, kinds = [], []
        for key, var in (("POSE_LOSS", "pose"), ("MESH_LOSS", "mesh"), ("JNT_LOSS", "jnt")):
            name = str(_field(loss_params, key, "l2"))
            if name in _REFUSED and var == "pose":
                raise NotImplementedError(f"{key} = '{name}' is not available: acos at its clamp has no finite gradient, and no shipped "
                                          "config uses it (DESIGN.md 9)")
            if name not in KINDS:
                name = "l2"                                   # losses.py:103-104: whatever get_loss does not know is MSELoss
            self.names.append(name)
            kinds.append(KINDS[name])
        self.kinds = tuple(kinds)
        self.valid_joints = list(range(1, 22)) if _field(loss_params, "ONLY_VALID_JNT", False) else None
        self.joint_range = (1, 22) if self.valid_joints is not None else (0, 73)
        self.weights = tuple(float(_field(loss_params, k, 1.0)) for k in ("POSE_LOSS_WT", "MESH_LOSS_WT", "JNT_LOSS_WT", "COMMIT_LOSS_WT",
                                                                          "LOSS_WT"))
        self._body_model_arg, self._layer, self._vw, self._buf = body_model, None, None, {}
        self._lib = None
        if self.names[1] == "wt_l2" and body_model is None:
            raise ValueError("MESH_LOSS = 'wt_l2' needs body_model= (the SMPL-H constants with their 'faces'): the vertex weights come from it")

    @property
    def lib(self):
        """The shared library, loaded by the first call that needs it: construction and every argument check need no build and no GPU."""
        if self._lib is None:
            self._lib = _cabi.load()
        return self._lib

    # ---- the body model and the vertex weights, on first need
    def _constants(self):
        from .smplh import SMPLHLayer, _constants
        bm = self._body_model_arg
        if bm is None:
            raise ValueError("this PoseReConsLoss was built without body_model=")
        return bm._host if isinstance(bm, SMPLHLayer) else _constants(bm, 10, "pkl", "neutral")

    def body_layer(self):
        """The SMPLHLayer whose folded backward value_and_grad runs: the one given, or one built on this object's device."""
        from .smplh import SMPLHLayer
        if self._layer is None:
            bm = self._body_model_arg
            self._layer = bm if isinstance(bm, SMPLHLayer) else SMPLHLayer(self._constants(), max_batch=self.max_batch, device=self.device)
            self._layer.enable_grad("folded")
        return self._layer

    def calculate_vertex_weights(self):
        """(6890,3) float64: calculate_vertex_weights() on the mesh SMPLH() returns with default arguments — the template posed by the
        mean hand pose, NOT the template — and the constants' faces.  Computed once."""
        from .smplh import SMPLH
        c = self._constants()
        if c.get("faces") is None:
            raise ValueError("calculate_vertex_weights: the SMPL-H constants carry no 'faces'")
        m = SMPLH(c, num_betas=10, ext="pkl", max_batch=1, device=self.device)
        try:
            verts = m().vertices[0].double().cpu().numpy()
        finally:
            m.close()
        return calculate_vertex_weights(verts, c["faces"].cpu().numpy() if torch.is_tensor(c["faces"]) else c["faces"])

    def _vert_w(self, device):
        if self.names[1] != "wt_l2":
            return None
        if self._vw is None:
            self._vw = torch.from_numpy(self.calculate_vertex_weights()).to(device, torch.float32).contiguous()
        return self._vw

    # ---- the reference's three methods
    def _term(self, term, gt, pred):
        n, key = self._SHAPES[term]
        if not (pred.is_cuda and pred.dtype == torch.float32):
            raise ValueError(f"'{key}' must be a float32 CUDA tensor")
        B = pred.shape[0]
        if pred.numel() != B * n or gt.numel() != B * n:
            raise ValueError(f"'{key}' and its ground truth hold {n} values per item, got {tuple(pred.shape)} and {tuple(gt.shape)}")
        gt = gt.detach().to(pred.device, torch.float32).reshape(pred.shape).contiguous()
        if torch.is_grad_enabled() and pred.requires_grad:
            return _TermFn.apply(self, term, pred.contiguous(), gt)
        with torch.no_grad():
            return _TermFn.apply(self, term, pred.contiguous(), gt)

    def forward_pose(self, gt_pose_body, output_batch):
        return self._term(0, gt_pose_body, output_batch["pred_pose_body_rotmat"])

    def forward_mesh(self, gt_mesh, output_batch):
        return self._term(1, gt_mesh, output_batch["pred_body_vertices"])

    def forward_joints(self, gt_jnts, output_batch):
        return self._term(2, gt_jnts, output_batch["pred_body_joints"])

    # ---- the fused entry
    def _buffers(self, B, dev):
        b = self._buf.get(B)
        if b is None:
            f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)      # noqa: E731
            b = dict(losses=f(4), g_rot=f(B, 21, 3, 3), g_verts=f(B, 6890, 3), g_joints=f(B, 73, 3), ws=f(WS_BASE + WS_PER_ITEM * B),
                     pose22=torch.eye(3, device=dev).repeat(B, 22, 1, 1).contiguous(), g_pose22=f(B, 22, 3, 3), g_rot_total=f(B, 21, 3, 3),
                     g6d=f(B, 21, 6))
            self._buf[B] = b
        return b

    LAUNCHES = 10      # per max_batch poses: 1 copy, 2 loss, 5 body-model backward, 1 add, 1 rot6d backward

    def value_and_grad(self, batch_gt, output, loss_commit=None):
        """batch_gt: 'gt_pose_body' (B,21,3,3) rotation matrices, 'body_vertices' (B,6890,3), 'body_joints' (B,73,3) (the reference's
        batch keys); output: the dict VanillaTokenizer returns with a body model — 'pred_pose_body_6d', 'pred_pose_body_rotmat',
        'pred_body_vertices', 'pred_body_joints'; loss_commit: a 0-dim device tensor or None.
        -> ({'loss_pose', 'loss_mesh', 'loss_jnts', 'loss'}: 0-dim device tensors, the three unweighted means and the weighted total),
           d loss / d pred_pose_body_6d (B,21,6)."""
        x6d, rot = output["pred_pose_body_6d"], output["pred_pose_body_rotmat"]
        dev, B = rot.device, rot.shape[0]
        layer = self.body_layer()
        cont = lambda t, shape: t.detach().to(dev, torch.float32).reshape(shape).contiguous()      # noqa: E731
        pred = (cont(rot, (B, 21, 3, 3)), cont(output["pred_body_vertices"], (B, 6890, 3)), cont(output["pred_body_joints"], (B, 73, 3)))
        gt = (cont(batch_gt["gt_pose_body"], (B, 21, 3, 3)), cont(batch_gt["body_vertices"], (B, 6890, 3)),
              cont(batch_gt["body_joints"], (B, 73, 3)))
        x6d = cont(x6d, (B * 21, 6))
        commit = None if loss_commit is None else loss_commit.detach().to(dev, torch.float32).reshape(1)
        b = self._buffers(B, dev)
        with torch.no_grad():
            b["pose22"][:, 1:].copy_(pred[0])
            _recon(self.lib, B, pred, gt, self.kinds, self.joint_range, self.weights, self._vert_w(dev), commit, b["losses"],
                   (b["g_rot"], b["g_verts"], b["g_joints"]), b["ws"], dev)
            for i in range(0, B, layer.max_batch):
                n = min(layer.max_batch, B - i)
                layer._backward(b["pose22"][i:i + n], False, None, None, True, n, b["g_verts"][i:i + n], b["g_joints"][i:i + n],
                                b["g_pose22"][i:i + n], None, None)
            torch.add(b["g_pose22"][:, 1:], b["g_rot"], out=b["g_rot_total"])
            with torch.cuda.device(dev):
                st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                rc = self.lib.thmr_op_rot6d_backward(_p(x6d), _p(b["g_rot_total"]), _p(b["g6d"]), B * 21, st)
            if rc != 0:
                _cabi.raise_error(rc, "thmr_op_rot6d_backward", self.lib.thmr_last_error(None))
        L = b["losses"]
        return {"loss_pose": L[0], "loss_mesh": L[1], "loss_jnts": L[2], "loss": L[3]}, b["g6d"]
