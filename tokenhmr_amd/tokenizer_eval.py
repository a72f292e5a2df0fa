"""The tokenizer's evaluation on the device: tokenization/utils/eval_poseVQ.py:70-143 eval_pose_vqvae.

    from tokenhmr_amd.tokenizer_eval import TokenizerEvaluator, run_eval
    metrics = run_eval(net, val_loader, body_model_gt=SMPLH(body_model_dir))      # the loop of eval_poseVQ.py:82-100, then :109-115
    curr_score = metrics["curr_score"]                                           # jnt_recons + mesh_recons, the checkpoint criterion

The three reconstruction errors (:47-55) are one kernel, `thmr_op_mean_row_dist`; a batch enqueues three launches and one small
accumulation, and nothing leaves the device until `get_metrics_dict()`, which synchronises once (the reference calls `.item()` five
times per batch).  The running sums are kept in float64 like the reference's Python floats.

The reference divides the sums by `batch_idx` — the LAST index, one less than the number of batches (:109-110) — so its reported
means are too large by n / (n - 1) and a single batch is a division by zero.  `mean="reference"` (the default) reproduces that divisor
and raises ValueError for a single batch; `mean="batches"` divides by the true count.  `results*.pkl`, `best_net.pth`, the log line
and the renders of the reference's function stay with the caller.
"""
import ctypes as C

import torch

from . import _cabi

KEYS = ("val/curr_pose_recons", "val/curr_mesh_recons", "val/curr_jnt_recons", "val/curr_perplexity", "val/curr_commit")


def _p(t):
    return C.c_void_p(t.data_ptr())


def mean_row_dist(a, b, row_lo=0, row_hi=None, out=None, workspace=None, lib=None):
    """mean_i ||a_i - b_i||_2 over rows [row_lo, row_hi) of every item of two (B, n, 3) device tensors -> a 0-dim device tensor (or
    `out`, one float).  No host synchronisation."""
    if a.dim() != 3 or a.shape[-1] != 3 or a.shape != b.shape:
        raise ValueError(f"mean_row_dist expects two (B, n, 3) tensors of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    B, n = int(a.shape[0]), int(a.shape[1])
    row_hi = n if row_hi is None else int(row_hi)
    if B < 1 or not 0 <= row_lo < row_hi <= n:
        raise ValueError(f"mean_row_dist: rows [{row_lo}, {row_hi}) of {n}, {B} items")
    lib = lib if lib is not None else _cabi.load()
    a, b = a.float().contiguous(), b.to(a.device).float().contiguous()
    out = out if out is not None else torch.empty((), device=a.device, dtype=torch.float32)
    workspace = workspace if workspace is not None else torch.empty(_cabi.MEAN_ROW_DIST_WS, device=a.device, dtype=torch.float32)
    with torch.cuda.device(a.device):
        st = C.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)
        _cabi.check(lib.thmr_op_mean_row_dist(_p(a), _p(b), n, int(row_lo), row_hi, B, _p(out), _p(workspace), st), lib=lib)
    return out


class TokenizerEvaluator:
    def __init__(self, device="cuda:0", mean="reference"):
        if mean not in ("reference", "batches"):
            raise ValueError(f"mean is 'reference' (divide by the last batch index, eval_poseVQ.py:109-110) or 'batches', got {mean!r}")
        self.mean = mean
        self.device = torch.device(device)
        self.sums = torch.zeros(5, device=self.device, dtype=torch.float64)      # in KEYS order
        self.batches = 0
        self._cur = torch.zeros(5, device=self.device, dtype=torch.float32)
        self._ws = torch.empty(_cabi.MEAN_ROW_DIST_WS, device=self.device, dtype=torch.float32)

    def __call__(self, batch, output, loss_commit, perplexity):
        """batch: 'gt_pose_body' (B,21,3,3), 'body_vertices' (B,6890,3), 'body_joints' (B,73,3); output: the tokenizer's dict with
        'pred_pose_body_rotmat', 'pred_body_vertices', 'pred_body_joints'; the two scalars as the tokenizer returns them."""
        for k in ("pred_pose_body_rotmat", "pred_body_vertices", "pred_body_joints"):
            if k not in output:
                raise KeyError(f"the tokenizer's output lacks '{k}': build it with mesh_inference=True and a body_model")
        dev = self.device
        pairs = ((batch["gt_pose_body"], output["pred_pose_body_rotmat"], 0, None),       # eval_poseVQ.py:47-48, rows of the matrices
                 (batch["body_vertices"], output["pred_body_vertices"], 0, None),         # :50-51
                 (batch["body_joints"], output["pred_body_joints"], 1, 22))               # :53-55, valid_joints = 1..21
        cur = self._cur
        for i, (gt, pred, lo, hi) in enumerate(pairs):
            gt, pred = gt.to(dev).float(), pred.to(dev).float()
            B = gt.shape[0]
            if gt.numel() != pred.numel() or pred.shape[0] != B:
                raise ValueError(f"{KEYS[i]}: ground truth {tuple(gt.shape)} and prediction {tuple(pred.shape)} differ")
            mean_row_dist(gt.reshape(B, -1, 3), pred.reshape(B, -1, 3), lo, hi, out=cur[i], workspace=self._ws)
        cur[3].copy_(perplexity.to(dev).float().reshape(()))
        cur[4].copy_(loss_commit.to(dev).float().reshape(()))
        self.sums += cur.double()
        self.batches += 1

    def get_metrics_dict(self):
        div = self.batches - 1 if self.mean == "reference" else self.batches
        if self.batches < 1:
            raise ValueError("no batch was evaluated")
        if div == 0:
            raise ValueError("mean='reference' divides by batch_idx, the last batch index (eval_poseVQ.py:109-110): 0 after a single "
                             "batch; evaluate at least two batches or use mean='batches'")
        s = (self.sums / div).cpu().tolist()            # the one synchronisation
        m = dict(zip(KEYS, s))
        m["val/curr_jnt_recons"] *= 1000
        m["val/curr_mesh_recons"] *= 1000
        m["curr_score"] = m["val/curr_jnt_recons"] + m["val/curr_mesh_recons"]
        return m


def run_eval(net, loader, body_model_gt=None, mean="reference"):
    """eval_poseVQ.py:82-100 + :109-115.  `body_model_gt`: a `tokenhmr_amd.smplh.SMPLH`; the ground-truth vertices and joints are then
    computed on the device from batch['pose_body_aa'] (B,63) — what dataset/dataset_poseVQ.py:111-113 does per item on the CPU — and the
    loader's 'body_vertices' / 'body_joints' are not used."""
    ev = TokenizerEvaluator(device=net.device, mean=mean)
    for batch in loader:
        gt_pose = batch["gt_pose_body"].to(ev.device).float()
        if body_model_gt is not None:
            aa = batch["pose_body_aa"].to(ev.device).float()
            parts = [body_model_gt(body_pose=aa[i:i + body_model_gt.max_batch].reshape(-1, 63))
                     for i in range(0, aa.shape[0], body_model_gt.max_batch)]
            gt = {"body_vertices": torch.cat([p.vertices for p in parts], 0), "body_joints": torch.cat([p.joints for p in parts], 0)}
        else:
            gt = {"body_vertices": batch["body_vertices"], "body_joints": batch["body_joints"]}
        output, loss_commit, perplexity = net(gt_pose)
        ev(dict(gt, gt_pose_body=gt_pose), output, loss_commit, perplexity)
    return ev.get_metrics_dict()
