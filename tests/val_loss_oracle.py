"""NumPy float64 restatement of the reference's validation loss, for the tests of thmr_val_loss / thmr_op_token_ce.

    compute_loss          tokenhmr/lib/models/tokenhmr.py:190-277   (plain branch :250-262, LOOSE_SUP branch :214-249)
    the loss modules      tokenhmr/lib/models/losses.py:36-228
    joint_angle_error     losses.py:22-33
    aa_to_rotmat          tokenhmr/lib/utils/geometry.py:5-44
    matrix_to_axis_angle  tokenhmr/lib/utils/rotation_utils.py:428-441 (matrix_to_quaternion :104-163, quaternion_to_axis_angle :478-506)
    TokenLoss             losses.py:230-252

Pinned to the reference's own float64 record (tests/golden/val_loss.npz) in tests/test_val_loss_host.py.
"""
import numpy as np

LOSS_KEYS = ("loss", "loss_keypoints_2d", "loss_keypoints_3d", "loss_global_orient", "loss_body_pose", "loss_betas")
TERMS = ("keypoints_2d", "keypoints_3d", "global_orient", "body_pose", "betas")


def aa_to_rotmat64(aa, dtype=np.float64):
    """geometry.py:14-44, (n,3) -> (n,3,3): the +1e-8 inside the norm, the re-normalised quaternion, the nine quadratic forms."""
    aa = np.asarray(aa, dtype=dtype)
    half, two = dtype(0.5), dtype(2)
    angle = np.sqrt(((aa + dtype(1e-8)) ** 2).sum(1, keepdims=True))               # :14
    n = aa / angle                                                                 # :16
    q = np.concatenate([np.cos(half * angle), np.sin(half * angle) * n], 1)        # :17-20
    q = q / np.sqrt((q ** 2).sum(1, keepdims=True))                                # :32
    w, x, y, z = q.T
    w2, x2, y2, z2, wx, wy, wz, xy, xz, yz = w * w, x * x, y * y, z * z, w * x, w * y, w * z, x * y, x * z, y * z
    out = np.stack([w2 + x2 - y2 - z2, two * xy - two * wz, two * wy + two * xz, two * wz + two * xy, w2 - x2 + y2 - z2, two * yz - two * wx,
                    two * xz - two * wy, two * wx + two * yz, w2 - x2 - y2 + z2], 1).reshape(-1, 3, 3)      # :41-43
    assert out.dtype == dtype
    return out


def matrix_to_axis_angle64(m, dtype=np.float64):
    """rotation_utils.py:104-163 + :478-506, (n,3,3) -> (n,3); no quaternion standardisation (an angle above pi stays above pi).
    dtype=np.float32 runs the same formula in float32 (the tests' measure of the formula's own rounding error)."""
    m = np.asarray(m, dtype=dtype)
    one, two, tenth = dtype(1), dtype(2), dtype(0.1)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m.reshape(-1, 9).T
    q_abs = np.sqrt(np.maximum(np.stack([one + m00 + m11 + m22, one + m00 - m11 - m22, one - m00 + m11 - m22, one - m00 - m11 + m22], 1),
                               dtype(0)))                                                             # :122-132
    cand = np.stack([np.stack([q_abs[:, 0] ** 2, m21 - m12, m02 - m20, m10 - m01], 1),
                     np.stack([m21 - m12, q_abs[:, 1] ** 2, m10 + m01, m02 + m20], 1),
                     np.stack([m02 - m20, m10 + m01, q_abs[:, 2] ** 2, m12 + m21], 1),
                     np.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[:, 3] ** 2], 1)], 1)            # :135-151
    cand = cand / (two * np.maximum(q_abs, tenth))[:, :, None]                                        # :155-156
    q = cand[np.arange(len(cand)), q_abs.argmax(1)]                                                   # :161-163, lowest index on ties
    norm = np.sqrt((q[:, 1:] ** 2).sum(1, keepdims=True))                                             # :492
    half = np.arctan2(norm, q[:, :1])
    angle = two * half
    small = np.abs(angle) < dtype(1e-6)
    with np.errstate(divide="ignore", invalid="ignore"):
        so = np.where(small, dtype(0.5) - angle * angle / dtype(48), np.sin(half) / np.where(small, one, angle))      # :496-504
    out = q[:, 1:] / np.maximum(so, np.finfo(np.float32).tiny.astype(dtype))                          # safe_zero_division (:38-40)
    assert out.dtype == dtype
    return out


def joint_angle_error64(pred, gt, dtype=np.float64):
    """losses.py:22-33: |matrix_to_axis_angle(R_pred R_gt^T)| per joint, (B,J,3,3) x 2 -> (B,J)."""
    B, J = pred.shape[:2]
    p, g = np.asarray(pred, dtype=dtype).reshape(-1, 3, 3), np.asarray(gt, dtype=dtype).reshape(-1, 3, 3)
    r = np.einsum("nik,njk->nij", p, g)
    aa = matrix_to_axis_angle64(r, dtype)
    return np.sqrt((aa ** 2).sum(1)).reshape(B, J)


def val_loss64(inp, weights, loose=False, loose_weight=0.0, thresholds=None, valid_3d=None, pelvis_id=39, gt_is_axis_angle=True):
    """`inp`: the arrays of scripts/gen_golden_val_loss.make_inputs ('gt_pose_aa' (B,72), or 'gt_pose_rotmat' (B,24,3,3) with
    gt_is_axis_angle=False).  weights: the five LOSS_WEIGHTS in TERMS order.  Returns a dict: 'losses' (6, LOSS_KEYS order), 'per_item'
    (B,5, TERMS order, unweighted) and — loose — kp2d_err, angle_err, the four masks and the three *_used arrays."""
    f = lambda k: np.asarray(inp[k], dtype=np.float64)      # noqa: E731
    p2, p3, R, pb = f("pred_keypoints_2d"), f("pred_keypoints_3d"), f("pred_rotmat"), f("pred_betas")
    g2, g3, gb = f("gt_keypoints_2d"), f("gt_keypoints_3d"), f("gt_betas")
    has_go, has_bp, has_b = f("has_global_orient"), f("has_body_pose"), f("has_betas")
    B = p2.shape[0]
    Rg = aa_to_rotmat64(f("gt_pose_aa").reshape(-1, 3)).reshape(B, 24, 3, 3) if gt_is_axis_angle else f("gt_pose_rotmat")      # :235 / :260
    sq9 = ((R - Rg) ** 2).sum((2, 3))                                       # (B,24): MSELoss(reduction='none') summed per joint
    has = np.concatenate([has_go[:, None], np.repeat(has_bp[:, None], 23, 1)], 1)
    l1_2d = np.abs(p2 - g2[:, :, :2]).sum(2)                                # (B,44)
    conf2, conf3 = g2[:, :, 2], g3[:, :, 3]
    out = {}
    if loose:
        v3 = np.asarray(valid_3d, dtype=np.float64)
        thr2 = np.asarray(thresholds["kp2d"], dtype=np.float64)
        thr_a = np.concatenate([np.asarray(thresholds["global_orient"], dtype=np.float64), np.asarray(thresholds["body_pose"], dtype=np.float64)])
        kp2d_err = conf2 * ((p2 - g2[:, :, :2]) ** 2).sum(2)                # :218-219
        valid2d = kp2d_err > thr2[None]                                     # :220
        weak2d = conf2 * ~valid2d                                           # :221
        conf2_used = conf2 * valid2d                                        # :223
        per2 = (conf2_used * l1_2d).sum(1) + loose_weight * (weak2d * l1_2d).sum(1)      # losses.py:126-131
        conf3 = conf3 * ((v3[:, None] + conf2_used) > 0.5)                  # :227
        angle = joint_angle_error64(R, Rg)                                  # :243
        valid = ((angle > thr_a[None]) * has + v3[:, None]) != 0            # :244-245
        weak = (~valid) * has                                               # :246
        per_rot = valid * sq9 + loose_weight * (weak * sq9)                 # losses.py:214-220
        per_go, per_bp = per_rot[:, 0], per_rot[:, 1:].sum(1)
        has_b = has_b * v3                                                  # :240
        out.update(kp2d_err=kp2d_err, angle_err=angle, valid2d=valid2d.astype(np.float64), weak2d=weak2d, valid_rot=valid.astype(np.float64),
                   weak_rot=weak, conf2d_used=conf2_used, conf3d_used=conf3, has_betas_used=has_b)
    else:
        per2 = (conf2 * l1_2d).sum(1)                                       # losses.py:61-64
        per_go, per_bp = has_go * sq9[:, 0], has_bp * sq9[:, 1:].sum(1)     # losses.py:187-192
    d3 = (p3 - p3[:, pelvis_id:pelvis_id + 1]) - (g3[:, :, :3] - g3[:, pelvis_id:pelvis_id + 1, :3])      # losses.py:94-95
    per3 = (conf3 * np.abs(d3).sum(2)).sum(1)
    perb = has_b * ((pb - gb) ** 2).sum(1)
    per = np.stack([per2, per3, per_go, per_bp, perb], 1)
    terms = per.sum(0)
    total = float(np.dot(np.asarray(weights, dtype=np.float64), terms))     # tokenhmr.py:264-266
    out["per_item"], out["losses"] = per, np.concatenate([[total], terms])
    return out


def token_ce64(x, target):
    """CrossEntropyLoss (mean) over rows: mean_r (logsumexp(x_r) - x_r[target_r]) — applied, as the reference writes it, to whatever
    matrix it is handed (losses.py:251 passes the softmax output)."""
    x = np.asarray(x, dtype=np.float64)
    mx = x.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(x - mx).sum(1))
    return float((lse - x[np.arange(x.shape[0]), np.asarray(target)]).mean())
