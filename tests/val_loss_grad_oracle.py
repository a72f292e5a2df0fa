"""NumPy float64 closed form of the gradient of the reference's loss, for the tests of thmr_val_loss_grad.

    compute_loss            tokenhmr/lib/models/tokenhmr.py:190-277   (sums over the batch: nothing is divided by B)
    the loss modules        tokenhmr/lib/models/losses.py:36-228      (L1Loss on the keypoints: sign(0) = 0; MSELoss on the parameters)
    pred_cam_t, projection  tokenhmr.py:166-168, 183-185; perspective_projection (utils/geometry.py)

The masks are tests/val_loss_oracle.py's: constants for the gradient (in the reference they pass through `>` and .bool()).
Pinned to the reference's own float64 autograd (tests/golden/val_loss_grad.npz) and to a torch restatement in
tests/test_val_loss_grad_host.py.  A plain module: no fixtures, no pytest hooks.
"""
import numpy as np
import torch

import val_loss_oracle as VO

SLOTS = ("kp2d", "kp3d", "joints", "cam", "rotmat", "betas")
# The shapes of tests/test_gpu_val_loss_grad.py, (B, pelvis_id): one wave, a full workgroup, one past it, sixteen workgroups and a ragged
# one; the reference's pelvis and lane 0.  Their seeds were accepted by input_conditions() (tests/test_val_loss_grad_host.py asserts it).
GPU_SHAPES = [(B, pelvis_id) for B in (1, 4, 5, 67) for pelvis_id in (39, 0)]


def gpu_seed(B, pelvis_id):
    return 5001 if B == 67 else 5000          # 5000 puts an angle of the 67-item batch within 1e-3 relative of its threshold


def project64(joints, cam, focal_length, image_size):
    """(B,44,3), (B,3) -> (t (B,3), kp2d (B,44,2)): t = (cam1, cam2, 2F / (S cam0 + 1e-9)), (u, v) = (F / S) X_xy / X_z, X = J + t."""
    J, cam = np.asarray(joints, dtype=np.float64), np.asarray(cam, dtype=np.float64)
    t = np.stack([cam[:, 1], cam[:, 2], 2.0 * focal_length / (image_size * cam[:, 0] + 1e-9)], 1)
    X = J + t[:, None]
    return t, (focal_length / image_size) * X[:, :, :2] / X[:, :, 2:]


def chain_view(inp, focal_length, image_size):
    """`inp` as a graph that starts at the joints and pred_cam sees it: pred_keypoints_2d is the float64 projection, not its float32
    rounding, and a keypoint whose given prediction equals its ground truth bit for bit (the planted one) keeps that property — its ground
    truth becomes the float64 projection too."""
    kp2 = project64(inp["pred_keypoints_3d"], inp["pred_cam"], focal_length, image_size)[1]
    g2 = np.asarray(inp["gt_keypoints_2d"], dtype=np.float64).copy()
    same = (np.asarray(inp["pred_keypoints_2d"]) == np.asarray(inp["gt_keypoints_2d"])[:, :, :2]).all(2)
    g2[:, :, :2][same] = kp2[same]
    return dict(inp, pred_keypoints_2d=kp2, gt_keypoints_2d=g2)


def val_loss_grad64(inp, weights, loose=False, loose_weight=0.0, thresholds=None, valid_3d=None, pelvis_id=39, gt_is_axis_angle=True,
                    focal_length=5000.0, image_size=256.0):
    """`inp`: the arrays of scripts/gen_golden_val_loss_grad.make_inputs; weights: the five LOSS_WEIGHTS in VO.TERMS order.
    -> {'kp2d' (B,44,2), 'kp3d' (B,44,3), 'rotmat' (B,24,3,3), 'betas' (B,10)} — the partial derivatives of the total by the four
    predictions — and, where inp has 'pred_cam', 'joints' (B,44,3) and 'cam' (B,3), through the projection."""
    f = lambda k: np.asarray(inp[k], dtype=np.float64)      # noqa: E731
    w2, w3, wgo, wbp, wb = (float(x) for x in weights)
    p2, p3, R, pb = f("pred_keypoints_2d"), f("pred_keypoints_3d"), f("pred_rotmat"), f("pred_betas")
    g2, g3, gb = f("gt_keypoints_2d"), f("gt_keypoints_3d"), f("gt_betas")
    B = p2.shape[0]
    fwd = VO.val_loss64(inp, weights, loose=loose, loose_weight=loose_weight, thresholds=thresholds, valid_3d=valid_3d, pelvis_id=pelvis_id,
                        gt_is_axis_angle=gt_is_axis_angle)
    has = np.concatenate([f("has_global_orient")[:, None], np.repeat(f("has_body_pose")[:, None], 23, 1)], 1)
    if loose:
        c2 = fwd["conf2d_used"] + loose_weight * fwd["weak2d"]
        c3 = fwd["conf3d_used"]
        m = fwd["valid_rot"] + loose_weight * fwd["weak_rot"]
        hb = fwd["has_betas_used"]
    else:
        c2, c3, m, hb = g2[:, :, 2], g3[:, :, 3], has, f("has_betas")
    out = {}
    # 2D: w2d c2 sign(pred - gt)
    out["kp2d"] = w2 * c2[:, :, None] * np.sign(p2 - g2[:, :, :2])
    # 3D: c_k on row k, minus the sum of every row on the pelvis row
    d3 = (p3 - p3[:, pelvis_id:pelvis_id + 1]) - (g3[:, :, :3] - g3[:, pelvis_id:pelvis_id + 1, :3])
    c = w3 * c3[:, :, None] * np.sign(d3)
    k3 = c.copy()
    k3[:, pelvis_id] -= c.sum(1)
    out["kp3d"] = k3
    # parameters: 2 w m (P - G), joint 0 with the weight of global_orient
    Rg = VO.aa_to_rotmat64(f("gt_pose_aa").reshape(-1, 3)).reshape(B, 24, 3, 3) if gt_is_axis_angle else f("gt_pose_rotmat")
    wj = np.concatenate([[wgo], np.repeat(wbp, 23)])
    out["rotmat"] = 2.0 * (wj[None] * m)[:, :, None, None] * (R - Rg)
    out["betas"] = 2.0 * wb * hb[:, None] * (pb - gb)
    if "pred_cam" in inp:
        # the projection's adjoint, with (u, v) as the loss saw them
        cam = f("pred_cam")
        t, _ = project64(p3, cam, focal_length, image_size)
        Xz = p3[:, :, 2] + t[:, 2:3]
        fs = focal_length / image_size
        gu, gv = out["kp2d"][:, :, 0], out["kp2d"][:, :, 1]
        dX = np.stack([fs * gu / Xz, fs * gv / Xz, -(gu * p2[:, :, 0] + gv * p2[:, :, 1]) / Xz], 2)
        out["joints"] = k3 + dX
        gt = dX.sum(1)
        out["cam"] = np.stack([gt[:, 2] * (-t[:, 2] * image_size / (image_size * cam[:, 0] + 1e-9)), gt[:, 0], gt[:, 1]], 1)
    return out


def input_conditions(inp, thresholds, valid_3d, pelvis_id, plant, focal_length=5000.0, image_size=256.0, full=True):
    """What keeps a test on these inputs from hiding a sign or mask flip; raises AssertionError naming the condition.
    Every |pred - gt| that enters a sign is >= 1e-3, except the pelvis's own 3D residual (exactly 0) and the planted keypoint of item 0
    (pred == gt bit for bit in 2D and, relative to the pelvis, in 3D); every kp2d_err and angle_err is at least 1e-3 relative away from its
    threshold; every X_z >= 1; float32 and float64 evaluations of the masks and the signs agree.  `full` (a batch of at least four
    items): confidences 0 and 1, every has_* 0 and 1, valid_3d 0 and 1, and both values of every mask occur."""
    f = lambda k: np.asarray(inp[k], dtype=np.float64)      # noqa: E731
    p2, g2, p3, g3 = f("pred_keypoints_2d"), f("gt_keypoints_2d"), f("pred_keypoints_3d"), f("gt_keypoints_3d")
    B = p2.shape[0]
    d2 = p2 - g2[:, :, :2]
    d3 = (p3 - p3[:, pelvis_id:pelvis_id + 1]) - (g3[:, :, :3] - g3[:, pelvis_id:pelvis_id + 1, :3])
    free = np.ones((B, 44), dtype=bool)
    free[0, plant] = False
    assert plant != pelvis_id and (d2[0, plant] == 0).all() and (d3[0, plant] == 0).all(), "the planted keypoint has pred == gt"
    assert g2[0, plant, 2] == 1 and g3[0, plant, 3] == 1, "the planted keypoint's zero comes from sign(0), not from its confidence"
    assert (np.abs(d2[free]) >= 1e-3).all(), "a 2D difference below 1e-3"
    assert (d3[:, pelvis_id] == 0).all(), "the pelvis's own residual is exactly 0"
    free[:, pelvis_id] = False
    assert (np.abs(d3[free]) >= 1e-3).all(), "a 3D residual below 1e-3"
    t, _ = project64(p3, f("pred_cam"), focal_length, image_size)
    assert (p3[:, :, 2] + t[:, 2:3] >= 1.0).all(), "an X_z below 1"
    # the same differences in float32, as the device forms them
    p2f, g2f, p3f, g3f = (np.asarray(inp[k], dtype=np.float32) for k in ("pred_keypoints_2d", "gt_keypoints_2d", "pred_keypoints_3d", "gt_keypoints_3d"))
    d3f = (p3f - p3f[:, pelvis_id:pelvis_id + 1]) - (g3f[:, :, :3] - g3f[:, pelvis_id:pelvis_id + 1, :3])
    assert np.array_equal(np.sign(p2f - g2f[:, :, :2]), np.sign(d2)) and np.array_equal(np.sign(d3f), np.sign(d3)), "fp32 and fp64 signs differ"
    # thresholds: relative margins, and the masks in both precisions
    thr2 = np.asarray(thresholds["kp2d"], dtype=np.float64)
    thr_a = np.concatenate([np.asarray(thresholds["global_orient"], dtype=np.float64), np.asarray(thresholds["body_pose"], dtype=np.float64)])
    err2 = g2[:, :, 2] * (d2 ** 2).sum(2)
    assert (np.abs(err2 - thr2[None]) >= 1e-3 * thr2[None]).all(), "a kp2d_err within 1e-3 relative of its threshold"
    masks = {}
    for gt_is_aa in (True, False):
        Rg = VO.aa_to_rotmat64(f("gt_pose_aa").reshape(-1, 3)).reshape(B, 24, 3, 3) if gt_is_aa else f("gt_pose_rotmat")
        ang = VO.joint_angle_error64(f("pred_rotmat"), Rg)
        assert (np.abs(ang - thr_a[None]) >= 1e-3 * thr_a[None]).all(), "an angle_err within 1e-3 relative of its threshold"
        Rg32 = (VO.aa_to_rotmat64(np.asarray(inp["gt_pose_aa"], dtype=np.float32).reshape(-1, 3), np.float32).reshape(B, 24, 3, 3) if gt_is_aa
                else np.asarray(inp["gt_pose_rotmat"], dtype=np.float32))
        ang32 = VO.joint_angle_error64(np.asarray(inp["pred_rotmat"], dtype=np.float32), Rg32, np.float32)
        assert np.array_equal(ang32 > thr_a[None].astype(np.float32), ang > thr_a[None]), "fp32 and fp64 angle masks differ"
        masks[gt_is_aa] = VO.val_loss64(inp, [1.0] * 5, loose=True, loose_weight=0.5, thresholds=thresholds, valid_3d=valid_3d,
                                        pelvis_id=pelvis_id, gt_is_axis_angle=gt_is_aa)
    err2f = g2f[:, :, 2] * ((p2f - g2f[:, :, :2]) ** 2).sum(2, dtype=np.float32)
    assert np.array_equal(err2f > thr2[None].astype(np.float32), err2 > thr2[None]), "fp32 and fp64 2D masks differ"
    if full:
        v3 = np.asarray(valid_3d)
        assert set(np.unique(v3)) == {0.0, 1.0}, "valid_3d takes both values"
        for k in ("has_global_orient", "has_body_pose", "has_betas"):
            assert set(np.unique(f(k))) == {0.0, 1.0}, k
        assert set(np.unique(g2[:, :, 2])) == {0.0, 1.0} and set(np.unique(g3[:, :, 3])) == {0.0, 1.0}, "confidences take both values"
        for m in masks.values():
            for k in ("valid2d", "weak2d", "valid_rot", "weak_rot", "conf2d_used", "conf3d_used", "has_betas_used"):
                assert set(np.unique(m[k])) == {0.0, 1.0}, f"{k} takes one value only"


# ------------------------------------------------------------------------------------------------ the same loss in torch, for autograd
def aa_to_rotmat_torch(aa):
    """VO.aa_to_rotmat64's formula (geometry.py:14-44) in torch, in aa's dtype: (n,3) -> (n,3,3)."""
    angle = ((aa + 1e-8) ** 2).sum(1, keepdim=True).sqrt()
    n = aa / angle
    q = torch.cat([torch.cos(0.5 * angle), torch.sin(0.5 * angle) * n], 1)
    q = q / (q ** 2).sum(1, keepdim=True).sqrt()
    w, x, y, z = q.unbind(1)
    w2, x2, y2, z2, wx, wy, wz, xy, xz, yz = w * w, x * x, y * y, z * z, w * x, w * y, w * z, x * y, x * z, y * z
    return torch.stack([w2 + x2 - y2 - z2, 2 * xy - 2 * wz, 2 * wy + 2 * xz, 2 * wz + 2 * xy, w2 - x2 + y2 - z2, 2 * yz - 2 * wx,
                        2 * xz - 2 * wy, 2 * wx + 2 * yz, w2 - x2 - y2 + z2], 1).reshape(-1, 3, 3)


def torch_grads(inp, weights, dtype, loose=False, loose_weight=0.0, thresholds=None, valid_3d=None, pelvis_id=39, gt_is_axis_angle=True,
                focal_length=5000.0, image_size=256.0):
    """The six slots by torch autograd of a restatement of compute_loss in `dtype` (torch.float64: the truth; torch.float32: the measure
    of the arithmetic's own rounding on these inputs).  The masks enter as constants, from VO.val_loss64 — input_conditions() holds that
    float32 and float64 agree on them.  Two graphs: the four predictions as leaves, then joints and pred_cam through the projection."""
    t = lambda k: torch.from_numpy(np.ascontiguousarray(inp[k])).to(dtype)      # noqa: E731
    w2, w3, wgo, wbp, wb = (float(x) for x in weights)
    B = inp["pred_betas"].shape[0]
    g2, g3, gb = t("gt_keypoints_2d"), t("gt_keypoints_3d"), t("gt_betas")
    has = torch.cat([t("has_global_orient")[:, None], t("has_body_pose")[:, None].repeat(1, 23)], 1)
    if loose:
        fwd = VO.val_loss64(inp, weights, loose=True, loose_weight=loose_weight, thresholds=thresholds, valid_3d=valid_3d, pelvis_id=pelvis_id,
                            gt_is_axis_angle=gt_is_axis_angle)
        m_ = lambda k: torch.from_numpy(fwd[k]).to(dtype)      # noqa: E731
        c2s, c2w, c3, ms, mw, hb = m_("conf2d_used"), m_("weak2d"), m_("conf3d_used"), m_("valid_rot"), m_("weak_rot"), m_("has_betas_used")
    else:
        c2s, c2w, c3, ms, mw, hb = g2[:, :, 2], None, g3[:, :, 3], has, None, t("has_betas")
    Rg = aa_to_rotmat_torch(t("gt_pose_aa").reshape(-1, 3)).reshape(B, 24, 3, 3) if gt_is_axis_angle else t("gt_pose_rotmat")

    def total(kp2d, kp3d, R, betas):
        l1 = (kp2d - g2[:, :, :2]).abs()
        loss2 = (c2s[:, :, None] * l1).sum()
        d3 = ((kp3d - kp3d[:, pelvis_id:pelvis_id + 1]) - (g3[:, :, :3] - g3[:, pelvis_id:pelvis_id + 1, :3])).abs()
        loss3 = (c3[:, :, None] * d3).sum()
        sq = ((R - Rg) ** 2).sum((2, 3))
        lgo, lbp = (ms[:, :1] * sq[:, :1]).sum(), (ms[:, 1:] * sq[:, 1:]).sum()
        if loose:
            loss2 = loss2 + loose_weight * (c2w[:, :, None] * l1).sum()
            lgo, lbp = lgo + loose_weight * (mw[:, :1] * sq[:, :1]).sum(), lbp + loose_weight * (mw[:, 1:] * sq[:, 1:]).sum()
        lb = (hb[:, None] * (betas - gb) ** 2).sum()
        return w3 * loss3 + w2 * loss2 + ((wgo * lgo + wbp * lbp) + wb * lb)

    leaf = lambda k: t(k).clone().requires_grad_(True)      # noqa: E731
    ins = [leaf("pred_keypoints_2d"), leaf("pred_keypoints_3d"), leaf("pred_rotmat"), leaf("pred_betas")]
    g = torch.autograd.grad(total(*ins), ins)
    out = {"kp2d": g[0], "kp3d": g[1], "rotmat": g[2], "betas": g[3]}
    if "pred_cam" in inp:
        J, cam = leaf("pred_keypoints_3d"), leaf("pred_cam")
        tr = torch.stack([cam[:, 1], cam[:, 2], 2 * focal_length / (image_size * cam[:, 0] + 1e-9)], -1)
        X = J + tr[:, None]
        kp2d = (focal_length / image_size) * X[:, :, :2] / X[:, :, 2:]
        # a keypoint given with pred == gt bit for bit (the planted one) is compared with this graph's own projection: an exact 0 in every
        # precision, as the loss saw it — not the rounding residue of a projection computed again
        same = (t("pred_keypoints_2d") == g2[:, :, :2]).all(-1, keepdim=True)
        g2 = torch.cat([torch.where(same, kp2d.detach(), g2[:, :, :2]), g2[:, :, 2:]], -1)
        out["joints"], out["cam"] = torch.autograd.grad(total(kp2d, J, t("pred_rotmat"), t("pred_betas")), [J, cam])
    return out
