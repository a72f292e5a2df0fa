"""TEST INFRASTRUCTURE ONLY — two restatements of the SMPL-H forward that csrc/body_model.hip is held to (smplx is installed nowhere, so
neither is pinned against smplx itself).

  (a) `smplh_forward_independent`: fp64 NumPy, derived from the SMPL paper like oracle/lbs_independent.py and built on ITS
      `_world` (explicit ancestor paths) — explicit 4x4 inverses of the rest chain, joints as J_regressor @ v_shaped per sample.
      It shares no algebra with the kernels.  Output: vertices (B,6890,3) and the 73 joints = 52 posed chain joints + the 21
      vertices of `extra_verts`.
  (b) `smplh_forward_smplx32`: smplx's own formulation (lbs.py: blend shapes, batch_rigid_transform in array order,
      A_j = G_j - [0 | G_j J_j], VertexJointSelector) in torch fp32 on the CPU.  It stands in for the reference's arithmetic: its
      distance to (a) is what fp32 costs on the same inputs, and the device is allowed twice that.
Plus the fold of the body-only path restated on the host (`fold_constants`) and the three errors of eval_poseVQ.py:47-55 in fp64.
"""
import numpy as np
import torch

from oracle.lbs_independent import _world, random_rotations    # noqa: F401  (random_rotations: re-exported for the tests)


def smplh_forward_independent(rotmat, betas, c, transl=None):
    """rotmat (B,NJ,3,3), betas (B,10), c: constants dict (smpl_assets.make_synthetic_smplh layout; NJ = len(parents), posedirs
    ((NJ-1)*9, 20670)) -> verts (B,6890,3), joints (B,NJ+21,3), float64."""
    f = lambda k: np.asarray(c[k], dtype=np.float64)   # noqa: E731
    vt, sd, pd, Jreg, W = f("v_template"), f("shapedirs"), f("posedirs"), f("J_regressor"), f("lbs_weights")
    parents = np.asarray(c["parents"], dtype=np.int64)
    extra = np.asarray(c["extra_verts"], dtype=np.int64)
    R_all, betas = np.asarray(rotmat, dtype=np.float64), np.asarray(betas, dtype=np.float64)
    B, NJ, V = R_all.shape[0], parents.shape[0], vt.shape[0]
    verts, joints = np.zeros((B, V, 3)), np.zeros((B, NJ + extra.shape[0], 3))
    I3 = np.eye(3)
    rest_R = np.broadcast_to(I3, (NJ, 3, 3))
    for b in range(B):
        R = R_all[b]
        v_shaped = vt + sd @ betas[b]
        J = Jreg @ v_shaped
        feat = np.concatenate([(R[k] - I3).reshape(-1) for k in range(1, NJ)])
        v_posed = v_shaped + (feat @ pd).reshape(V, 3)
        Gp = np.stack([_world(parents, R, J, j) for j in range(NJ)])
        Gr = np.stack([_world(parents, rest_R, J, j) for j in range(NJ)])
        Gprime = np.stack([Gp[j] @ np.linalg.inv(Gr[j]) for j in range(NJ)])
        Tv = np.einsum("vj,jrc->vrc", W, Gprime)
        vh = np.concatenate([v_posed, np.ones((V, 1))], axis=1)
        out = np.einsum("vrc,vc->vr", Tv, vh)
        verts[b] = out[:, :3] / out[:, 3:4]
        joints[b] = np.concatenate([Gp[:, :3, 3], verts[b][extra]], axis=0)
    if transl is not None:
        t = np.asarray(transl, dtype=np.float64)[:, None, :]
        verts, joints = verts + t, joints + t
    return verts, joints


def smplh_forward_smplx32(rotmat, betas, c, transl=None):
    """smplx lbs.lbs(pose2rot=False) + VertexJointSelector, torch fp32 on the CPU.  rotmat (B,52,3,3), betas (B,10)."""
    R, betas = torch.as_tensor(rotmat).float(), torch.as_tensor(betas).float()
    vt, sd, pd = c["v_template"].float(), c["shapedirs"].float(), c["posedirs"].float()
    Jreg, W = c["J_regressor"].float(), c["lbs_weights"].float()
    parents = [int(p) for p in c["parents"]]
    B, NJ = R.shape[0], len(parents)
    v_shaped = vt[None] + torch.einsum("bl,mkl->bmk", betas, sd)
    J = torch.einsum("bik,ji->bjk", v_shaped, Jreg)
    pose_feature = (R[:, 1:] - torch.eye(3)).reshape(B, -1)
    v_posed = v_shaped + torch.matmul(pose_feature, pd).view(B, -1, 3)
    rel = J.clone()
    rel[:, 1:] = J[:, 1:] - J[:, parents[1:]]
    T = torch.zeros(B, NJ, 4, 4)
    T[:, :, :3, :3], T[:, :, :3, 3], T[:, :, 3, 3] = R, rel, 1.0
    chain = [T[:, 0]]
    for i in range(1, NJ):
        chain.append(torch.matmul(chain[parents[i]], T[:, i]))
    G = torch.stack(chain, dim=1)
    posed_joints = G[:, :, :3, 3]
    Jh = torch.cat([J, torch.zeros(B, NJ, 1)], dim=2).unsqueeze(-1)
    A = G - torch.nn.functional.pad(torch.matmul(G, Jh), [3, 0, 0, 0, 0, 0, 0, 0])
    Tv = torch.matmul(W[None].expand(B, -1, -1), A.view(B, NJ, 16)).view(B, -1, 4, 4)
    vh = torch.cat([v_posed, torch.ones(B, v_posed.shape[1], 1)], dim=2)
    verts = torch.matmul(Tv, vh.unsqueeze(-1))[:, :, :3, 0]
    joints = torch.cat([posed_joints, verts[:, [int(i) for i in c["extra_verts"]]]], dim=1)
    if transl is not None:
        t = torch.as_tensor(transl).float().unsqueeze(1)
        verts, joints = verts + t, joints + t
    return verts, joints


def batch_rodrigues64(aa):
    """Axis-angle (n,3) -> (n,3,3) in fp64 by Rodrigues' closed form with smplx's epsilon (lbs.batch_rodrigues)."""
    aa = np.asarray(aa, dtype=np.float64)
    angle = np.linalg.norm(aa + 1e-8, axis=1, keepdims=True)
    d = aa / angle
    K = np.zeros((aa.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -d[:, 2], d[:, 1], d[:, 2], -d[:, 0], -d[:, 1], d[:, 0]
    s, cth = np.sin(angle)[:, :, None], np.cos(angle)[:, :, None]
    return np.eye(3)[None] + s * K + (1 - cth) * (K @ K)


def fold_constants(c, n_body=22):
    """The body-only path's constants restated on the host: every joint >= n_body folded into its nearest ancestor below n_body
    (weights added, regressor / parents / posedirs cut to the body joints).  For (a): 22-joint model == 52-joint model with identity
    hands, EXCEPT the posed hand joints, which the folded model does not have."""
    parents = [int(p) for p in c["parents"]]
    fold = list(range(len(parents)))
    for j in range(n_body, len(parents)):
        fold[j] = fold[parents[j]]
    W = c["lbs_weights"].double()
    Wf = torch.zeros(W.shape[0], n_body, dtype=torch.float64)
    for j, a in enumerate(fold):
        Wf[:, a] += W[:, j]
    out = dict(c)
    out.update(lbs_weights=Wf, parents=c["parents"][:n_body], J_regressor=c["J_regressor"][:n_body],
               posedirs=c["posedirs"][:(n_body - 1) * 9])
    return out


def mean_row_dist64(a, b, lo=0, hi=None):
    """eval_poseVQ.py:47-55 in fp64: sqrt(((a - b)^2).sum(-1)).mean() over rows [lo, hi) of (B, n, 3)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = a[:, lo:hi] - b[:, lo:hi]
    return float(np.sqrt((d * d).sum(-1)).mean())
