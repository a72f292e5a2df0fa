"""SMPL-H's vector-Jacobian product in float64 numpy, one pose at a time, both paths: the algebra the SMPL-H instantiations of
lbs_skin_backward_kernel and lbs_chain_backward_kernel (tokenhmr_amd/csrc/body_model.hip) are written from, in their notation and their
order of steps — tests/lbs_backward_numpy.py's SMPL restatement with the joint finish exchanged: no regressor, no remap, the 21 picked
vertices, and on the folded path the hand joints' term through their wrist.  Also here: a dtype-generic restatement of smplx's forward
(tests/smplh_oracle.py::smplh_forward_smplx32 is hard-wired to fp32; the generic one equals it bit for bit in fp32), the adjoint of the 6D
-> rotation matrix step, the three loss kinds of PoseReConsLoss with their gradients, and the reference's vertex-weight loop restated.
tests/test_smplh_grad_host.py holds each to float64 autograd.  A plain module: no fixtures, no pytest hooks."""
import numpy as np
import torch

NV, NJ, NBODY, NOUT = 6890, 52, 22, 73


def _np(c, key, dtype=np.float64):
    v = c[key]
    return (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)).astype(dtype)


# ------------------------------------------------------------------------------------------------ the forward, any dtype
def smplh_forward_generic(rotmat, betas, c, transl=None, dtype=torch.float32):
    """smplh_oracle.smplh_forward_smplx32 statement by statement, in `dtype`; differentiable by rotmat, betas and transl.
    rotmat (B,52,3,3) -> verts (B,6890,3), joints (B,73,3)."""
    R, betas = torch.as_tensor(rotmat).to(dtype), torch.as_tensor(betas).to(dtype)
    vt, sd, pd = c["v_template"].to(dtype), c["shapedirs"].to(dtype), c["posedirs"].to(dtype)
    Jreg, W = c["J_regressor"].to(dtype), c["lbs_weights"].to(dtype)
    parents = [int(p) for p in c["parents"]]
    B, nj = R.shape[0], len(parents)
    v_shaped = vt[None] + torch.einsum("bl,mkl->bmk", betas, sd)
    J = torch.einsum("bik,ji->bjk", v_shaped, Jreg)
    pose_feature = (R[:, 1:] - torch.eye(3, dtype=dtype)).reshape(B, -1)
    v_posed = v_shaped + torch.matmul(pose_feature, pd).view(B, -1, 3)
    rel = J.clone()
    rel[:, 1:] = J[:, 1:] - J[:, parents[1:]]
    T = torch.zeros(B, nj, 4, 4, dtype=dtype)
    T[:, :, :3, :3], T[:, :, :3, 3], T[:, :, 3, 3] = R, rel, 1.0
    chain = [T[:, 0]]
    for i in range(1, nj):
        chain.append(torch.matmul(chain[parents[i]], T[:, i]))
    G = torch.stack(chain, dim=1)
    posed_joints = G[:, :, :3, 3]
    Jh = torch.cat([J, torch.zeros(B, nj, 1, dtype=dtype)], dim=2).unsqueeze(-1)
    A = G - torch.nn.functional.pad(torch.matmul(G, Jh), [3, 0, 0, 0, 0, 0, 0, 0])
    Tv = torch.matmul(W[None].expand(B, -1, -1), A.view(B, nj, 16)).view(B, -1, 4, 4)
    vh = torch.cat([v_posed, torch.ones(B, v_posed.shape[1], 1, dtype=dtype)], dim=2)
    verts = torch.matmul(Tv, vh.unsqueeze(-1))[:, :, :3, 0]
    joints = torch.cat([posed_joints, verts[:, [int(i) for i in c["extra_verts"]]]], dim=1)
    if transl is not None:
        t = torch.as_tensor(transl).to(dtype).unsqueeze(1)
        verts, joints = verts + t, joints + t
    return verts, joints


def batch_rodrigues_generic(aa):
    """smplx lbs.batch_rodrigues in aa's dtype: (n,3) -> (n,3,3), differentiable."""
    angle = torch.norm(aa + 1e-8, dim=1, keepdim=True)
    d = aa / angle
    cos, sin = torch.cos(angle).unsqueeze(1), torch.sin(angle).unsqueeze(1)
    rx, ry, rz = torch.split(d, 1, dim=1)
    zeros = torch.zeros_like(rx)
    K = torch.cat([zeros, -rz, ry, rz, zeros, -rx, -ry, rx, zeros], dim=1).view(-1, 3, 3)
    return torch.eye(3, dtype=aa.dtype).unsqueeze(0) + sin * K + (1 - cos) * torch.bmm(K, K)


def with_identity_hands(R22):
    """(B,22,3,3) -> (B,52,3,3): what the folded path computes is the 52-joint model with the hands at the identity."""
    R22 = torch.as_tensor(R22)
    eye = torch.eye(3, dtype=R22.dtype).expand(R22.shape[0], NJ - NBODY, 3, 3)
    return torch.cat([R22, eye], dim=1)


# ------------------------------------------------------------------------------------------------ the backward
def fold_map(parents):
    fold = list(range(len(parents)))
    for j in range(NBODY, len(parents)):
        fold[j] = fold[int(parents[j])]
    return fold


def smplh_backward(R, betas, gV, gJ, c, body_only=False):
    """R (B,52,3,3), or (B,22,3,3) with body_only; betas (B,10) or None; gV (B,6890,3) or None; gJ (B,73,3) or None
    -> grad_R (R's shape), grad_betas (B,10), grad_transl (B,3)."""
    R = np.asarray(R, np.float64)
    B = R.shape[0]
    betas = np.zeros((B, 10)) if betas is None else np.asarray(betas, np.float64)
    vt, sd, pd, Jreg, W = _np(c, "v_template"), _np(c, "shapedirs"), _np(c, "posedirs"), _np(c, "J_regressor"), _np(c, "lbs_weights")
    parents, extra = _np(c, "parents", np.int64), _np(c, "extra_verts", np.int64)
    fold = fold_map(parents)
    NC = NBODY if body_only else NJ
    if body_only:                                          # the folded tables (smplh_fold_weights_kernel, build_dirs_kernel with npf = 189)
        Wf = np.zeros((NV, NC))
        for j in range(NJ):
            Wf[:, fold[j]] += W[:, j]
        W, pd = Wf, pd[:(NC - 1) * 9]
    dirs = np.concatenate([sd.reshape(NV * 3, 10), pd.T], axis=1)          # v_posed = v_template + dirs . x
    Jt, Jsd = Jreg @ vt, np.einsum("jv,vil->jil", Jreg, sd)                # all 52 rest joints, on either path
    gR_out, gb_out, gt_out = np.zeros((B, NC, 3, 3)), np.zeros((B, 10)), np.zeros((B, 3))
    for b in range(B):
        J = Jt + Jsd @ betas[b]
        Gr, Gt = np.zeros((NC, 3, 3)), np.zeros((NC, 3))
        Gr[0], Gt[0] = R[b, 0], J[0]
        for i in range(1, NC):
            p = parents[i]
            Gr[i] = Gr[p] @ R[b, i]
            Gt[i] = Gr[p] @ (J[i] - J[p]) + Gt[p]
        A = np.concatenate([Gr, (Gt - np.einsum("jrc,jc->jr", Gr, J[:NC]))[:, :, None]], axis=2)
        x = np.concatenate([betas[b], (R[b, 1:] - np.eye(3)).reshape(-1)])
        vposed = vt + (dirs @ x).reshape(NV, 3)
        T = np.einsum("vj,jrc->vrc", W, A)
        gj = np.zeros((NOUT, 3)) if gJ is None else np.asarray(gJ[b], np.float64)
        # skin-backward: the picked joints 52..72 land on their vertex (a vertex named by two slots receives both)
        g = np.zeros((NV, 3)) if gV is None else np.asarray(gV[b], np.float64).copy()
        for k in range(21):
            g[extra[k]] += gj[NJ + k]
        gvposed = np.einsum("vrc,vr->vc", T[:, :, :3], g)
        gT = np.einsum("vr,vc->vrc", g, np.concatenate([vposed, np.ones((NV, 1))], axis=1))
        gA = np.einsum("vj,vrc->jrc", W, gT)
        gones = gT[:, :, 3].sum(axis=0)                                    # the row of ones: sum_v g_v
        # blend reverse
        gx = gvposed.reshape(-1) @ dirs
        gbeta = gx[:10].copy()
        gR = np.zeros((NC, 3, 3))
        gR[1:] = gx[10:].reshape(NC - 1, 3, 3)
        # chain-backward
        gGr = gA[:, :, :3] - np.einsum("jr,jc->jrc", gA[:, :, 3], J[:NC])
        gGt = gA[:, :, 3] + gj[:NC]
        gJ_ = np.zeros((NJ, 3))
        gJ_[:NC] = -np.einsum("jkr,jk->jr", Gr, gA[:, :, 3])
        for j in range(NC, NJ):                                            # folded: joint_j = Gr_w (J_j - J_w) + Gt_w, w its wrist
            w = fold[j]
            gGr[w] += np.outer(gj[j], J[j] - J[w])
            gGt[w] += gj[j]
            grel = Gr[w].T @ gj[j]
            gJ_[j] += grel
            gJ_[w] -= grel
        for i in range(NC - 1, 0, -1):
            p = parents[i]
            gR[i] += Gr[p].T @ gGr[i]
            gGr[p] += gGr[i] @ R[b, i].T + np.outer(gGt[i], J[i] - J[p])
            grel = Gr[p].T @ gGt[i]
            gGt[p] += gGt[i]
            gJ_[i] += grel
            gJ_[p] -= grel
        gR[0] += gGr[0]
        gJ_[0] += gGt[0]
        gbeta += np.einsum("jil,ji->l", Jsd, gJ_)
        gR_out[b], gb_out[b], gt_out[b] = gR, gbeta, gones + gj[:NJ].sum(axis=0)
    return gR_out, gb_out, gt_out


# ------------------------------------------------------------------------------------------------ 6D -> rotation matrix
def rot6d_generic(x):
    """rotation_6d_to_matrix / geometry.rot6d_to_rotmat in x's dtype: (n,6) -> (n,3,3), rows b1, b2, b3."""
    a1, a2 = x[:, :3], x[:, 3:]
    b1 = torch.nn.functional.normalize(a1, dim=-1)
    b2 = torch.nn.functional.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)


def rot6d_backward(x, gR, eps=1e-12):
    """rot6d_backward_kernel's steps: (n,6), (n,3,3) -> (n,6)."""
    x, gR = np.asarray(x, np.float64), np.asarray(gR, np.float64)
    out = np.zeros_like(x)
    for n in range(x.shape[0]):
        a1, a2 = x[n, :3], x[n, 3:]
        l1 = np.linalg.norm(a1)
        n1 = max(l1, eps)
        b1 = a1 / n1
        dp = b1 @ a2
        u = a2 - dp * b1
        l2 = np.linalg.norm(u)
        n2 = max(l2, eps)
        b2 = u / n2
        g1, g2, g3 = gR[n]
        gb1 = g1 + np.cross(b2, g3)
        gb2 = g2 + np.cross(g3, b1)
        gu = (gb2 - b2 * ((b2 @ gb2) if l2 >= eps else 0.0)) / n2
        gdp = -(gu @ b1)
        gb1 = gb1 + gdp * a2 - dp * gu
        out[n, :3] = (gb1 - b1 * ((b1 @ gb1) if l1 >= eps else 0.0)) / n1
        out[n, 3:] = gu + gdp * b1
    return out


# ------------------------------------------------------------------------------------------------ the loss kinds
def recon_term(kind, pred, gt, w=None):
    """One term of PoseReConsLoss with mean reduction and its gradient by pred: (value, grad).  Kinks as torch: l1 gives 0 at d = 0,
    l1_smooth (beta = 1) is d below |d| = 1 and sign(d) from it on."""
    d = np.asarray(pred, np.float64) - np.asarray(gt, np.float64)
    if kind == "l1":
        val, g = np.abs(d), np.sign(d)
    elif kind == "l1_smooth":
        small = np.abs(d) < 1.0
        val, g = np.where(small, 0.5 * d * d, np.abs(d) - 0.5), np.where(small, d, np.sign(d))
    elif kind == "wt_l2" and w is not None:
        val, g = w * d * d, 2.0 * w * d
    else:
        val, g = d * d, 2.0 * d
    return val.mean(), g / d.size


def torch_term(kind, pred, gt, w=None):
    """The same term as the reference builds it (losses.py:81-104), called as the reference calls it: loss(gt, pred)."""
    if kind == "l1":
        return torch.nn.L1Loss()(gt, pred)
    if kind == "l1_smooth":
        return torch.nn.SmoothL1Loss()(gt, pred)
    if kind == "wt_l2" and w is not None:
        return torch.mean(w * (gt - pred) ** 2)
    return torch.nn.MSELoss()(gt, pred)


def loss_inputs(shape, seed, kinks=True):
    """pred = gt + d with |d| >= 1e-3 except planted exact zeros and exact +-1: fp32 and fp64 take the same branch everywhere."""
    rng = np.random.default_rng(seed)
    gt = np.round(rng.standard_normal(shape) * 4) / 4                              # exactly representable, so gt + d - gt == d in fp32
    d = rng.standard_normal(shape) * 0.8
    d = np.where(np.abs(d) < 1e-3, 0.5, d)
    d = np.where(np.abs(np.abs(d) - 1.0) < 1e-3, 0.5, d)
    d = np.round(d * 1024) / 1024
    d = np.where(d == 0, 0.5, d)
    if kinks:
        f = d.reshape(-1)
        f[0::7][:12] = 0.0
        f[1::7][:12] = 1.0
        f[2::7][:12] = -1.0
    return (gt + d).astype(np.float32), gt.astype(np.float32)


# ------------------------------------------------------------------------------------------------ vertex weights
def vertex_weights_reference_loop(vertices, faces):
    """losses.py:110-119 restated: the reference's Python loop, face by face."""
    p, q, r = (vertices[faces[:, k]] for k in range(3))
    area = 0.5 * np.linalg.norm(np.cross(q - p, r - p), axis=1)
    area = (area - area.min()) / (area.max() - area.min())
    out = np.zeros((vertices.shape[0], 1))
    for f in range(faces.shape[0]):            # face-major, corner by corner: the order the sums of a vertex are taken in
        for k in range(3):
            out[faces[f, k]] += area[f]
    return np.repeat(out, 3, axis=1)
