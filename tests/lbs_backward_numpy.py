"""The body model's vector-Jacobian product in float64 numpy, one crop at a time: the algebra the kernels of
tokenhmr_amd/csrc/body_model.hip (lbs_skin_backward_kernel, lbs_chain_backward_kernel, rodrigues_backward_kernel) are written from, in
their notation and their order of steps.  tests/test_smpl_grad_host.py holds it to float64 autograd of oracle.tokenhmr_oracle.smpl_forward.
A plain module: no fixtures, no pytest hooks."""
import numpy as np

NV, NJ = 6890, 24


def _np(smpl, key, dtype=np.float64):
    v = smpl[key]
    return (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)).astype(dtype)


def forward_chain(R, betas, smpl):
    """One crop: J (24,3), Gr (24,3,3), Gt (24,3) as prep_kernel computes them."""
    vt, sd, Jreg = _np(smpl, "v_template"), _np(smpl, "shapedirs"), _np(smpl, "J_regressor")
    parents = _np(smpl, "parents", np.int64)
    Jt = Jreg @ vt                                        # (24,3)
    Jsd = np.einsum("jv,vil->jil", Jreg, sd)              # (24,3,10)
    J = Jt + Jsd @ betas
    Gr, Gt = np.zeros((NJ, 3, 3)), np.zeros((NJ, 3))
    Gr[0], Gt[0] = R[0], J[0]
    for i in range(1, NJ):
        p = parents[i]
        Gr[i] = Gr[p] @ R[i]
        Gt[i] = Gr[p] @ (J[i] - J[p]) + Gt[p]
    return J, Jsd, Gr, Gt


def joint_adjoint(gJ, smpl):
    """Step 1: (44,3) -> gJtr (24,3), the per-vertex additions of the picked slots as a (6890,3) array, g19 (19,3)."""
    jmap, extra = _np(smpl, "joint_map", np.int64), _np(smpl, "extra_verts", np.int64)
    gm, g19 = gJ[:25].copy(), gJ[25:]
    if smpl.get("update_hips", False):
        g9, g12, g8 = gm[9].copy(), gm[12].copy(), gm[8].copy()
        gm[9], gm[12], gm[8] = g9 - 0.5 * g12, g12 - 0.5 * g9, g8 + 0.5 * (g9 + g12)
    gJtr, gpick = np.zeros((NJ, 3)), np.zeros((NV, 3))
    for slot in range(25):
        src = jmap[slot]
        if src < NJ:
            gJtr[src] += gm[slot]
        else:
            gpick[extra[src - NJ]] += gm[slot]            # a vertex id named by two slots receives both
    return gJtr, gpick, g19


def smpl_backward(R, betas, gV, gJ, smpl):
    """R (B,24,3,3), betas (B,10), gV (B,6890,3) or None, gJ (B,44,3) or None -> (grad_R (B,24,3,3), grad_betas (B,10))."""
    R, betas = np.asarray(R, np.float64), np.asarray(betas, np.float64)
    B = R.shape[0]
    vt, sd, pd = _np(smpl, "v_template"), _np(smpl, "shapedirs"), _np(smpl, "posedirs")
    W, J19 = _np(smpl, "lbs_weights"), _np(smpl, "J19_regressor")
    parents = _np(smpl, "parents", np.int64)
    dirs = np.concatenate([sd.reshape(NV * 3, 10), pd.T], axis=1)          # (20670, 217): v_posed = v_template + dirs . x
    gR_out, gb_out = np.zeros((B, NJ, 3, 3)), np.zeros((B, 10))
    for b in range(B):
        J, Jsd, Gr, Gt = forward_chain(R[b], betas[b], smpl)
        A = np.concatenate([Gr, (Gt - np.einsum("jrc,jc->jr", Gr, J))[:, :, None]], axis=2)      # (24,3,4)
        x = np.concatenate([betas[b], (R[b, 1:] - np.eye(3)).reshape(-1)])
        vposed = vt + (dirs @ x).reshape(NV, 3)
        T = np.einsum("vj,jrc->vrc", W, A)                                                      # (6890,3,4)
        # step 1
        gJtr, gpick, g19 = joint_adjoint(np.zeros((44, 3)) if gJ is None else np.asarray(gJ[b], np.float64), smpl)
        # step 2
        g = (np.zeros((NV, 3)) if gV is None else np.asarray(gV[b], np.float64)) + J19.T @ g19 + gpick
        gvposed = np.einsum("vrc,vr->vc", T[:, :, :3], g)
        gT = np.einsum("vr,vc->vrc", g, np.concatenate([vposed, np.ones((NV, 1))], axis=1))     # (6890,3,4)
        gA = np.einsum("vj,vrc->jrc", W, gT)                                                    # (24,3,4)
        # step 3
        gx = gvposed.reshape(-1) @ dirs
        gbeta = gx[:10].copy()
        gR = np.zeros((NJ, 3, 3))
        gR[1:] = gx[10:].reshape(23, 3, 3)
        # step 4
        gGr = gA[:, :, :3] - np.einsum("jr,jc->jrc", gA[:, :, 3], J)
        gGt = gA[:, :, 3] + gJtr
        gJ_ = -np.einsum("jkr,jk->jr", Gr, gA[:, :, 3])
        for i in range(NJ - 1, 0, -1):
            p = parents[i]
            rel = J[i] - J[p]
            gR[i] += Gr[p].T @ gGr[i]
            gGr[p] += gGr[i] @ R[b, i].T + np.outer(gGt[i], rel)
            grel = Gr[p].T @ gGt[i]
            gGt[p] += gGt[i]
            gJ_[i] += grel
            gJ_[p] -= grel
        gR[0] += gGr[0]
        gJ_[0] += gGt[0]
        gbeta += np.einsum("jil,ji->l", Jsd, gJ_)
        gR_out[b], gb_out[b] = gR, gbeta
    return gR_out, gb_out


def rodrigues(aa, eps=1e-8):
    """rodrigues_kernel's formula, (n,3) -> (n,3,3)."""
    aa = np.asarray(aa, np.float64)
    out = np.zeros((aa.shape[0], 3, 3))
    for n, r in enumerate(aa):
        a = np.linalg.norm(r + eps)
        d = r / a
        K = np.array([[0, -d[2], d[1]], [d[2], 0, -d[0]], [-d[1], d[0], 0]])
        out[n] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    return out


def rodrigues_backward(aa, gR, eps=1e-8, half_angle=True):
    """Step 5: the adjoint of rodrigues(): (n,3), (n,3,3) -> (n,3).  K^2 = d d^T - |d|^2 I.  half_angle: 1 - cos a as 2 sin^2(a / 2),
    the kernel's form; False: as written, the form autograd differentiates."""
    aa, gR = np.asarray(aa, np.float64), np.asarray(gR, np.float64)
    out = np.zeros_like(aa)
    for n, (r, G) in enumerate(zip(aa, gR)):
        e = r + eps
        a = np.linalg.norm(e)
        d = r / a
        s, c = np.sin(a), np.cos(a)
        oc = 2.0 * np.sin(0.5 * a) ** 2 if half_angle else 1.0 - c
        w = np.array([G[2, 1] - G[1, 2], G[0, 2] - G[2, 0], G[1, 0] - G[0, 1]])      # sum(G o K(d)) = w . d
        tr = np.trace(G)
        gs = w @ d
        goc = d @ G @ d - (d @ d) * tr                                               # sum(G o K^2)
        gd = s * w + oc * ((G + G.T) @ d - 2.0 * tr * d)
        ga = gs * c + goc * s - (gd @ r) / (a * a)
        out[n] = gd / a + ga * e / a
    return out
