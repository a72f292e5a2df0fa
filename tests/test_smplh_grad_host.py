"""SMPL-H's backward and the tokenizer's reconstruction loss, the part that needs no GPU: the algebra of DESIGN.md 3.5 restated in float64
numpy (tests/smplh_backward_numpy.py, what the kernels are written from) against float64 autograd of smplx's formulation, the 6D adjoint
and the loss kinds likewise, the vertex weights against the reference's loop, and the new entry points in the header."""
import numpy as np
import pytest
import torch

import smplh_backward_numpy as HB
import smplh_oracle as SO

REL = 1e-12          # float64 restatement vs float64 autograd, relative to the largest element (tests/test_smpl_grad_host.py's constant)


@pytest.fixture(scope="module")
def asset():
    from tokenhmr_amd.smpl_assets import make_synthetic_smplh
    return make_synthetic_smplh(seed=0)


def _dup(c):
    c = dict(c)
    ev = c["extra_verts"].clone()
    ev[1], ev[9] = ev[0], ev[4]                # one vertex named by two slots, twice
    c["extra_verts"] = ev
    return c


def _case(B, seed, nj):
    rng = np.random.default_rng(seed + 1)
    R = torch.from_numpy(SO.random_rotations(B * nj, seed=seed).reshape(B, nj, 3, 3))
    return (R, torch.from_numpy(rng.standard_normal((B, 10))), torch.from_numpy(0.3 * rng.standard_normal((B, 3))),
            torch.from_numpy(rng.standard_normal((B, 6890, 3))), torch.from_numpy(rng.standard_normal((B, 73, 3))))


def _autograd64(c, R, betas, transl, gV, gJ, body_only):
    R, betas = R.double().clone().requires_grad_(True), betas.double().clone().requires_grad_(True)
    t = None if transl is None else transl.double().clone().requires_grad_(True)
    v, j = HB.smplh_forward_generic(HB.with_identity_hands(R) if body_only else R, betas, c, t, torch.float64)
    loss = (0 if gV is None else (v * gV).sum()) + (0 if gJ is None else (j * gJ).sum())
    g = torch.autograd.grad(loss, (R, betas) + (() if t is None else (t,)))
    return [x.numpy() for x in g]


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_generic_forward_is_the_fp32_oracle_bit_for_bit(asset):
    R, betas, transl, _, _ = _case(2, 3, 52)
    for t in (None, transl):
        a = SO.smplh_forward_smplx32(R, betas, asset, t)
        b = HB.smplh_forward_generic(R, betas, asset, t, torch.float32)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("dup", [False, True], ids=["plain_ids", "duplicate_ids"])
@pytest.mark.parametrize("body_only", [False, True], ids=["full", "folded"])
def test_backward_algebra_matches_fp64_autograd(asset, body_only, dup):
    c = _dup(asset) if dup else asset
    R, betas, transl, gV, gJ = _case(2, 7, 22 if body_only else 52)
    for arm, (v, j) in {"both": (gV, gJ), "gV": (gV, None), "gJ": (None, gJ)}.items():
        for t in (transl, None):
            want = _autograd64(c, R, betas, t, v, j, body_only)
            got = HB.smplh_backward(R.numpy(), betas.numpy(), None if v is None else v.numpy(), None if j is None else j.numpy(), c, body_only)
            d = [_rel(g, w) for g, w in zip(got, want)]         # grad_transl is compared when transl is present
            print(f"numpy backward vs fp64 autograd ({'folded' if body_only else 'full'}, duplicate ids={dup}, {arm}, transl "
                  f"{'present' if t is not None else 'absent'}): " + ", ".join(f"{x:.1e}" for x in d) + " relative")
            assert max(d) <= REL


def test_folded_hand_joints_reach_the_wrist_and_the_betas(asset):
    """gJ on the hand joints 22..51 alone: on the folded path they exist only as the wrist's transform of their rest position."""
    R, betas, transl, _, gJ = _case(2, 11, 22)
    gJ = gJ.clone()
    gJ[:, :22] = 0
    gJ[:, 52:] = 0
    want = _autograd64(asset, R, betas, transl, None, gJ, True)
    got = HB.smplh_backward(R.numpy(), betas.numpy(), None, gJ.numpy(), asset, True)
    assert np.abs(want[1]).max() > 0
    for g, w in zip(got, want):
        assert _rel(g, w) <= REL


def test_folded_agrees_with_full_at_identity_hands(asset):
    R22, betas, _, gV, gJ = _case(2, 13, 22)
    full = HB.smplh_backward(HB.with_identity_hands(R22).numpy(), betas.numpy(), gV.numpy(), gJ.numpy(), asset, False)
    fold = HB.smplh_backward(R22.numpy(), betas.numpy(), gV.numpy(), gJ.numpy(), asset, True)
    d = (_rel(fold[0], full[0][:, :22]), _rel(fold[1], full[1]), _rel(fold[2], full[2]))
    print("folded vs full with identity hands: grad_pose[:22] %.1e, grad_betas %.1e, grad_transl %.1e relative" % d)
    assert max(d) <= REL


# ------------------------------------------------------------------------------------------------ 6D adjoint
def _x6d():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((40, 6))
    x[1] *= 1e-3
    x[2] *= 1e3
    return x


def test_rot6d_adjoint_matches_fp64_autograd():
    x = _x6d()
    G = np.random.default_rng(6).standard_normal((x.shape[0], 3, 3))
    t = torch.from_numpy(x).clone().requires_grad_(True)
    want, = torch.autograd.grad((HB.rot6d_generic(t) * torch.from_numpy(G)).sum(), t)
    got = HB.rot6d_backward(x, G)
    for n in range(x.shape[0]):                                    # each rotation on its own scale
        assert _rel(got[n], want[n].numpy()) <= REL, n


def test_rot6d_adjoint_below_the_clamp_is_a_division_by_eps():
    x = np.zeros((2, 6))
    x[0, :3], x[0, 3:] = [1e-13, 0, 0], [0.0, 1.0, 0.0]            # |a1| under F.normalize's eps
    x[1, :3], x[1, 3:] = [1.0, 0, 0], [1.0, 0.0, 0.0]              # u = 0 exactly
    G = np.random.default_rng(7).standard_normal((2, 3, 3))
    t = torch.from_numpy(x).clone().requires_grad_(True)
    want, = torch.autograd.grad((HB.rot6d_generic(t) * torch.from_numpy(G)).sum(), t)
    got = HB.rot6d_backward(x, G)
    assert np.isfinite(got).all() and _rel(got, want.numpy()) <= REL


# ------------------------------------------------------------------------------------------------ the loss kinds
@pytest.mark.parametrize("kind", ["l1", "l2", "l1_smooth", "wt_l2"])
def test_loss_kinds_match_fp64_autograd(kind):
    pred, gt = HB.loss_inputs((3, 50, 3), 8)
    w = np.abs(np.random.default_rng(9).standard_normal((50, 3))) if kind == "wt_l2" else None
    val, g = HB.recon_term(kind, pred, gt, w)
    p = torch.from_numpy(pred).double().requires_grad_(True)
    want = HB.torch_term(kind, p, torch.from_numpy(gt).double(), None if w is None else torch.from_numpy(w))
    gw, = torch.autograd.grad(want, p)
    assert abs(val - want.item()) <= REL * abs(want.item()) and _rel(g, gw.numpy()) <= REL
    # the kinks: zero at a zero difference, continuous at |d| = 1; and fp32 torch takes the same branches (no sign flip)
    d = pred.astype(np.float64) - gt
    assert (g[d == 0] == 0).all()
    p32 = torch.from_numpy(pred).requires_grad_(True)
    g32, = torch.autograd.grad(HB.torch_term(kind, p32, torch.from_numpy(gt), None if w is None else torch.from_numpy(w).float()), p32)
    assert (np.sign(g32.numpy()) == np.sign(gw.numpy())).all()


# ------------------------------------------------------------------------------------------------ vertex weights
def test_vertex_weights_equal_the_reference_loop_bit_for_bit(asset):
    from tokenhmr_amd.tokenizer_loss import calculate_vertex_weights
    rng = np.random.default_rng(10)
    verts = rng.standard_normal((60, 3))
    faces = np.stack([rng.permutation(60)[:3] for _ in range(150)])
    a, b = calculate_vertex_weights(verts, faces), HB.vertex_weights_reference_loop(verts, faces)
    assert a.shape == (60, 3) and a.dtype == np.float64 and np.array_equal(a, b)
    with pytest.raises(ValueError, match="degenerate"):
        calculate_vertex_weights(asset["v_template"].numpy(), asset["faces"].numpy())      # the synthetic asset's all-zero topology
    with pytest.raises(ValueError, match="no 'faces'"):
        calculate_vertex_weights(verts, None)
    with pytest.raises(ValueError, match="outside"):
        calculate_vertex_weights(verts, faces + 58)


def test_loss_constructor_refuses_by_name():
    from tokenhmr_amd.tokenizer_loss import PoseReConsLoss
    base = dict(POSE_LOSS="l2", MESH_LOSS="l1", JNT_LOSS="l2", ONLY_VALID_JNT=True)
    for name in ("geodesic", "rotdist"):
        with pytest.raises(NotImplementedError, match=name):
            PoseReConsLoss(dict(base, POSE_LOSS=name), 21, "rotmat", "smplh")
    with pytest.raises(ValueError, match="wt_l2"):
        PoseReConsLoss(dict(base, MESH_LOSS="wt_l2"), 21, "rotmat", "smplh")
    loss = PoseReConsLoss(dict(base, JNT_LOSS="something_else", LOSS_WT=5.0), 21, "rotmat", "smplh")
    assert loss.names == ["l2", "l1", "l2"] and loss.joint_range == (1, 22) and loss.weights == (1.0, 1.0, 1.0, 1.0, 5.0)
    assert PoseReConsLoss(dict(base, ONLY_VALID_JNT=False), 21, "rotmat", "smplh").joint_range == (0, 73)


# ------------------------------------------------------------------------------------------------ header
def test_header_declares_the_new_entry_points():
    from tokenhmr_amd import _cabi
    protos = _cabi.declared_functions()
    assert protos["thmr_smplh_grad_reserve"] == ("int", ["thmr_smplh*", "int32_t"])
    assert protos["thmr_smplh_backward"] == ("int", ["thmr_smplh*", "float*", "int32_t", "float*", "float*", "int32_t", "int32_t", "float*",
                                                      "float*", "float*", "float*", "float*", "void*"])
    assert protos["thmr_op_rot6d_backward"] == ("int", ["float*", "float*", "float*", "int32_t", "void*"])
    assert protos["thmr_tok_recon_loss"] == ("int", ["float*"] * 8 + ["int32_t"] * 5 + ["double"] * 5 + ["int32_t"] + ["float*"] * 5 + ["void*"])
