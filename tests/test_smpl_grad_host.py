"""The body model's backward, the part that needs no GPU: the algebra of DESIGN.md 3.5 restated in float64 numpy
(tests/lbs_backward_numpy.py, what the kernels are written from) against float64 autograd of the oracle's forward, and the three entry
points in the header."""
import numpy as np
import pytest
import torch

import lbs_backward_numpy as LB

REL = 1e-12          # float64 restatement vs float64 autograd, relative to the largest element (measured 3e-15)


def _case(B, seed, hips=False, dup=False):
    from oracle.lbs_independent import random_rotations
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    smpl = make_synthetic_smpl(seed=0)
    smpl["update_hips"] = hips
    if dup:                                    # one vertex named by two slots, as test_gpu_lbs_duplicate_extra_vertex_ids_and_repeated_calls
        ev = smpl["extra_verts"].clone()
        ev[1], ev[9] = ev[0], ev[4]
        smpl["extra_verts"] = ev
    R = torch.from_numpy(random_rotations(B * 24, seed=seed).reshape(B, 24, 3, 3))
    rng = np.random.default_rng(seed + 1)
    betas = torch.from_numpy(rng.standard_normal((B, 10)))
    gV = torch.from_numpy(rng.standard_normal((B, 6890, 3)))
    gJ = torch.from_numpy(rng.standard_normal((B, 44, 3)))
    return smpl, R, betas, gV, gJ


def _autograd64(smpl, R, betas, gV, gJ):
    import stage_bounds as SB
    from oracle import tokenhmr_oracle as O
    s64 = SB.to64(smpl)
    R, betas = R.double().clone().requires_grad_(True), betas.double().clone().requires_grad_(True)
    v, j = O.smpl_forward(R[:, :1], R[:, 1:], betas, s64)
    loss = (0 if gV is None else (v * gV).sum()) + (0 if gJ is None else (j * gJ).sum())
    gR, gb = torch.autograd.grad(loss, (R, betas))
    return gR.numpy(), gb.numpy()


@pytest.mark.parametrize("dup", [False, True], ids=["plain_ids", "duplicate_ids"])
@pytest.mark.parametrize("hips", [False, True], ids=["plain", "update_hips"])
def test_backward_algebra_matches_fp64_autograd(hips, dup):
    smpl, R, betas, gV, gJ = _case(3, 7, hips, dup)
    for arm, (v, j) in {"both": (gV, gJ), "gV": (gV, None), "gJ": (None, gJ)}.items():
        wR, wb = _autograd64(smpl, R, betas, v, j)
        gR, gb = LB.smpl_backward(R.numpy(), betas.numpy(), None if v is None else v.numpy(), None if j is None else j.numpy(), smpl)
        dR, db = np.abs(gR - wR).max() / np.abs(wR).max(), np.abs(gb - wb).max() / np.abs(wb).max()
        print(f"numpy backward vs fp64 autograd (update_hips={hips}, duplicate ids={dup}, {arm}): grad_R {dR:.1e}, grad_betas {db:.1e} relative")
        assert dR <= REL and db <= REL


def _aa_cases():
    rng = np.random.default_rng(3)
    d = rng.standard_normal((6, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([np.zeros((1, 3)), 1e-4 * d[:2], 3.0 * d[2:4], rng.standard_normal((8, 3))])


def test_rodrigues_adjoint_matches_fp64_autograd():
    from oracle import tokenhmr_oracle as O
    aa = _aa_cases()
    G = np.random.default_rng(4).standard_normal((aa.shape[0], 3, 3))
    t = torch.from_numpy(aa).clone().requires_grad_(True)
    Rm = O.batch_rodrigues(t)
    assert np.abs(LB.rodrigues(aa) - Rm.detach().numpy()).max() <= 1e-15
    want, = torch.autograd.grad((Rm * torch.from_numpy(G)).sum(), t)
    # each vector held on its own.  1 - cos as written, the form autograd differentiates: REL.  As 2 sin^2(a / 2), the kernel's form, the
    # difference IS autograd's rounding of 1 - cos a in float64: 2^-53 absolute on a^2 / 2, which enters the gradient as
    # (1 - cos a) / a x ((G + G^T) d - 2 tr(G) d), a term of up to ~8 |G|_max / a x 2^-53 -> REL + 8 x 2^-53 / a (1e-11 at a = 1e-4)
    for half in (False, True):
        got = LB.rodrigues_backward(aa, G, half_angle=half)
        for n in range(aa.shape[0]):
            a = np.linalg.norm(aa[n])
            d = np.abs(got[n] - want[n].numpy()).max() / np.abs(want[n].numpy()).max()
            print(f"rodrigues adjoint (1 - cos as {'2 sin^2(a/2)' if half else 'written'}), |aa| = {a:.1e}: {d:.1e} relative")
            assert d <= REL + (8 * 2.0 ** -53 / a if half and a > 0 else 0.0)


def test_header_declares_the_backward_entry_points():
    from tokenhmr_amd import _cabi
    names = _cabi.declared_symbols()
    for fn in ("thmr_smpl_grad_reserve", "thmr_smpl_backward", "thmr_op_aa_to_rotmat_backward"):
        assert fn in names, fn
    protos = _cabi.declared_functions()
    assert protos["thmr_smpl_backward"] == ("int", ["thmr_smpl*", "float*", "int32_t", "float*", "int32_t", "float*", "float*", "float*",
                                                     "float*", "void*"])
    assert protos["thmr_smpl_grad_reserve"] == ("int", ["thmr_smpl*"])
    assert protos["thmr_op_aa_to_rotmat_backward"] == ("int", ["float*", "float*", "float*", "int32_t", "void*"])
