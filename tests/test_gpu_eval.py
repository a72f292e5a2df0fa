"""Per-kernel parity (-m gpu) of the evaluation metric kernels (csrc/eval.hip: eval_pose_kernel with its fp64 Jacobi Procrustes,
eval_pve_kernel, regress_joints_kernel), called through tokenhmr_amd.evaluator and compared with plain fp64 statements written here.
Three kinds of assertion, named in every test (the convention of test_gpu_rowops.py):

  (E) exact   torch.equal / bit-identical floats.
  (B) bound   derived from the operation, with U = 2^-24 the unit roundoff of fp32:
                MPJPE            |mp - mp64|   <= 16 U mp64          (~3 U per joint distance, 6 levels of the wave sum, a divide, a multiply;
                                                                      every term is non-negative)
                PVE              |pve - pve64| <= (ceil(nv/256) + 16) U pve64     (a serial sum of ceil(nv/256) terms per thread on top)
                regress_joints   |out - out64| <= (ceil(nv/256) + 10) U sum_v |J_jv| |verts_v|     (the dot-product bound), per element
                PA-MPJPE         |re - re64|   <= 2 U re64 + floor   (the one fp32 cast of an fp64 result); floor = 1e-8 mm * max(1, L) with
                                                                      L the largest |coordinate| in metres: fp64 noise under the conditioning
                                                                      allowed below
  (C) class   PA-MPJPE is no further from fp64 than the fp32 oracle (oracle/eval_oracle.py, torch.svd in fp32) is:
              err_hip <= err_oracle + floor, both printed.

The fp64 statements start from the fp32 numbers the kernel holds: the pelvis subtraction (for PVE, (p - pp) - (g - gp) in that order) is done
by torch in fp32 — one IEEE operation per element, no products, so bit-identical to the kernel's — and everything after it is fp64.  The
Procrustes statement is the reference's algorithm (pose_utils.py:76-112) with numpy.linalg.svd in fp64, Z[-1, -1] = sign(det(U Vh)) on the
last (smallest) singular value.

Condition on every Procrustes input (`_statement64` asserts it for every crop of every case): when the fp64 statement has det(U Vh) < 0 the
rotation is defined only if the two smallest singular values differ, so (s1 - s2) / s0 >= 1e-4 is required.  One kind of input cannot have
that gap and still has a defined answer: K of numerical rank <= 1 (s1 / s0 < 1e-12: two keypoints, collinear points), where s1 = s2 = 0 and
the sign of det(U Vh) is rounding noise.  There the centred pred (or gt) lies along u0 (v0) alone, so Z multiplies only zeros.  Such a crop
is not waved through: the statement is evaluated with both signs of Z and the two answers must agree to the floor.

Ground truth is anisotropic — randn * (0.3, 0.2, 0.1) under a random rotation — with fixed seeds chosen so that no crop misses the gap
(the smallest gap among the 70 reflected crops of this file is 2.2e-2).

Observed on the MI355X over the 94 cases (every test prints its own figures; the torch fp32 figures are the CPU's):
  MPJPE            kernel 0.30 ... 2.89 U, torch fp32 0.42 ... 2.89 U                                   (bound 16 U)
  PVE              kernel 0.14 ... 2.41 U, torch fp32 0.05 ... 2.55 U                                   (bound 17 ... 43 U)
  regress_joints   kernel <= 2.43 U, torch fp32 <= 50.5 U (a serial sum; its figure is not asserted)     (bound 11 ... 37 U)
  PA-MPJPE         kernel 2.9e-14 ... 7.4e-6 mm at metre scale (6.1e-3 mm at 1e3), never above 0.44 of its bound and never above the fp32
                   oracle's 7.4e-6 ... 1.1e-4 mm (3.3e-2 mm at 1e3); exact similarity copy: 1.2e-13 mm against a floor of 1.6e-8 mm
The whole file takes 2.9 s there.

"collinear gt on an axis" is the case that found a kernel bug: with two singular values exactly 0 procrustes_rotation completed only one of
the two undefined columns of U, R lost a direction of pred, and PA-MPJPE came out 12 ... 80 mm (1 ... 8 %) too small."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from oracle import eval_oracle as E
from tokenhmr_amd import _cabi
from tokenhmr_amd import evaluator as EV

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32
FLOOR_MM = 1e-8
GAP = 1e-4
RANK1 = 1e-12
NV = [1, 63, 255, 256, 257, 6890]        # one vertex, a partial wave, one short of / exactly / one past the 256-thread stride, SMPL


# ------------------------------------------------------------------------------------------------ inputs
def _rotation(g):
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))
    if torch.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


@functools.lru_cache(maxsize=None)
def _case(B, nj, seed, gt_stride=4, mirror=True):
    """gt: anisotropic cloud under a random rotation, somewhere in the room; pred: a rotated, rescaled, shifted, noisy copy; every odd crop
    mirrored.  fp32 (B,nj,3) and (B,nj,gt_stride) with a confidence column of ones."""
    g = torch.Generator().manual_seed(seed)
    aniso = torch.tensor([0.3, 0.2, 0.1], dtype=torch.float64)
    gt = torch.empty(B, nj, 3, dtype=torch.float64)
    pred = torch.empty(B, nj, 3, dtype=torch.float64)
    for b in range(B):
        gt[b] = (torch.randn(nj, 3, generator=g, dtype=torch.float64) * aniso) @ _rotation(g).T + torch.randn(3, generator=g, dtype=torch.float64)
        pred[b] = 1.1 * (gt[b] @ _rotation(g).T) + 0.03 * torch.randn(nj, 3, generator=g, dtype=torch.float64) + 0.2
    if mirror:
        pred[1::2, :, 0] *= -1
    pred, gt = pred.float(), gt.float()
    if gt_stride == 4:
        gt = torch.cat([gt, torch.ones(B, nj, 1)], -1)
    return pred, gt


def _held(pred, gt, kpl, pelvis_ind, mode):
    """the fp32 numbers eval_pose_kernel holds in shared memory: listed joints minus the pelvis, and the two pelvises"""
    g3 = gt[..., :3]
    if mode == 0:
        pp, gp = pred[:, pelvis_ind], g3[:, pelvis_ind]
    else:
        pp, gp = (pred[:, 1] + pred[:, 2]) / 2.0, (g3[:, 1] + g3[:, 2]) / 2.0
    return pred[:, kpl] - pp[:, None], g3[:, kpl] - gp[:, None], pp, gp


# ------------------------------------------------------------------------------------------------ fp64 statements
def _procrustes64(p, g, flip=False):
    """pose_utils.py:76-112 on one crop in fp64 -> (re_mm, singular values, sign(det(U Vh)))"""
    mu1, mu2 = p.mean(0), g.mean(0)
    x1, x2 = p - mu1, g - mu2
    var1 = (x1 ** 2).sum()
    K = x1.T @ x2
    Uk, s, Vh = np.linalg.svd(K)
    d = np.sign(np.linalg.det(Uk @ Vh))
    Z = np.eye(3)
    Z[-1, -1] *= -d if flip else d
    R = Vh.T @ Z @ Uk.T
    with np.errstate(all="ignore"):
        scale = np.trace(R @ K) / var1
        hat = scale * (p @ R.T) + (mu2 - scale * (R @ mu1))
        return 1000.0 * np.sqrt(((hat - g) ** 2).sum(-1)).mean(), s, d


def _floor(P, G):
    return FLOOR_MM * max(1.0, float(torch.cat([P, G]).abs().max()))


def _statement64(P, G):
    """(mp64, re64, number of reflections, smallest gap among them) per crop, with the condition on Procrustes inputs asserted"""
    P64, G64 = P.double().numpy(), G.double().numpy()
    mp64 = 1000.0 * np.sqrt(((P64 - G64) ** 2).sum(-1)).mean(-1)
    re64, nrefl, mingap = np.empty(len(P64)), 0, math.inf
    for b in range(len(P64)):
        re64[b], s, d = _procrustes64(P64[b], G64[b])
        if d < 0 and s[0] > 0:
            if s[1] < RANK1 * s[0]:          # rank <= 1: Z multiplies zeros only — shown, not assumed
                other = _procrustes64(P64[b], G64[b], flip=True)[0]
                assert abs(other - re64[b]) <= _floor(P[b], G[b]), (b, re64[b], other)
            else:
                gap = (s[1] - s[2]) / s[0]
                assert gap >= GAP, f"crop {b}: reflection with singular values {s}: gap {gap:.1e} < {GAP}; pick another seed"
                nrefl, mingap = nrefl + 1, min(mingap, gap)
    return mp64, re64, nrefl, mingap


def _check_pose(tag, mp, re, P, G, nan_re=False):
    """MPJPE (B), PA-MPJPE (B) and (C) of every crop against the fp64 statement on the held numbers P, G (fp32, on the host)"""
    mp, re = mp.cpu().double().numpy(), re.cpu().double().numpy()
    mp64, re64, nrefl, mingap = _statement64(P, G)
    mp32, re32 = (t.double().numpy() for t in E.eval_pose(P, G))          # the fp32 oracle on the same numbers
    floor = np.array([_floor(P[b], G[b]) for b in range(len(P))])
    e_mp, e_mp32 = np.abs(mp - mp64), np.abs(mp32 - mp64)
    rel = lambda e: float((e / np.maximum(mp64, 1e-300)).max() / U)      # noqa: E731
    print(f"[{tag}] MPJPE |err|/(U mp64): kernel {rel(e_mp):.2f}, torch fp32 {rel(e_mp32):.2f}", end="")
    assert np.isfinite(mp).all() and (e_mp <= 16 * U * mp64).all(), (tag, mp, mp64)                       # (B)
    if nan_re:
        print("; PA-MPJPE NaN as in the reference")
        assert np.isnan(re).all() and np.isnan(re64).all(), (tag, re, re64)
        return
    e_re, e_re32 = np.abs(re - re64), np.abs(re32 - re64)
    e_re32 = np.where(np.isfinite(e_re32), e_re32, np.inf)
    print(f"; PA-MPJPE max|err| mm: kernel {e_re.max():.2e} (bound {(2 * U * re64 + floor).max():.2e}), fp32 oracle {e_re32.max():.2e}; "
          f"re64 {re64.min():.3g}..{re64.max():.3g} mm; {nrefl} reflections" + (f", min gap {mingap:.1e}" if nrefl else ""))
    assert np.isfinite(re).all() and (e_re <= 2 * U * re64 + floor).all(), (tag, re, re64)               # (B)
    assert (e_re <= e_re32 + floor).all(), (tag, e_re, e_re32)                                           # (C)


def _run_pose(tag, pred, gt, kpl, pelvis_ind, mode, dev, **kw):
    mp, re, pve = EV.eval_pose_gpu(pred.to(dev), gt.to(dev), kpl, pelvis_ind, mode)
    assert pve is None
    P, G, _, _ = _held(pred, gt, kpl, pelvis_ind, mode)
    _check_pose(tag, mp, re, P, G, **kw)
    return mp, re


def _pve64(pv, gv, pp, gp):
    d = (pv - pp[:, None]) - (gv - gp[:, None])          # fp32, the kernel's order
    return 1000.0 * d.double().pow(2).sum(-1).sqrt().mean(-1), 1000.0 * d.pow(2).sum(-1).sqrt().mean(-1)


def _check_pve(tag, pve, pv, gv, pp, gp):
    nv = pv.shape[1]
    p64, p32 = _pve64(pv, gv, pp, gp)
    err, err32 = (pve.cpu().double() - p64).abs() / p64, (p32.double() - p64).abs() / p64
    print(f"[{tag}] PVE |err|/(U pve64): kernel {err.max().item() / U:.2f}, torch fp32 {err32.max().item() / U:.2f} (bound {math.ceil(nv / 256) + 16})")
    assert bool(torch.isfinite(pve).all()) and bool((err <= (math.ceil(nv / 256) + 16) * U).all()), (tag, pve, p64)          # (B)


def _check_regress(tag, out, J, verts):
    nv = verts.shape[1]
    out64 = torch.matmul(J.double(), verts.double())
    mag = torch.matmul(J.double().abs(), verts.double().abs())
    out, o32 = out.cpu().double(), torch.matmul(J, verts).double()
    scale = torch.where(mag > 0, mag, torch.ones_like(mag))
    err, err32 = ((out - out64).abs() / scale).max().item() / U, ((o32 - out64).abs() / scale).max().item() / U
    print(f"[{tag}] regress |err|/(U sum|J||v|): kernel {err:.2f}, torch fp32 {err32:.2f} (bound {math.ceil(nv / 256) + 10})")
    assert bool(torch.isfinite(out).all()) and bool(((out - out64).abs() <= (math.ceil(nv / 256) + 10) * U * mag).all()), tag        # (B)


# ------------------------------------------------------------------------------------------------ eval_pose
KP14 = [25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 43]          # the product's 14 of 44 joints
NJ = 70          # more joints than the kernel's 64 lanes, so that 64 distinct keypoints leave joints unlisted


def _kpl(nkp, seed):
    return sorted(torch.randperm(NJ, generator=torch.Generator().manual_seed(seed))[:nkp].tolist())


@pytest.mark.parametrize("gt_stride", [3, 4])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("nkp", [2, 3, 4, 14, 24, 63, 64])
def test_eval_pose_sizes_modes_strides(built_lib, cuda_dev, nkp, mode, gt_stride):
    """MPJPE (B), PA-MPJPE (B) and (C): 2 keypoints (rank 1), 3 (rank 2), 4 (the first full rank), the product's 14 and 24, one short of
    and exactly the 64 lanes; both pelvis rules, both gt layouts; crops 1 and 3 of the 5 mirrored (det < 0)."""
    pred, gt = _case(5, NJ, 100 + nkp, gt_stride)
    _run_pose(f"eval_pose nkp={nkp} mode={mode} stride={gt_stride}", pred, gt, _kpl(nkp, nkp), 39, mode, cuda_dev)


@pytest.mark.parametrize("mode", [0, 1])
def test_eval_pose_reads_only_the_listed_joints(built_lib, cuda_dev, mode):
    """(B)/(C) with NaN in the confidence column and in every joint that is neither listed nor a pelvis joint: all three metrics stay
    finite and within their bounds, so nothing else is read."""
    pred, gt = (t.clone() for t in _case(5, NJ, 7))
    kpl = _kpl(14, 5)
    keep = set(kpl) | ({39} if mode == 0 else {1, 2})
    dead = [j for j in range(NJ) if j not in keep]
    pred[:, dead], gt[:, dead], gt[:, :, 3] = math.nan, math.nan, math.nan
    g = torch.Generator().manual_seed(8)
    pv, gv = torch.randn(5, 63, 3, generator=g), torch.randn(5, 63, 3, generator=g)
    mp, re, pve = EV.eval_pose_gpu(pred.to(cuda_dev), gt.to(cuda_dev), kpl, 39, mode, pv.to(cuda_dev), gv.to(cuda_dev))
    P, G, pp, gp = _held(pred, gt, kpl, 39, mode)
    _check_pose(f"listed joints only, mode={mode}", mp, re, P, G)
    _check_pve(f"listed joints only, mode={mode}", pve, pv, gv, pp, gp)


@pytest.mark.parametrize("name,kpl,pelvis", [("unsorted", [43, 5, 17, 2, 30, 9, 21], 39), ("repeated", [4, 4, 7, 9, 12, 4, 20, 9], 39),
                                             ("pelvis listed", [39, 0, 5, 8, 11, 39], 39), ("pelvis listed, mode 1", [2, 1, 5, 8, 11], 0)])
def test_eval_pose_keypoint_lists(built_lib, cuda_dev, name, kpl, pelvis):
    """(B)/(C) for keypoint lists that are unsorted, repeat an index (a weighted Procrustes) or contain the pelvis joint (a held point that is
    exactly 0, or in mode 1 the two joints the pelvis is the midpoint of)."""
    pred, gt = _case(5, 44, 21)
    _run_pose(f"eval_pose list {name}", pred, gt, kpl, pelvis, 1 if "mode 1" in name else 0, cuda_dev)


def _dyadic(x, bits=10):
    return torch.round(x * 2 ** bits) / 2 ** bits


@functools.lru_cache(maxsize=None)
def _degenerate(name):
    """(pred, gt) (3, n, 3) fp32 with pelvis joint 0; gt_stride 3"""
    pred, gt = (t.clone() for t in _case(3, 12, 31, gt_stride=3))
    g = torch.Generator().manual_seed(32)
    if name == "coplanar pred":          # dyadic x, y and a dyadic plane: z is exact in fp32, so is the plane after the pelvis is subtracted
        pred = _dyadic(pred)
        pred[:, :, 2] = 0.25 * pred[:, :, 0] - 0.5 * pred[:, :, 1] + 0.125
    elif name == "coplanar gt":
        gt = _dyadic(gt)
        gt[:, :, 2] = 0.25 * gt[:, :, 0] - 0.5 * gt[:, :, 1] + 0.125
    elif name == "collinear pred":          # pelvis + (k / 16) * (a dyadic direction): exactly on a line in fp32, K of rank 1 to fp64 rounding
        steps = torch.stack([torch.randperm(64, generator=g)[:12] for _ in range(3)]).float().sub(32.0).div(16.0)
        pred = _dyadic(pred[:, :1]) + steps[:, :, None] * torch.tensor([0.25, -0.125, 0.0625])
    elif name.startswith("collinear gt"):          # the same for gt; "on an axis": two columns of K are exactly 0, two singular values too
        steps = torch.stack([torch.randperm(64, generator=g)[:12] for _ in range(3)]).float().sub(32.0).div(16.0)
        gt = _dyadic(gt[:, :1]) + steps[:, :, None] * torch.tensor([1.0, 0.0, 0.0] if name.endswith("axis") else [0.25, -0.125, 0.0625])
    elif name == "2 keypoints":
        pred, gt = pred[:, :3], gt[:, :3]          # joint 0 is the pelvis, joints 1 and 2 are listed
    elif name == "3 keypoints":
        pred, gt = pred[:, :4], gt[:, :4]
    elif name == "tied singular values":          # cube corners against a rotated, rescaled copy: K = c R, s0 = s1 = s2, det > 0
        cube = torch.tensor([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)]) * 0.25
        rz = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
        gt = torch.cat([torch.zeros(1, 3), cube])[None].repeat(3, 1, 1) + torch.tensor([0.5, -0.25, 2.0])
        pred = torch.stack([torch.cat([torch.zeros(1, 3), cube @ r.T]) for r in (torch.eye(3), rz, rz @ rz)]) * 1.5
        pred = pred + 0.01 * torch.randn(3, 9, 3, generator=g) * torch.tensor([0.0, 1.0, 1.0]).view(3, 1, 1)      # crop 0 exact, 1 and 2 noisy
    elif name == "mirror image":
        pred = gt * torch.tensor([-1.0, 1.0, 1.0])
    elif name == "exact similarity":          # a quarter turn, a factor 2 and a dyadic shift of dyadic points: pred is exact in fp32
        gt = _dyadic(gt)
        pred = 2.0 * torch.stack([-gt[..., 1], gt[..., 0], gt[..., 2]], -1) + torch.tensor([0.5, -1.25, 3.0])
    else:
        raise KeyError(name)
    return pred.contiguous(), gt.contiguous()


@pytest.mark.parametrize("name", ["coplanar pred", "coplanar gt", "collinear pred", "collinear gt", "collinear gt on an axis", "2 keypoints",
                                  "3 keypoints", "tied singular values", "mirror image", "exact similarity"])
def test_eval_pose_rank_deficient_and_tied(built_lib, cuda_dev, name):
    """(B)/(C) where the 3x3 SVD is degenerate: K of rank 2 (coplanar pred or gt, 3 keypoints), of rank 1 (collinear pred, 2 keypoints),
    all singular values tied without a reflection (cube corners: every rotation of the singular vectors is an SVD), a pure mirror image
    of gt (z = -1 with a wide gap), and an exact similarity copy, whose error is 0 and must come out below the floor."""
    pred, gt = _degenerate(name)
    kpl = list(range(1, pred.shape[1]))
    mp, re = _run_pose(f"eval_pose {name}", pred, gt, kpl, 0, 0, cuda_dev)
    if name == "exact similarity":
        assert re.abs().max().item() <= FLOOR_MM * 4.0, re          # L < 4 m here
    if name == "mirror image":
        assert _statement64(*_held(pred, gt, kpl, 0, 0)[:2])[2] == 3          # all three crops reflect


@pytest.mark.parametrize("name", ["one keypoint", "identical pred points"])
def test_eval_pose_zero_variance_is_nan_like_the_reference(built_lib, cuda_dev, name):
    """One keypoint, or pred points that all coincide: var1 = 0 and trace = 0, the reference's scale is 0/0 and its PA-MPJPE NaN.  The
    kernel returns (the call completes), PA-MPJPE is NaN, MPJPE is finite and (B) to its bound."""
    pred, gt = (t.clone() for t in _case(3, 12, 41, gt_stride=3))
    kpl = [5] if name == "one keypoint" else list(range(1, 12))
    if name != "one keypoint":
        pred[:, 1:] = pred[:, 1:2]
    _run_pose(f"eval_pose {name}", pred, gt, kpl, 0, 0, cuda_dev, nan_re=True)


@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
def test_eval_pose_coordinate_scales(built_lib, cuda_dev, scale):
    """(B)/(C) on one case in millimetres-as-metres, metres and kilometres: every bound is relative (the floor grows with L only), so a
    threshold inside the Jacobi loop that is absolute shows here."""
    pred, gt = _case(5, 44, 51)
    gt = torch.cat([gt[..., :3] * scale, gt[..., 3:]], -1)
    _run_pose(f"eval_pose scale={scale:g}", pred * scale, gt, KP14, 39, 0, cuda_dev)


def test_eval_pose_crops_do_not_interact(built_lib, cuda_dev):
    """(E) B = 130 with crop 7 all NaN and crop 64 holding one Inf: every other crop's MPJPE, PA-MPJPE and PVE are bit-identical to that crop
    evaluated alone at B = 1; the poisoned crops are non-finite.  (The Jacobi loop is bounded at 30 sweeps: NaN cannot spin it.)"""
    B, nv = 130, 63
    pred, gt = (t.clone() for t in _case(B, 44, 61))
    g = torch.Generator().manual_seed(62)
    pv, gv = torch.randn(B, nv, 3, generator=g), torch.randn(B, nv, 3, generator=g)
    kpl = KP14
    pred[7], gt[7], pv[7], gv[7] = math.nan, math.nan, math.nan, math.nan
    pred[64, 30, 1] = math.inf
    d = [t.to(cuda_dev) for t in (pred, gt, pv, gv)]
    whole = torch.stack(EV.eval_pose_gpu(d[0], d[1], kpl, 39, 0, d[2], d[3])).cpu()
    alone = torch.cat([torch.stack(EV.eval_pose_gpu(d[0][b:b + 1], d[1][b:b + 1], kpl, 39, 0, d[2][b:b + 1], d[3][b:b + 1])) for b in range(B)], 1).cpu()
    clean = [b for b in range(B) if b not in (7, 64)]
    assert bool(torch.isfinite(whole[:, clean]).all()) and torch.equal(whole[:, clean], alone[:, clean])          # (E)
    assert not torch.isfinite(whole[:, 7]).any() and not torch.isfinite(whole[:2, 64]).any(), (whole[:, 7], whole[:, 64])
    P, G, pp, gp = _held(pred[:5], gt[:5], kpl, 39, 0)
    _check_pose("crops do not interact, crops 0-4", whole[0, :5], whole[1, :5], P, G)


def test_eval_pose_guard_on_out_of_range_keypoints(built_lib, cuda_dev):
    """The kernel's own guard (j < 0 || j >= nj), reached past the Python checks through the C entry point with a keypoint list holding nj
    and -1: MPJPE and PA-MPJPE are NaN for every crop.  pred and gt are views inside larger allocations filled with finite numbers, so a
    wrong guard would read memory this test owns and return finite values."""
    B, nj, pad = 4, 12, 64
    pred, gt = _case(B, nj, 71)
    big_p, big_g = torch.full((pad + B * nj * 3 + pad,), 0.5, device=cuda_dev), torch.full((pad + B * nj * 4 + pad,), 0.25, device=cuda_dev)
    p, g = big_p[pad:pad + B * nj * 3].view(B, nj, 3), big_g[pad:pad + B * nj * 4].view(B, nj, 4)
    p.copy_(pred)
    g.copy_(gt)
    for kpl in ([3, nj, 5, 7], [3, 4, -1, 7], [nj, -1]):
        kp = torch.tensor(kpl, dtype=torch.int32, device=cuda_dev)
        mp, re = torch.zeros(B, device=cuda_dev), torch.zeros(B, device=cuda_dev)
        pelv = torch.zeros(B, 6, device=cuda_dev)
        st = C.c_void_p(torch.cuda.current_stream(cuda_dev).cuda_stream)
        rc = _cabi.load().thmr_eval_pose(EV._p(p), EV._p(g), nj, 4, EV._p(kp), len(kpl), 0, 0, None, None, 0, B, EV._p(mp), EV._p(re), None,
                                        EV._p(pelv), st)
        assert rc == 0
        assert bool(torch.isnan(mp).all()) and bool(torch.isnan(re).all()), (kpl, mp, re)
        assert torch.equal(pelv.cpu(), torch.cat([pred[:, 0], gt[:, 0, :3]], 1))          # (E) the pelvises are still this crop's own
    assert bool((big_p[:pad] == 0.5).all()) and bool((big_p[-pad:] == 0.5).all()) and bool((big_g[:pad] == 0.25).all())


# ------------------------------------------------------------------------------------------------ PVE
@functools.lru_cache(maxsize=None)
def _far(B, n, centre, seed):
    """(pred, gt) clouds of n points 10 m from the origin around `centre`, pred 3 cm of noise and a 10 cm shift from gt"""
    g = torch.Generator().manual_seed(seed)
    gt = torch.tensor(centre) + 0.3 * torch.randn(B, n, 3, generator=g)
    return gt + 0.03 * torch.randn(B, n, 3, generator=g) + 0.1, gt


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nv", NV)
def test_pve(built_lib, cuda_dev, nv, B):
    """PVE (B) in both pelvis modes, with the vertices 10 m from the origin in one direction and the pelvises 10 m in another.  p - pp and
    g - gp are then ~14 m and each rounds at 2^-21 m, against a vertex error of ~4 cm: the fp64 statement keeps the kernel's order
    (p - pp) - (g - gp) in fp32, and a kernel with another order (such as (p - g) - (pp - gp), which is exact here) is ~30 U away.
    (E) asking for PVE changes neither MPJPE nor PA-MPJPE, and not asking (either vertex tensor absent) returns None."""
    pv, gv = _far(B, nv, (6.0, -8.0, 0.5), 80 + nv % 97)
    pred, gt = _far(B, 24, (-8.0, 0.75, 6.0), 81)
    kpl = list(range(24))
    for mode in (0, 1):
        mp, re, pve = EV.eval_pose_gpu(pred.to(cuda_dev), gt.to(cuda_dev), kpl, 0, mode, pv.to(cuda_dev), gv.to(cuda_dev))
        _, _, pp, gp = _held(pred, gt, kpl, 0, mode)
        _check_pve(f"pve nv={nv} B={B} mode={mode}", pve, pv, gv, pp, gp)
        mp0, re0, none = EV.eval_pose_gpu(pred.to(cuda_dev), gt.to(cuda_dev), kpl, 0, mode)
        assert none is None and torch.equal(mp0, mp) and torch.equal(re0, re)          # (E)
        mp1, re1, none = EV.eval_pose_gpu(pred.to(cuda_dev), gt.to(cuda_dev), kpl, 0, mode, pv.to(cuda_dev), None)
        assert none is None and torch.equal(mp1, mp) and torch.equal(re1, re)


# ------------------------------------------------------------------------------------------------ regress_joints
def _J(kind, nj, nv, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "softmax":
        return torch.softmax(2.0 * torch.randn(nj, nv, generator=g), -1)
    if kind == "signed":          # rows that sum to ~0 against vertices with a common offset: the result is far smaller than its terms
        J = torch.randn(nj, nv, generator=g)
        return J - J.mean(-1, keepdim=True)
    if kind == "one-hot":
        J = torch.zeros(nj, nv)
        J[torch.arange(nj), (torch.arange(nj) * 97 + nv - 1) % nv] = 1.0          # row 0 picks the last vertex
        return J
    if kind == "zero":
        return torch.zeros(nj, nv)
    # mixed: the one-hot row, the zero row, softmax rows, signed rows
    J = torch.cat([_J("one-hot", 1, nv, seed), _J("zero", 1, nv, seed), _J("softmax", (nj - 2) // 2, nv, seed),
                   _J("signed", nj - 2 - (nj - 2) // 2, nv, seed)])
    return J


@pytest.mark.parametrize("nj,kind", [(1, "softmax"), (1, "signed"), (1, "one-hot"), (1, "zero"), (24, "mixed")])
@pytest.mark.parametrize("nv", NV)
def test_regress_joints(built_lib, cuda_dev, nv, nj, kind):
    """regress_joints (B) per element; (E) a one-hot row returns that vertex bit-exactly and an all-zero row returns exactly 0."""
    J = _J(kind, nj, nv, 90 + nv % 89)
    g = torch.Generator().manual_seed(91)
    verts = torch.randn(2, nv, 3, generator=g) + torch.tensor([5.0, -3.0, 0.0])
    out = EV.regress_joints_gpu(J.to(cuda_dev), verts.to(cuda_dev))
    assert out.shape == (2, nj, 3) and out.dtype == torch.float32
    _check_regress(f"regress nv={nv} nj={nj} {kind}", out, J, verts)
    out = out.cpu()
    if kind in ("one-hot", "mixed"):
        assert torch.equal(out[:, 0], verts[:, nv - 1])          # (E)
    if kind == "one-hot":
        assert torch.equal(out, verts[:, (torch.arange(nj) * 97 + nv - 1) % nv])
    if kind == "zero":
        assert torch.equal(out, torch.zeros(2, nj, 3))          # (E)
    if kind == "mixed":
        assert torch.equal(out[:, 1], torch.zeros(2, 3))


def test_emdb_path_end_to_end(built_lib, cuda_dev):
    """Evaluator(dataset="EMDB") at the smallest size that strides (nv = 257, 24 joints, B = 3, crop 1 mirrored): regress_joints (B) against
    fp64; then MPJPE (B), PA-MPJPE (B)/(C) and PVE (B) of the evaluator's arrays against the fp64 statements on the joints the regress
    kernel produced, with pelvis mode 1."""
    B, nv = 3, 257
    J = _J("softmax", 24, nv, 95)
    g = torch.Generator().manual_seed(96)
    aniso = torch.tensor([0.3, 0.2, 0.1], dtype=torch.float64)
    gv = torch.stack([(torch.randn(nv, 3, generator=g, dtype=torch.float64) * aniso * 3.0) @ _rotation(g).T + 2.0 for _ in range(B)])
    pv = torch.stack([1.05 * (gv[b] @ _rotation(g).T) + 0.03 * torch.randn(nv, 3, generator=g, dtype=torch.float64) for b in range(B)])
    pv[1, :, 0] *= -1
    gv, pv = gv.float(), pv.float()
    ev = EV.Evaluator(10, list(range(24)), 39, metrics=["mode_re", "mode_mpjpe", "mode_pve"], J_regressor_24_SMPL=J.to(cuda_dev), dataset="EMDB")
    r = ev({"pred_vertices": pv.to(cuda_dev)}, {"imgname": ["x"] * B, "vertices": gv.to(cuda_dev)})
    pj, gj = EV.regress_joints_gpu(J.to(cuda_dev), pv.to(cuda_dev)).cpu(), EV.regress_joints_gpu(J.to(cuda_dev), gv.to(cuda_dev)).cpu()
    _check_regress("EMDB regress pred", pj, J, pv)
    _check_regress("EMDB regress gt", gj, J, gv)
    P, G, pp, gp = _held(pj, gj, list(range(24)), 0, 1)
    f32 = lambda a: torch.from_numpy(np.asarray(a)).float()          # noqa: E731  (the arrays hold the kernel's fp32 values, widened)
    _check_pose("EMDB end to end", f32(r["mode_mpjpe"]), f32(r["mode_re"]), P, G)
    _check_pve("EMDB end to end", f32(r["mode_pve"]), pv, gv, pp, gp)
    assert ev.counter == B and np.array_equal(ev.mode_re[:B], r["mode_re"])
