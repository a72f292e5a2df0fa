"""Edge sets, float64 truths, the per-group rule and fp32 numpy restatements for the rotation kernels (tests/test_rotation_cases_host.py on
the CPU, tests/test_gpu_rotation_edges.py on the device).  A plain module: no fixtures, no pytest hooks, numpy and torch only.

Every group has GROUP = 64 rows, so a group's bound is the largest of 64 draws; the groups are concatenated, so one call crosses the
256-thread workgroup boundary several times with groups straddling it.  `aa_set` and `rot6d_set` return (tensor, spans) with
spans[name] = [lo, hi], the shape of scripts/gen_golden_tokenizer_rt.py::rotation_set.

The rule is tests/stage_bounds.py's, applied PER GROUP: the device may be MULT x as far from float64 as the oracle in fp32 is on the same
rows, and never needs to be closer than 4 ulp of that group's largest element.  One bound over the whole tensor would let a group of
|aa| = 1e-4 rows be wrong in every digit beside O(1) rows.

Two groups are checked by properties only (PROPERTY_ONLY): `a2_eq_2a1` (u = a2 - (b1 . a2) b1 is pure rounding there, so fp32 and fp64 pick
unrelated directions for b2 and the reference's own distance is O(1)) and `nan_row` (theta + 1e-8 is exactly zero in fp32, the reference
returns NaN)."""
import math

import numpy as np
import torch

import stage_bounds as SB

GROUP = 64
LEAD = 37                                              # ordinary rows in front of the first group
SEED_AA, SEED_6D, SEED_GRAD = 20241, 20242, 20243      # the seeds BOTH test files use
MULT = 2.0                                             # the project's rule

AA_GROUPS = ("zero", "n1e-9", "n1e-8", "n1e-7", "n1e-6", "n1e-4", "n1e-2", "randn0.8", "pi", "2pi", "4pi", "one_axis")
R6_GROUPS = ("randn", "x1e-3", "x1e3", "x1e-10", "x1e10", "collinear1e-2", "collinear1e-4", "a1_zero", "a2_zero", "all_zero",
             "a1_1e-13", "axis_aligned", "a2_eq_2a1")
PROPERTY_ONLY = ("a2_eq_2a1", "nan_row")
CLAMP_GROUPS = ("a1_zero", "a2_zero", "all_zero", "a1_1e-13")
# per-group multipliers above MULT, each with its arithmetic reason beside it (never above stage_bounds.MULT_MAX); operator -> group -> mult
MULT_OF = {}

# theta + 1e-8 == 0 exactly in fp32: angle = 0, theta / angle = -inf, sin(0) * -inf = NaN
NAN_ROW = np.full(3, -1e-8, dtype=np.float32)


def mult_of(op, group):
    m = MULT_OF.get(op, {}).get(group, MULT)
    assert m <= SB.MULT_MAX
    return m


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def aa_set(seed=SEED_AA):
    """(37 + 12 * 64, 3) fp32 axis-angle rows and their spans."""
    rng = np.random.default_rng(seed)
    parts = {"zero": np.zeros((GROUP, 3))}
    for name in ("n1e-9", "n1e-8", "n1e-7", "n1e-6", "n1e-4", "n1e-2"):
        parts[name] = float(name[1:]) * _unit(rng, GROUP)
    parts["randn0.8"] = 0.8 * rng.standard_normal((GROUP, 3))
    for name, k in (("pi", 1), ("2pi", 2), ("4pi", 4)):            # |aa| = k pi - 1e-3 (even rows) and + 1e-3 (odd rows)
        r = k * math.pi + np.where(np.arange(GROUP) % 2 == 0, -1e-3, 1e-3)
        parts[name] = r[:, None] * _unit(rng, GROUP)
    one = np.zeros((GROUP, 3))                                      # about one coordinate axis, angle from -3 to 3
    one[np.arange(GROUP), np.arange(GROUP) % 3] = np.linspace(-3.0, 3.0, GROUP)
    parts["one_axis"] = one
    return _cat(parts, AA_GROUPS, 0.8 * rng.standard_normal((LEAD, 3)))


def rot6d_set(seed=SEED_6D):
    """(37 + 13 * 64, 6) fp32 6D rows (a1 = columns 0..2, a2 = 3..5) and their spans."""
    rng = np.random.default_rng(seed)
    parts = {"randn": rng.standard_normal((GROUP, 6))}
    for name in ("x1e-3", "x1e3", "x1e-10", "x1e10"):
        parts[name] = float(name[1:]) * rng.standard_normal((GROUP, 6))
    for name, eps in (("collinear1e-2", 1e-2), ("collinear1e-4", 1e-4)):       # a2 = 1.7 a1 + eps |a1| p, p a unit vector normal to a1
        a1 = rng.standard_normal((GROUP, 3))
        p = np.cross(a1, _unit(rng, GROUP))
        p /= np.linalg.norm(p, axis=1, keepdims=True)
        parts[name] = np.concatenate([a1, 1.7 * a1 + eps * np.linalg.norm(a1, axis=1, keepdims=True) * p], axis=1)
    z = np.zeros((GROUP, 3))
    parts["a1_zero"] = np.concatenate([z, rng.standard_normal((GROUP, 3))], axis=1)
    parts["a2_zero"] = np.concatenate([rng.standard_normal((GROUP, 3)), z], axis=1)
    parts["all_zero"] = np.zeros((GROUP, 6))
    parts["a1_1e-13"] = np.concatenate([1e-13 * _unit(rng, GROUP), rng.standard_normal((GROUP, 3))], axis=1)      # under F.normalize's eps
    parts["axis_aligned"] = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0]), (GROUP, 1))
    a1 = rng.standard_normal((GROUP, 3)).astype(np.float32)
    parts["a2_eq_2a1"] = np.concatenate([a1, 2.0 * a1], axis=1)                 # exact in fp32
    return _cat(parts, R6_GROUPS, rng.standard_normal((LEAD, 6)))


def _cat(parts, order, lead):
    """LEAD ordinary rows in front (in no group), so that the 64-row groups straddle the 256-thread workgroup boundaries."""
    spans, lo = {}, LEAD
    for name in order:
        assert parts[name].shape[0] == GROUP
        spans[name] = [lo, lo + GROUP]
        lo += GROUP
    return torch.from_numpy(np.concatenate([lead] + [parts[n] for n in order], axis=0).astype(np.float32)), spans


def nan_rows(seed=SEED_AA):
    """The NaN row between two ordinary rows: (3, 3) fp32."""
    rng = np.random.default_rng(seed + 7)
    t = (0.8 * rng.standard_normal((3, 3))).astype(np.float32)
    t[1] = NAN_ROW
    return torch.from_numpy(t)


def grad_out(n, seed=SEED_GRAD):
    """The incoming gradient of a backward check: (n, 3, 3) fp32, N(0, 1)."""
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n, 3, 3)).astype(np.float32))


def compared(spans):
    return [g for g in spans if g not in PROPERTY_ONLY]


# ------------------------------------------------------------------------------------------------ truths (the oracle, either precision)
def fwd(fn, x, dtype):
    with torch.no_grad():
        return fn(x.to(dtype))


def vjp(fn, x, gR, dtype):
    """autograd of sum(fn(x) * gR) by x in `dtype`."""
    t = x.to(dtype).clone().requires_grad_(True)
    return torch.autograd.grad((fn(t) * gR.to(dtype)).sum(), t)[0]


def tighter(cands, truth64, lo, hi):
    """Of several fp32 references {name: tensor}, the one closest to the truth on rows lo..hi: (name, tensor)."""
    name = min(cands, key=lambda k: SB.dist(cands[k][lo:hi], truth64[lo:hi]))
    return name, cands[name]


# ------------------------------------------------------------------------------------------------ the per-group rule
def ratio(dev, ref32, ref64):
    d, own = SB.dist(dev, ref64), SB.dist(ref32, ref64)
    return d / own if own > 0 else (0.0 if d == 0 else float("inf"))


def check_groups(op, dev, ref32, ref64, spans, groups=None, fails=None, table=None, keep=None):
    """stage_bounds.check on each group's rows (of them, those where the mask `keep` holds); ref32 may be a dict group -> tensor (the tighter
    reference per group).  Appends the failing lines to `fails` and (group, device distance, reference's own, ratio, bound) to `table`;
    returns the fails."""
    fails = [] if fails is None else fails
    for g in (compared(spans) if groups is None else groups):
        lo, hi = spans[g]
        sel = torch.arange(lo, hi)
        if keep is not None:
            sel = sel[keep[lo:hi]]
        r32 = ref32[g] if isinstance(ref32, dict) else ref32
        m = mult_of(op, g)
        ok, line = SB.check(f"{op} [{g}, {sel.numel()} rows]", dev[sel], r32[sel], ref64[sel], m)
        if table is not None:
            table.append((g, SB.dist(dev[sel], ref64[sel]), SB.dist(r32[sel], ref64[sel]), ratio(dev[sel], r32[sel], ref64[sel]),
                          SB.bound(r32[sel], ref64[sel], m)))
        if not ok:
            fails.append(line)
    return fails


# ------------------------------------------------------------------------------------------------ fp32 numpy restatements (host test only)
# Operation by operation as the kernels are written, every intermediate rounded to fp32; WITHOUT the compiler's contraction into fma and
# with numpy's sinf / cosf in place of the device library's.
F32 = np.float32


def _cols(a):
    a = np.asarray(a, F32)
    return a[:, 0], a[:, 1], a[:, 2]


def aa_to_rotmat_kernel_np(aa):
    """aa_to_rotmat_kernel (csrc/head.hip) == aa_to_rotmat_dev (csrc/rotation_device.h)."""
    with np.errstate(all="ignore"):
        tx, ty, tz = _cols(aa)
        e = F32(1e-8)
        ex, ey, ez = tx + e, ty + e, tz + e
        angle = np.sqrt(ex * ex + ey * ey + ez * ez)
        nx, ny, nz = tx / angle, ty / angle, tz / angle
        half = angle * F32(0.5)
        qw, sn = np.cos(half), np.sin(half)
        qx, qy, qz = sn * nx, sn * ny, sn * nz
        qn = np.sqrt(qw * qw + qx * qx + qy * qy + qz * qz)
        w, x, y, z = qw / qn, qx / qn, qy / qn, qz / qn
        w2, x2, y2, z2 = w * w, x * x, y * y, z * z
        wx, wy, wz, xy, xz, yz = w * x, w * y, w * z, x * y, x * z, y * z
        two = F32(2)
        R = np.stack([w2 + x2 - y2 - z2, two * xy - two * wz, two * wy + two * xz,
                      two * wz + two * xy, w2 - x2 + y2 - z2, two * yz - two * wx,
                      two * xz - two * wy, two * wx + two * yz, w2 - x2 - y2 + z2], axis=1)
    assert R.dtype == F32
    return R.reshape(-1, 3, 3)


def rodrigues_kernel_np(aa):
    """rodrigues_kernel (csrc/body_model.hip)."""
    with np.errstate(all="ignore"):
        x, y, z = _cols(aa)
        e = F32(1e-8)
        ex, ey, ez = x + e, y + e, z + e
        angle = np.sqrt(ex * ex + ey * ey + ez * ez)
        rx, ry, rz = x / angle, y / angle, z / angle
        s, c = np.sin(angle), np.cos(angle)
        oc = F32(1) - c
        zero, one = np.zeros_like(x), np.ones_like(x)
        k2 = [-(rz * rz) - ry * ry, rx * ry, rx * rz, rx * ry, -(rz * rz) - rx * rx, ry * rz, rx * rz, ry * rz, -(ry * ry) - rx * rx]
        k1 = [zero, -rz, ry, rz, zero, -rx, -ry, rx, zero]
        R = np.stack([(one if i in (0, 4, 8) else zero) + s * k1[i] + oc * k2[i] for i in range(9)], axis=1)
    assert R.dtype == F32
    return R.reshape(-1, 3, 3)


def rodrigues_backward_kernel_np(aa, gR, mistake=None):
    """rodrigues_backward_kernel (csrc/body_model.hip).  mistake "one_minus_cos": 1 - cos a in place of 2 sin^2(a / 2); "x_over_a": x / a in
    place of ex / a in the last line; "no_epsilon": the + 1e-8 dropped."""
    with np.errstate(all="ignore"):
        x, y, z = _cols(aa)
        G = np.asarray(gR, F32).reshape(-1, 9)
        e = F32(0 if mistake == "no_epsilon" else 1e-8)
        ex, ey, ez = x + e, y + e, z + e
        a = np.sqrt(ex * ex + ey * ey + ez * ez)
        dx, dy, dz = x / a, y / a, z / a
        s, c, sh = np.sin(a), np.cos(a), np.sin(F32(0.5) * a)
        oc = (F32(1) - c) if mistake == "one_minus_cos" else F32(2) * sh * sh
        g00, g01, g02, g10, g11, g12, g20, g21, g22 = (G[:, i] for i in range(9))
        wx, wy, wz = g21 - g12, g02 - g20, g10 - g01
        tr = g00 + g11 + g22
        sx = (g00 + g00) * dx + (g01 + g10) * dy + (g02 + g20) * dz
        sy = (g10 + g01) * dx + (g11 + g11) * dy + (g12 + g21) * dz
        sz = (g20 + g02) * dx + (g21 + g12) * dy + (g22 + g22) * dz
        dd = dx * dx + dy * dy + dz * dz
        gs = wx * dx + wy * dy + wz * dz
        goc = F32(0.5) * (sx * dx + sy * dy + sz * dz) - dd * tr
        two = F32(2)
        gdx, gdy, gdz = s * wx + oc * (sx - two * tr * dx), s * wy + oc * (sy - two * tr * dy), s * wz + oc * (sz - two * tr * dz)
        ga = (gs * c + goc * s) - (gdx * x + gdy * y + gdz * z) / (a * a)
        lx, ly, lz = (x, y, z) if mistake == "x_over_a" else (ex, ey, ez)
        out = np.stack([gdx / a + ga * (lx / a), gdy / a + ga * (ly / a), gdz / a + ga * (lz / a)], axis=1)
    assert out.dtype == F32
    return out


def rot6d_kernel_np(x):
    """rot6d_kernel (csrc/head.hip) == assemble_kernel's inline step."""
    with np.errstate(all="ignore"):
        x = np.asarray(x, F32)
        a1x, a1y, a1z, a2x, a2y, a2z = (x[:, i] for i in range(6))
        eps = F32(1e-12)
        n1 = np.maximum(np.sqrt(a1x * a1x + a1y * a1y + a1z * a1z), eps)
        b1x, b1y, b1z = a1x / n1, a1y / n1, a1z / n1
        dp = b1x * a2x + b1y * a2y + b1z * a2z
        ux, uy, uz = a2x - dp * b1x, a2y - dp * b1y, a2z - dp * b1z
        n2 = np.maximum(np.sqrt(ux * ux + uy * uy + uz * uz), eps)
        b2x, b2y, b2z = ux / n2, uy / n2, uz / n2
        R = np.stack([b1x, b1y, b1z, b2x, b2y, b2z,
                      b1y * b2z - b1z * b2y, b1z * b2x - b1x * b2z, b1x * b2y - b1y * b2x], axis=1)
    assert R.dtype == F32
    return R.reshape(-1, 3, 3)


def rot6d_backward_np(x, gR, dtype=np.float64):
    """rot6d_backward_kernel's steps (tests/smplh_backward_numpy.py::rot6d_backward, vectorised) in `dtype`, rounded to fp32 at the end.
    float64 is the kernel; float32 is the planted mistake of tests/test_rotation_cases_host.py."""
    with np.errstate(all="ignore"):
        x, gR = np.asarray(x, F32).astype(dtype), np.asarray(gR, F32).astype(dtype)
        eps = dtype(1e-12)
        dot = lambda p, q: (p * q).sum(axis=1, keepdims=True)      # noqa: E731
        a1, a2 = x[:, :3], x[:, 3:]
        l1 = np.sqrt(dot(a1, a1))
        n1 = np.maximum(l1, eps)
        b1 = a1 / n1
        dp = dot(b1, a2)
        u = a2 - dp * b1
        l2 = np.sqrt(dot(u, u))
        n2 = np.maximum(l2, eps)
        b2 = u / n2
        g1, g2, g3 = gR[:, 0], gR[:, 1], gR[:, 2]
        gb1 = g1 + np.cross(b2, g3)
        gb2 = g2 + np.cross(g3, b1)
        gu = (gb2 - b2 * np.where(l2 >= eps, dot(b2, gb2), 0)) / n2
        gdp = -dot(gu, b1)
        gb1 = gb1 + gdp * a2 - dp * gu
        out = np.concatenate([(gb1 - b1 * np.where(l1 >= eps, dot(b1, gb1), 0)) / n1, gu + gdp * b1], axis=1)
    assert out.dtype == dtype
    return out.astype(F32)
