"""The conditions tests/test_gpu_rotation_edges.py rests on, on the CPU, for exactly the seeds that file uses (tests/rotation_cases.py): the
reference is finite and meaningful in every compared group, the property-only groups are exactly the two that are spelled out, the two
float64 truths of the axis-angle backward agree, the fp32 numpy restatements of the kernels pass the per-group rule, three planted
mistakes do not, and the oracle's functions equal the reference's own where the reference tree exists."""
import numpy as np
import pytest
import torch

import rotation_cases as RC
import smplh_backward_numpy as S
import stage_bounds as SB
from oracle import tokenhmr_oracle as O

MEANINGFUL = 1e-2          # the reference's own fp32-to-fp64 distance over the group's largest fp64 element: a condition, not a measurement
TRUTHS_AGREE = 1e-7


@pytest.fixture(scope="module")
def aa():
    x, spans = RC.aa_set()
    gR = RC.grad_out(x.shape[0])
    t = {"x": x, "spans": spans, "gR": gR}
    for name, fn in (("quat", O.aa_to_rotmat), ("rod", O.batch_rodrigues)):
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            t[f"{name}.fwd{tag}"], t[f"{name}.bwd{tag}"] = RC.fwd(fn, x, dt), RC.vjp(fn, x, gR, dt)
    return t


@pytest.fixture(scope="module")
def r6():
    x, spans = RC.rot6d_set()
    gR = RC.grad_out(x.shape[0], RC.SEED_GRAD + 1)
    t = {"x": x, "spans": spans, "gR": gR}
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        t[f"fwd{tag}"], t[f"bwd{tag}"] = RC.fwd(O.rot6d_to_rotmat, x, dt), RC.vjp(O.rot6d_to_rotmat, x, gR, dt)
    return t


def _own(r32, r64, lo, hi):
    return SB.dist(r32[lo:hi], r64[lo:hi]), r64[lo:hi].abs().max().item()


def test_the_sets_are_what_the_module_says(aa, r6):
    assert tuple(aa["spans"]) == RC.AA_GROUPS and tuple(r6["spans"]) == RC.R6_GROUPS
    assert aa["x"].shape == (RC.LEAD + len(RC.AA_GROUPS) * RC.GROUP, 3) and r6["x"].shape == (RC.LEAD + len(RC.R6_GROUPS) * RC.GROUP, 6)
    assert aa["x"].dtype == torch.float32 and r6["x"].dtype == torch.float32
    for (x, spans), again in (((aa["x"], aa["spans"]), RC.aa_set()), ((r6["x"], r6["spans"]), RC.rot6d_set())):
        assert torch.equal(x, again[0]) and spans == again[1]                      # deterministic from the seed
        assert any(lo < k * 256 < hi for lo, hi in spans.values() for k in (1, 2, 3))     # a group straddles a workgroup boundary
    n = aa["x"].double().norm(dim=1)
    for g, want in (("n1e-9", 1e-9), ("n1e-4", 1e-4), ("n1e-2", 1e-2)):
        lo, hi = aa["spans"][g]
        assert torch.allclose(n[lo:hi], torch.full((RC.GROUP,), want, dtype=torch.float64), rtol=1e-6, atol=0)
    for g, k in (("pi", 1), ("2pi", 2), ("4pi", 4)):
        lo, hi = aa["spans"][g]
        assert ((n[lo:hi] - k * np.pi).abs() - 1e-3).abs().max() < 1e-5
    lo, hi = aa["spans"]["zero"]
    assert not aa["x"][lo:hi].any()
    lo, hi = r6["spans"]["a2_eq_2a1"]
    assert torch.equal(r6["x"][lo:hi, 3:], 2 * r6["x"][lo:hi, :3])
    lo, hi = r6["spans"]["a1_1e-13"]
    assert (r6["x"][lo:hi, :3].double().norm(dim=1) < 1e-12).all() and r6["x"][lo:hi, :3].any(dim=1).all()
    for name, eps in (("collinear1e-2", 1e-2), ("collinear1e-4", 1e-4)):           # the angle between a1 and a2 is eps / 1.7, in the fp32 bits
        lo, hi = r6["spans"][name]
        a1, a2 = r6["x"][lo:hi, :3].double(), r6["x"][lo:hi, 3:].double()
        sin = torch.cross(a1, a2, dim=1).norm(dim=1) / (a1.norm(dim=1) * a2.norm(dim=1))
        assert ((sin * 1.7 / eps - 1).abs() < 2e-2).all(), (sin * 1.7 / eps - 1).abs().max()


def test_reference_finite_and_meaningful_and_the_property_only_groups_are_exactly_two(aa, r6):
    not_compared = []
    print()
    for op, t, keys in (("aa_to_rotmat", aa, ("quat.fwd", "quat.bwd", "rod.fwd", "rod.bwd")), ("rot6d", r6, ("fwd", "bwd"))):
        for g, (lo, hi) in t["spans"].items():
            bad = False
            for k in keys:
                r32, r64 = t[k + "32"], t[k + "64"]
                finite = bool(torch.isfinite(r32[lo:hi]).all() and torch.isfinite(r64[lo:hi]).all())
                own, big = _own(r32, r64, lo, hi)
                print(f"{op} [{g}] {k}: finite {finite}, reference's own fp32 {own:.3e}, max|value| {big:.3g}, own / max {own / big if big else 0:.2e}")
                if k == "rod.bwd":       # the backward is held to the TIGHTER form; the Rodrigues form in fp32 only has to be finite
                    bad |= not finite
                else:
                    bad |= not (finite and own <= MEANINGFUL * big)
            if bad:
                not_compared.append(g)
    # the NaN row
    rows = RC.nan_rows()
    gR = RC.grad_out(3, RC.SEED_GRAD + 2)
    for fn in (O.aa_to_rotmat, O.batch_rodrigues):
        f32, b32 = RC.fwd(fn, rows, torch.float32), RC.vjp(fn, rows, gR, torch.float32)
        assert torch.isnan(f32[1]).all() and torch.isnan(b32[1]).all(), fn.__name__
        assert torch.isfinite(f32[[0, 2]]).all() and torch.isfinite(b32[[0, 2]]).all()
        # in float64 the row is NaN where it IS -1e-8 (the double literal); the fp32 bits widened are -9.99999993922529e-09, theta + 1e-8
        # is 6.1e-17 there and the float64 run is finite: the record below is the fp32 reference's
        lit = torch.full((1, 3), -1e-8, dtype=torch.float64)
        assert torch.isnan(RC.fwd(fn, lit, torch.float64)).all() and torch.isnan(RC.vjp(fn, lit, gR[1:2], torch.float64)).all()
        wide = RC.fwd(fn, rows[1:2], torch.float64)
        print(f"{fn.__name__}: NaN row in fp32: 9 of 9 and 3 of 3 NaN; float64 on the double literal: NaN; float64 on the widened fp32 bits: "
              f"finite {bool(torch.isfinite(wide).all())}")
    not_compared.append("nan_row")
    assert tuple(not_compared) == RC.PROPERTY_ONLY, not_compared
    assert set(RC.compared(r6["spans"])) | {"a2_eq_2a1"} == set(RC.R6_GROUPS) and RC.compared(aa["spans"]) == list(RC.AA_GROUPS)


def test_both_truths_of_the_axis_angle_backward_agree(aa):
    print()
    for g, (lo, hi) in aa["spans"].items():
        d = SB.dist(aa["quat.bwd64"][lo:hi], aa["rod.bwd64"][lo:hi])
        q, r = SB.dist(aa["quat.bwd32"][lo:hi], aa["quat.bwd64"][lo:hi]), SB.dist(aa["rod.bwd32"][lo:hi], aa["quat.bwd64"][lo:hi])
        name, _ = RC.tighter({"quat": aa["quat.bwd32"], "rod": aa["rod.bwd32"]}, aa["quat.bwd64"], lo, hi)
        print(f"aa backward [{g}]: the two float64 truths differ by {d:.2e}; fp32 distance to float64: quaternion form {q:.3e}, "
              f"Rodrigues form {r:.3e} (x{r / q if q else float('inf'):.1f}); tighter: {name}")
        assert d < TRUTHS_AGREE, (g, d)
    d = SB.dist(aa["quat.fwd64"], aa["rod.fwd64"])
    print(f"forward: the two float64 forms differ by {d:.2e}")
    assert d < TRUTHS_AGREE


def _aa_ref32(aa):
    return {g: RC.tighter({"quat": aa["quat.bwd32"], "rod": aa["rod.bwd32"]}, aa["quat.bwd64"], lo, hi)[1] for g, (lo, hi) in aa["spans"].items()}


def _table(title, table):
    print(f"\n{title}\n  group            restatement   reference's own   ratio   bound")
    for g, d, own, r, b in table:
        print(f"  {g:<16} {d:.3e}     {own:.3e}         {r:5.2f}   {b:.3e}")


def test_restatements_pass_the_per_group_rule(aa, r6):
    x, gR = aa["x"].numpy(), aa["gR"].numpy()
    fails = []
    for title, op, dev, r32, r64, spans in (
            ("aa_to_rotmat_kernel", "aa_to_rotmat", RC.aa_to_rotmat_kernel_np(x), aa["quat.fwd32"], aa["quat.fwd64"], aa["spans"]),
            ("rodrigues_kernel", "rodrigues", RC.rodrigues_kernel_np(x), aa["rod.fwd32"], aa["rod.fwd64"], aa["spans"]),
            ("rodrigues_backward_kernel", "aa_to_rotmat_backward", RC.rodrigues_backward_kernel_np(x, gR), _aa_ref32(aa), aa["quat.bwd64"], aa["spans"]),
            ("rot6d_kernel", "rot6d", RC.rot6d_kernel_np(r6["x"].numpy()), r6["fwd32"], r6["fwd64"], r6["spans"]),
            ("rot6d_backward_kernel", "rot6d_backward", S.rot6d_backward(r6["x"].numpy(), r6["gR"].numpy()).astype(np.float32), r6["bwd32"],
             r6["bwd64"], r6["spans"])):
        table = []
        RC.check_groups(op, torch.from_numpy(dev), r32, r64, spans, fails=fails, table=table)
        _table(f"{title} (fp32 numpy restatement, no contraction, numpy's sinf / cosf)", table)
    # the vectorised restatement of the 6D adjoint is the looped one of tests/smplh_backward_numpy.py
    a, b = RC.rot6d_backward_np(r6["x"].numpy(), r6["gR"].numpy()), S.rot6d_backward(r6["x"].numpy(), r6["gR"].numpy()).astype(np.float32)
    lo, hi = r6["spans"]["a2_eq_2a1"]
    keep = np.r_[0:lo, hi:a.shape[0]]                 # not where u is pure rounding
    assert np.allclose(a[keep], b[keep], rtol=1e-6, atol=0)
    # the zero group is the identity exactly, in both forward restatements
    lo, hi = aa["spans"]["zero"]
    eye = np.broadcast_to(np.eye(3, dtype=np.float32), (RC.GROUP, 3, 3))
    assert np.array_equal(RC.aa_to_rotmat_kernel_np(x)[lo:hi], eye) and np.array_equal(RC.rodrigues_kernel_np(x)[lo:hi], eye)
    assert not fails, "\n".join(fails)


GENERIC = {"aa": ("randn0.8",), "r6": ("randn",)}


def _mutant(aa, r6, mistake):
    if mistake == "rot6d_adjoint_fp32":
        dev = RC.rot6d_backward_np(r6["x"].numpy(), r6["gR"].numpy(), np.float32)
        op, r32, r64, spans, generic = "rot6d_backward", r6["bwd32"], r6["bwd64"], r6["spans"], GENERIC["r6"]
    else:
        dev = RC.rodrigues_backward_kernel_np(aa["x"].numpy(), aa["gR"].numpy(), mistake)
        op, r32, r64, spans, generic = "aa_to_rotmat_backward", _aa_ref32(aa), aa["quat.bwd64"], aa["spans"], GENERIC["aa"]
    print()
    table = []
    RC.check_groups(op, torch.from_numpy(dev), r32, r64, spans, table=table)
    broken = [g for g, d, own, r, b in table if not d <= b]
    _table(f"planted mistake {mistake}: breaks {broken}", table)
    return broken, generic


@pytest.mark.parametrize("mistake", ["one_minus_cos", "no_epsilon"])
def test_the_rule_has_teeth(aa, r6, mistake):
    """1 - cos a in place of 2 sin^2(a / 2), and the + 1e-8 dropped ("simplified"), in the Rodrigues adjoint: each breaks at least one edge
    group and passes the generic group, which is all the suite fed the kernel before."""
    broken, generic = _mutant(aa, r6, mistake)
    assert broken, f"{mistake} passes every group"
    assert not set(generic) & set(broken), f"{mistake} is caught by the generic group already"


@pytest.mark.parametrize("mistake", ["rot6d_adjoint_fp32", "x_over_a"])
def test_two_planted_mistakes_the_rule_does_not_catch(aa, r6, mistake):
    """Recorded, not hidden: these two break NO group, and the arithmetic says why.
    rot6d_adjoint_fp32: the rule grants MULT x the reference's own fp32 distance, and the reference's own adjoint IS an fp32 evaluation, so
    an fp32 kernel sits at ratio ~1 in every group (0.7 ... 1.2); the fp64 kernel sits at 0.00 ... 0.6.  The rule cannot tell a kernel that
    is as good as the reference from one that is better; what keeps the fp64 evaluation is tests/test_gpu_tokenizer_loss.py's row checks.
    x_over_a: the last line's factor ga is the difference of w . d cos a and (gd . r) / a^2, which cancel to rounding noise (1e-7) wherever
    1e-8 / a is not negligible, so ga (ex - x) / a is below the bound in every group.
    If a change of the rule or of the sets makes either fail a group, move it to test_the_rule_has_teeth."""
    broken, _ = _mutant(aa, r6, mistake)
    assert not broken, f"{mistake} now breaks {broken}: move it to test_the_rule_has_teeth"


def test_the_oracle_equals_the_reference_on_the_edge_sets(aa, r6):
    """aa_to_rotmat and rot6d_to_rotmat against the reference's own geometry.py, NaN row included.  batch_rodrigues stays a restatement:
    smplx is not installed where this suite runs (oracle/ref_import.py stubs it)."""
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("reference tree not present")
    geo = ref_import.load().geometry
    for dt in (torch.float32, torch.float64):
        x = torch.cat([aa["x"], RC.nan_rows()], 0).to(dt)
        assert torch.equal(torch.nan_to_num(geo.aa_to_rotmat(x), nan=7.0), torch.nan_to_num(O.aa_to_rotmat(x), nan=7.0))
        y = r6["x"].to(dt)
        assert torch.equal(geo.rot6d_to_rotmat(y), O.rot6d_to_rotmat(y))
        for fn_ref, fn, inp, gR in ((geo.aa_to_rotmat, O.aa_to_rotmat, aa["x"], aa["gR"]), (geo.rot6d_to_rotmat, O.rot6d_to_rotmat, r6["x"], r6["gR"])):
            assert torch.equal(RC.vjp(fn_ref, inp, gR, dt), RC.vjp(fn, inp, gR, dt))
