"""CPU (-m "not gpu"): the proof that the rule of tests/attention_cases.py sees what the older attention tests
(tests/test_gpu_ops.py::test_vit_attention*: softmax(q k^T) v on Gaussian q, k, v against float64, atol 5e-6 at scale 1 and
max(4 err_cpu, 2e-5) on peaked scores) do not.  The plain fp32 statement (q @ k^T).softmax(-1) is inside every condition on all seven
cases; five mutations of it — each the natural side effect of an optimisation of the attention kernels — are outside the rule at the
ceiling of the multipliers (4) on the cases named, and inside the older tolerance wherever that tolerance lets them through.

Measured here (seed 1; mutant's units / the fp32 statement's units on the same case, the rule's multiplier being at most 4):
    probabilities below 2^-20 of the row maximum flushed to zero     peaked 6.3e4, rising 1.7e4, falling 1.8e4, edge_onehot 2.9e4
    P as two bf16 pieces instead of three                            uniform 128, zero_q 128, gauss 5.2 (peaked 1.0: not named)
    q as two bf16 pieces                                             gauss 7.0, peaked 8.5
    running row sum not rescaled on a maximum update (64-key blocks) gauss 4.8e5, rising 2.2e4, edge_onehot 6.3e4
    v as two bf16 pieces (V side, units of P64 @ |V|)                edge_onehot 126 against a ceiling of 4; gauss 4.1 x the statement's own"""
import pytest
import torch

import attention_cases as AC

SEED = 1


def _two_pieces(x):
    hi = x.bfloat16().float()
    return hi + (x - hi).bfloat16().float()


def _flush(q, k):
    s = q @ k.transpose(-2, -1)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    e = torch.where(e < 2.0 ** -20, torch.zeros_like(e), e)
    return e / e.sum(-1, keepdim=True)


def _two_piece_P(q, k):
    return _two_pieces(AC.statement32(q, k))


def _two_piece_q(q, k):
    return AC.statement32(_two_pieces(q), k)


def _sum_not_rescaled(q, k):
    """Three 64-key blocks under a running maximum; the accumulators are rescaled on a maximum update, the row sum is not."""
    s = q @ k.transpose(-2, -1)
    m = torch.full(s.shape[:-1] + (1,), -1e30)
    l = torch.zeros_like(m)
    acc = torch.zeros_like(s)
    for b in range(3):
        sb = s[..., 64 * b:64 * b + 64]
        mn = torch.maximum(m, sb.amax(-1, keepdim=True))
        acc = acc * torch.exp(m - mn)
        e = torch.exp(sb - mn)
        acc[..., 64 * b:64 * b + 64] = e
        l = l + e.sum(-1, keepdim=True)
        m = mn
    return acc / l


# mutant -> (the statement, the cases it must fail the rule on at MULT_MAX, the cases on which the older criterion passes it)
MUTANTS = {"flush": (_flush, ("peaked", "rising", "falling", "edge_onehot"), ("peaked", "edge_onehot")),
           "two_piece_P": (_two_piece_P, ("uniform", "zero_q", "gauss"), ("gauss",)),
           "two_piece_q": (_two_piece_q, ("gauss", "peaked"), ("gauss",)),
           "sum_not_rescaled": (_sum_not_rescaled, ("gauss", "rising", "edge_onehot"), ())}


@pytest.fixture(scope="module")
def refs():
    """Per case: q, k, the float64 side and the fp32 statement, computed once and left unchanged."""
    out = {}
    for name in AC.CASES:
        q, k = AC.crop(name, SEED)
        out[name] = dict(q=q, k=k, ref=AC.Reference(q, k), P32=AC.statement32(q, k))
    return out


def _old_criterion(name, P, r):
    """What tests/test_gpu_ops.py asks of an attention output on Gaussian V: allclose(atol 5e-6, rtol 1e-5) to float64, and on peaked
    scores max |err| <= max(4 err_cpu, 2e-5)."""
    v = AC.gauss_v(SEED)
    o64 = r["ref"].P64 @ v.double()
    err = ((P @ v).double() - o64).abs()
    own = ((r["P32"] @ v).double() - o64).abs().max().item()
    print(f"   older criterion on {name}: max |out - out64| {err.max().item():.2e}, the fp32 statement's own {own:.2e}")
    if name == "peaked":
        return err.max().item() <= max(4 * own, 2e-5)
    return bool((err <= 5e-6 + 1e-5 * o64.abs()).all())


@pytest.mark.parametrize("name", AC.CASES)
def test_fp32_statement_is_inside_every_condition(refs, name):
    r = refs[name]
    ref, P32 = r["ref"], r["P32"]
    ok, fig = AC.check_P(f"[{name}] fp32 statement", P32, ref, P32, 1.0)
    assert ok and fig["out_of_rule"] == 0 and fig["masked"] <= AC.MASK_CAP, fig
    assert fig["below_max"] <= AC.P_BELOW_MAX, fig
    ones = AC.rowsum_ulps(P32 @ torch.ones(AC.NH, AC.NTOK, AC.HD))
    v = AC.wide_v(SEED)
    uv = AC.v_units(P32 @ v, ref, v)
    print(f"[{name}] fp32 statement: row sums {ones:.1f} ulp off 1, V side {uv:.3g} units of P64 @ |V|")
    assert ones <= AC.ROWSUM_ULPS, ones
    if name == "edge_onehot":
        assert uv <= AC.ONEHOT_V_UNITS, uv


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_rule_sees_the_mutant_the_older_criterion_passes(refs, mutant):
    fn, fails_on, old_passes_on = MUTANTS[mutant]
    for name in fails_on:
        r = refs[name]
        P = fn(r["q"], r["k"])
        ok, fig = AC.check_P(f"[{name}] {mutant}", P, r["ref"], r["P32"], AC.MULT_MAX)
        assert not ok and fig["out_of_rule"] > 0, (mutant, name, fig)
        assert fig["ratio"] > AC.MULT_MAX, (mutant, name, fig)
        if name in old_passes_on:
            assert _old_criterion(name, P, r), (mutant, name)
    if mutant == "sum_not_rescaled":                                     # the row sums see it too: off by 1e-3 or more, not by ulps
        for name in fails_on:
            r = refs[name]
            ones = AC.rowsum_ulps(fn(r["q"], r["k"]) @ torch.ones(AC.NH, AC.NTOK, AC.HD))
            print(f"[{name}] {mutant}: row sums {ones:.3g} ulp off 1")
            assert ones > 1e-3 / AC.ULP > AC.ROWSUM_ULPS, (name, ones)


def test_v_side_sees_two_piece_v(refs):
    """v cut to two bf16 pieces: on `edge_onehot` the output is one V row, so the derived 4 units catch it; on `gauss` the ratio rule does at
    the ceiling; the older criterion (Gaussian V, scale 1) passes it."""
    v = AC.wide_v(SEED)
    v2 = _two_pieces(v)
    r = refs["edge_onehot"]
    own, got = AC.v_units(r["P32"] @ v, r["ref"], v), AC.v_units(r["P32"] @ v2, r["ref"], v)
    print(f"[edge_onehot] V side: fp32 statement {own:.3g} units, two-piece v {got:.3g}")
    assert own <= AC.ONEHOT_V_UNITS < got
    r = refs["gauss"]
    own, got = AC.v_units(r["P32"] @ v, r["ref"], v), AC.v_units(r["P32"] @ v2, r["ref"], v)
    print(f"[gauss] V side: fp32 statement {own:.3g} units, two-piece v {got:.3g} ({got / own:.1f} x)")
    assert got > max(AC.FLOOR_UNITS, AC.MULT_MAX * own)
    gv = AC.gauss_v(SEED)
    o64 = r["ref"].P64 @ gv.double()
    err = ((r["P32"] @ _two_pieces(gv)).double() - o64).abs()
    print(f"   older criterion on gauss: max |out - out64| {err.max().item():.2e}")
    assert bool((err <= 5e-6 + 1e-5 * o64.abs()).all())


def test_cases_and_read_out():
    """The constructions are what they claim, and the three probes read a probability matrix out of a P.V exactly."""
    q, k = AC.crop("edge_onehot", SEED)
    s = q.double() @ k.double().transpose(-2, -1)
    for h in (0, 5, 15):
        for i in (0, 13, 14, 191):
            bonus = torch.zeros(AC.NTOK, dtype=torch.float64)
            bonus[AC.EDGE[i % 14]] = 49.0
            rest = q[h, i, 14:].double() @ k[h, :, 14:].double().T
            assert torch.allclose(s[h, i], rest + bonus, atol=1e-12)
    assert AC.Reference(q, k).P64.amax(-1).min() > 1 - 1e-15              # a one-hot to 1e-21 ...
    assert bool((AC.Reference(q, k).P64.argmax(-1) == torch.tensor(AC.EDGE)[torch.arange(192) % 14]).all())       # ... on the key meant
    for name in ("uniform", "zero_q"):
        qu, ku = AC.crop(name, SEED)
        assert torch.equal(AC.Reference(qu, ku).P64, torch.full((AC.NH, AC.NTOK, AC.NTOK), 1.0 / 192, dtype=torch.float64))
    qr, kr = AC.crop("rising", SEED)
    qf, kf = AC.crop("falling", SEED)
    assert torch.equal(kr[:, :, 0], (3.0 * (torch.arange(192) // 16)).expand(16, 192)) and torch.equal(kf[:, :, 0], kr[:, :, 0].flip(-1))
    assert torch.equal(kr[:, :, 1:], kf[:, :, 1:]) and torch.equal(qr, qf) and bool((qr[:, :, 0] == 1).all())
    with pytest.raises(AssertionError):                                   # the mask cap is a condition: scores x 36 put 77 % below 2^-100
        qg, kg = AC.crop("gauss", SEED)
        AC.Reference(6.0 * qg, 6.0 * kg)
    # the read-out, through a plain fp32 P.V standing in for a kernel, on two crops of different cases
    qs, ks = torch.stack([qr, q]), torch.stack([kr, k])
    P32 = AC.statement32(qs, ks)

    def run(qkv):
        t = qkv.reshape(2, 192, 3, 16, 80).permute(2, 0, 3, 1, 4)
        assert torch.equal(t[0], qs) and torch.equal(t[1], ks)
        return (P32 @ t[2]).transpose(1, 2).reshape(2, 192, 1280)

    P, pad = AC.read_out(run, qs, ks)
    assert torch.equal(P, P32) and pad.shape == (2, 16, 192, 48) and bool((pad == 0).all())
    assert torch.equal(AC.unpack(AC.pack(qs, ks, 1.0)[:, :, 2560:]), torch.ones(2, 16, 192, 80))
