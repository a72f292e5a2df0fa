"""Strided operands and guard bands for the GEMM and attention operators (-m gpu).

Every GEMM entry point of the C ABI takes leading dimensions, and the engine depends on them (the token head's read-out is N = 31 into
ldc = 32; proj / fc2 / to_out add their residual in place; attention -> proj and fc1 -> fc2 go through ldcs).  Here each operator id runs
with its operands and its result as WINDOWS of larger buffers full of NaN canaries (tests/guarded.py):

  * A, W, bias and the residual sit between NaN pads (lda = K + 8, ldw = K + 16 where the operator has an ldw; two guard rows before and
    after): a pad that leaks into a product poisons the result;
  * the result must be torch.equal to the SAME call on contiguous copies with a fresh output — the form the parity tests of
    test_gpu_ops.py hold to fp64 — so no tolerance appears in this file;
  * afterwards every canary outside every window must be intact, compared as integers.

The cases are planned by the functions `f32_cases` / `s3_cases` below from rules stated there; a case the operator must REFUSE (the split-K
reduce stores 16-byte vectors) is asserted to raise and to leave its output untouched rather than skipped.  `test_every_production_id_is_planned`
checks the plan against ops.VARIANT / ops.SPLIT3_VARIANT without a GPU."""
import pytest
import torch

from tests import guarded as G

gpu = pytest.mark.gpu
QS = dict(qscale=80 ** -0.5)


def _ops():
    from tokenhmr_amd import ops
    return ops


def _rnd(dev, *shape, seed, scale=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=dev) * scale


def _up(n, m):
    return (n + m - 1) // m * m


def _ksplit(variant):
    return int(variant.rsplit("/k", 1)[1]) if "/k" in variant else 1


# ---- the ldc / base-pointer cases of an fp32 result: name -> (ldc, first column of the window in its buffer)
def c_cases(N, unaligned_base=False):
    """plain: ldc = N.  ld+1: row starts lose their 16-byte alignment; the scalar path of the split3 kernels whenever N + 1 is odd.
    ld+4: an aligned pad.  round32+32: N rounded up to 32, plus 32.  col4: the window starts at column 4 of its buffer — 16-byte aligned,
    never 64 (the buffer starts 2 ldc floats in; ldc % 4 == 0 there).  col1 (split3 kernels, epilogues without a residual): C & 15 != 0
    with ldc % 4 == 0, so it is the base pointer alone that forces the scalar stores."""
    c = {"plain": (N, 0), "ld+1": (N + 1, 0), "ld+4": (N + 4, 0), "round32+32": (_up(N, 32) + 32, 0), "col4": (_up(N, 4) + 8, 4)}
    if unaligned_base:
        c["col1"] = (_up(N, 4) + 8, 1)
    return c


def splitk_refusal(variant, N, ld, col0):
    """The one stated rule by which a planned case is refused instead of run: a split-K id reduces its partial planes with 16-byte loads
    and stores (launch_splitk_epilogue), so it needs N % 4 == 0, ldc % 4 == 0 and a 16-byte aligned C."""
    return _ksplit(variant) > 1 and (N % 4 != 0 or ld % 4 != 0 or col0 % 4 != 0)


# ---- the plan: thmr_op_gemm ----
F32_SHAPES = [(37, 31, 64), (130, 164, 96), (200, 72, 256), (1, 8, 64)]
F32_MAIN = ["128x128", "128x160", "128x96", "64x64", "64x128", "128x64", "128x128reg", "128x160reg", "auto",
            "ring4", "ring8", "ring4/k2", "ring16", "skinny", "tiny", "128x128/k2", "auto/k4"]
F32_EPIS = ["none", "bias_gelu", "bias_resid", "bias_qscale"]


def f32_epis(variant):
    """the epilogues the id takes: ring16 (120) has no residual epilogue (op_gemm_variants.h), the skinny kernel none beyond 0 ... 4
    (launch_gemm_skinny: no column scale)"""
    return [e for e in F32_EPIS if (variant, e) not in (("ring16", "bias_resid"), ("skinny", "bias_qscale"))]


def f32_K(variant, K):
    """K = 256 (more for a deeper split) where the id needs it: split-K wants K % (32 ksplit) == 0, tiny K % 256, skinny K % 64."""
    need = 256 if variant == "tiny" else 64 if variant == "skinny" else 32 * _ksplit(variant)
    return K if K % need == 0 else max(256, need)


def f32_cases():
    """(variant, (M, N, K)): the ids the engine and the per-kernel tests use at all four shapes — skinny, the M <= 64 kernel, at the two
    shapes with M <= 64 — and every other name of ops.VARIANT (deeper splits, split-K on the other tiles) at (200, 72, 256)."""
    from tokenhmr_amd import ops
    out = []
    for v in F32_MAIN:
        for M, N, K in F32_SHAPES:
            if v == "skinny" and M > 64:
                continue
            out.append((v, (M, N, f32_K(v, K))))
    for v in ops.VARIANT:
        if v not in F32_MAIN:
            out.append((v, (200, 72, f32_K(v, 256))))
    return out


# ---- the plan: thmr_op_gemm_split3, fp32 C ----
S3_SHAPES = [(200, 300, 96), (129, 257, 64), (37, 31, 64), (1, 8, 64)]
S3_MAIN = ["auto", "128x256/w8", "128x128/w4", "128x128/w4/s3", "128x256/w8/front", "auto/k2", "auto/k4"]
S3_EPIS = ["none", "bias", "bias_gelu", "bias_resid", "bias_qscale"]
# experiments-build ids that run on any shape (the old/*, ring*, /w8 and 256x256 forms and the schedule experiment; the timing-only abl/*
# ids write documented garbage, and old/persist* need whole 128-row tiles of a stream shape: neither is planned)
S3_EXP = ["old/128x256/w8", "old/128x128/w4", "ring", "ring/k2", "ring/k4", "128x128/w8", "128x128/w8/s3", "128x128/w4/s3/front", "128x256/w4",
          "256x256/w4", "exp/reads-every-2nd"]
# ids with an acceptance rule of their own: each at the smallest shape it admits (derived at test_split3_streams_and_tail)
S3_RULED = ["tail", "persist", "persist/swap", "persist/128x128", "persist/128x128/k2", "persist/128x128/k4"]


def s3_K(variant, K):
    need = 32 * _ksplit(variant)
    return K if K % need == 0 else 256


def s3_cases():
    out = [(v, (M, N, s3_K(v, K))) for v in S3_MAIN for M, N, K in S3_SHAPES]
    return out + [(v, (200, 300, s3_K(v, 96))) for v in S3_EXP]


def test_every_production_id_is_planned():
    """Coverage bookkeeping, without a GPU: every name of ops.VARIANT (the named rows of kOpGemmF32 and launch_gemm's own tiles) and every
    name of ops.SPLIT3_VARIANT outside SPLIT3_EXP_ONLY (the non-experiment rows of kOpGemmS3) has at least one case in this file; the
    experiments ids are the planned ones plus the stated exclusions, and every fp32 case list holds every ldc case."""
    ops = _ops()
    assert {v for v, _ in f32_cases()} == set(ops.VARIANT)
    production = set(ops.SPLIT3_VARIANT) - ops.SPLIT3_EXP_ONLY
    assert {v for v, _ in s3_cases() if v not in ops.SPLIT3_EXP_ONLY} | set(S3_RULED) == production
    assert set(S3_EXP) | {"tail/w8"} == {v for v in ops.SPLIT3_EXP_ONLY if not v.startswith(("abl/", "old/persist"))}
    assert set(S3_EXP) <= ops.SPLIT3_EXP_ONLY and not set(S3_MAIN + S3_RULED) & ops.SPLIT3_EXP_ONLY
    assert set(c_cases(31)) == {"plain", "ld+1", "ld+4", "round32+32", "col4"} and set(c_cases(31, True)) - set(c_cases(31)) == {"col1"}
    for N in (31, 72, 257, 300):
        cs = c_cases(N, True)
        assert cs["ld+1"][0] == N + 1 and cs["round32+32"][0] % 32 == 0 and cs["round32+32"][0] >= N + 32
        assert cs["col4"][0] % 4 == 0 and cs["col4"][0] >= 4 + N and cs["col1"][0] % 4 == 0 and cs["col1"][0] >= 1 + N
        assert (2 * cs["col4"][0] + 4) % 16 != 0                  # 16-byte aligned, not 64
    # the refusal rule bites exactly on the split-K ids
    assert splitk_refusal("auto/k2", 31, 31, 0) and splitk_refusal("ring4/k2", 72, 73, 0) and splitk_refusal("auto/k4", 300, 308, 1)
    assert not splitk_refusal("auto/k4", 300, 304, 4) and not splitk_refusal("128x128", 31, 32, 1)


# ---- operands in guard bands ----
class Operands:
    """A (M, K), W (N, K), bias (N), resid (M, N) on the device: contiguous, and as windows between NaN pads.  split3: A and W as split3
    operands (lda = K + 8, ldw = K + 16); else fp32 A with lda = K + 8 and a dense W (thmr_op_gemm has no ldw) between NaN guard rows."""

    def __init__(self, dev, M, N, K, split3, seed=0):
        ops = _ops()
        self.M, self.N, self.K, self.split3, self.dev = M, N, K, split3, dev
        a, w = _rnd(dev, M, K, seed=seed + 1), _rnd(dev, N, K, seed=seed + 2, scale=K ** -0.5)
        self.bias, self.resid = _rnd(dev, N, seed=seed + 3), _rnd(dev, M, N, seed=seed + 4)
        self.checks = []
        if split3:
            self.a, self.w = ops.split3(a), ops.split3(w)
            self.a_g, ca = G.guarded_split3(M, K, K + 8, device=dev, fill=self.a)
            self.w_g, cw = G.guarded_split3(N, K, K + 16, device=dev, fill=self.w)
        else:
            self.a, self.w = a, w
            self.a_g, ca = G.guarded(M, K, K + 8, device=dev, fill=a)
            self.w_g, cw = G.guarded(N, K, K, device=dev, fill=w)
        b_g, cb = G.guarded(1, N, _up(N, 4) + 4, device=dev, fill=self.bias.reshape(1, N))
        self.bias_g = b_g[0]
        self.checks += [("A", ca), ("W", cw), ("bias", cb)]
        self._ref = {}

    def call(self, variant, epi, **kw):
        ops = _ops()
        if epi == "bias_qscale":
            kw.update(QS, qcols=self.N // 3 + 1)                    # the scaled columns end inside a quad
        a, w, bias, resid = kw.pop("a"), kw.pop("w"), kw.pop("bias"), kw.pop("resid", None)
        return (ops.gemm_split3 if self.split3 else ops.gemm)(a, w, bias if epi != "none" else None, resid, epi=epi, variant=variant, **kw)

    def ref(self, variant, epi, **kw):
        """the already-tested form, once per (id, epilogue): contiguous operands, a fresh output"""
        key = (variant, epi, tuple(sorted(kw.items())))
        if key not in self._ref:
            self._ref[key] = self.call(variant, epi, a=self.a, w=self.w, bias=self.bias, resid=self.resid if epi == "bias_resid" else None, **kw)
            assert not torch.isnan(self._ref[key].float() if self._ref[key].dtype == torch.float32 else self._ref[key].view(torch.bfloat16).float()).any()
        return self._ref[key]

    def guarded_call(self, variant, epi, **kw):
        return self.call(variant, epi, a=self.a_g, w=self.w_g, bias=self.bias_g, **kw)


_OPERANDS = {}


def operands(dev, M, N, K, split3):
    key = (str(dev), M, N, K, split3)
    if key not in _OPERANDS:
        if len(_OPERANDS) > 6:
            _OPERANDS.clear()
        _OPERANDS[key] = Operands(dev, M, N, K, split3)
    return _OPERANDS[key]


def intact(checks, ctx, fails):
    for name, chk in checks:
        try:
            chk()
        except AssertionError as e:
            fails.append(f"{ctx}: {name}: {e}")


def is_canary(t):
    bits = t.view(torch.int32) if t.dtype == torch.float32 else t
    return bool((bits == G.CANARY[t.dtype]).all())


def run_fp32_c_case(o, variant, epi, cname, ld, col0, fails, inplace=False):
    """One case of the common recipe.  The result window (and, out of place, the residual's: the operator reads both with one stride) has
    row stride ld and starts at column col0 of a guarded buffer."""
    from tokenhmr_amd._cabi import EngineError
    ctx = f"{variant} {(o.M, o.N, o.K)} {epi} {cname} (ldc {ld}, column {col0})" + (" in place" if inplace else "")
    c_w, cc = G.guarded(o.M, o.N, ld, col0=col0, device=o.dev, fill=o.resid if inplace else None)
    checks = o.checks + [("C", cc)]
    kw = {}
    if inplace:
        kw["resid"] = c_w
    elif epi == "bias_resid":
        r_w, cr = G.guarded(o.M, o.N, ld, col0=col0, device=o.dev, fill=o.resid)
        checks.append(("resid", cr))
        kw["resid"] = r_w
    if splitk_refusal(variant, o.N, ld, col0):
        with pytest.raises(EngineError, match="split-K"):
            o.guarded_call(variant, epi, out=c_w, **kw)
        if not (torch.equal(c_w, o.resid) if inplace else is_canary(c_w)):
            fails.append(f"{ctx}: a refused call wrote its output")
    else:
        try:
            got = o.guarded_call(variant, epi, out=c_w, **kw)
        except EngineError as e:
            fails.append(f"{ctx}: refused: {e}")
            return
        assert got is c_w
        want = o.ref(variant, epi)
        if not torch.equal(c_w, want):
            bad = (c_w.view(torch.int32) != want.view(torch.int32))
            n, where = G._first_difference(bad, ("row", "column"))
            fails.append(f"{ctx}: {n} element(s) differ from the contiguous call, the first at {where}")
        if epi == "bias_resid" and not inplace and not torch.equal(kw["resid"], o.resid):
            fails.append(f"{ctx}: the residual was written")
    intact(checks, ctx, fails)


def report(fails):
    assert not fails, f"{len(fails)} failure(s):\n" + "\n".join(fails[:12])


# ---- a. thmr_op_gemm ----
@gpu
@pytest.mark.parametrize("variant,shape", f32_cases(), ids=lambda x: x.replace("/", "_") if isinstance(x, str) else "x".join(map(str, x)))
def test_gemm_strided(built_lib, cuda_dev, variant, shape):
    """thmr_op_gemm, every id: every epilogue the id takes x every ldc case; with bias_resid also the sum IN PLACE (out is resid: the
    engine's normal form) at ldc = N and N + 4."""
    o = operands(cuda_dev, *shape, False)
    fails = []
    for epi in f32_epis(variant):
        for cname, (ld, col0) in c_cases(o.N).items():
            run_fp32_c_case(o, variant, epi, cname, ld, col0, fails)
        if epi == "bias_resid":
            for cname in ("plain", "ld+4"):
                run_fp32_c_case(o, variant, epi, cname, *c_cases(o.N)[cname], fails, inplace=True)
    report(fails)


@gpu
@pytest.mark.parametrize("M", [1, 5, 64])
def test_gemm_skinny_is_the_engines_read_out(built_lib, cuda_dev, M):
    """The token head's read-out as the engine runs it: the skinny kernel, N = 31 into ldc = 32 (head_finish reads ro with ld 32)."""
    o = operands(cuda_dev, M, 31, 1024, False)
    fails = []
    for epi in ("none", "bias", "bias_gelu", "bias_resid"):
        run_fp32_c_case(o, "skinny", epi, "read-out", 32, 0, fails)
    run_fp32_c_case(o, "skinny", "bias_resid", "read-out", 32, 0, fails, inplace=True)
    report(fails)


# ---- b. thmr_op_gemm_split3, fp32 C ----
def _exp_or_skip(variant):
    ops = _ops()
    if variant in ops.SPLIT3_EXP_ONLY:
        try:
            from tokenhmr_amd import _cabi
            _cabi.load(exp=True)
        except Exception as e:       # noqa: BLE001
            pytest.skip(f"{variant} exists in the experiments build only, and that build is absent: {e}")


def s3_epis(variant):
    if variant == "exp/reads-every-2nd":
        return ["none"]                                                # op_gemm_variants.h: id 3 takes no epilogue
    return S3_EPIS


@gpu
@pytest.mark.parametrize("variant,shape", s3_cases(), ids=lambda x: x.replace("/", "_") if isinstance(x, str) else "x".join(map(str, x)))
def test_gemm_split3_strided(built_lib, cuda_dev, variant, shape):
    """thmr_op_gemm_split3 with an fp32 result: every epilogue x every ldc case, the unaligned base (column 1) for the epilogues without a
    residual, and the residual sum in place at ldc = N and N + 4.  N = 257 and N = 31 reach the scalar tail inside a vector-store launch;
    ldc = N + 1 forces the scalar path everywhere.  The experiments-build ids run the two padded cases."""
    _exp_or_skip(variant)
    ops = _ops()
    o = operands(cuda_dev, *shape, True)
    fails = []
    for epi in s3_epis(variant):
        cases = c_cases(o.N, unaligned_base=epi != "bias_resid")
        if variant in ops.SPLIT3_EXP_ONLY:
            cases = {k: cases[k] for k in ("ld+1", "ld+4")}
        for cname, (ld, col0) in cases.items():
            run_fp32_c_case(o, variant, epi, cname, ld, col0, fails)
        if epi == "bias_resid":
            for cname in ("plain", "ld+4"):
                run_fp32_c_case(o, variant, epi, cname, *c_cases(o.N)[cname], fails, inplace=True)
    report(fails)


@gpu
@pytest.mark.parametrize("variant", ["128x256/w8", "128x128/w4"])
def test_gemm_split3_pos_embed_strided(built_lib, cuda_dev, variant):
    """The patch-embed epilogue at M = 193 — one row past the wrap of the position index — N = 64, K = 64, every ldc case (the position
    table is (193, N), dense: it is not a residual and has no stride)."""
    ops = _ops()
    o = operands(cuda_dev, 193, 64, 64, True)
    pos = _rnd(cuda_dev, 193, 64, seed=9)
    want = ops.gemm_split3(o.a, o.w, o.bias, pos, epi="bias_pos", variant=variant)
    fails = []
    for cname, (ld, col0) in c_cases(64, unaligned_base=True).items():
        c_w, cc = G.guarded(193, 64, ld, col0=col0, device=cuda_dev)
        ops.gemm_split3(o.a_g, o.w_g, o.bias_g, pos, epi="bias_pos", variant=variant, out=c_w)
        if not torch.equal(c_w, want):
            fails.append(f"{variant} bias_pos {cname}: differs from the contiguous call")
        intact(o.checks + [("C", cc)], f"{variant} bias_pos {cname}", fails)
    report(fails)


# The ids with an acceptance rule, each at the SMALLEST shape the rule admits (smallest = fewest tiles, then fewest rows and the shortest K),
# and at that shape plus one tile column — the first with a ragged last round, whose hand-over between workgroups is what the workspace is
# for.  P = 256 workgroups (8 XCDs x 32 CUs).
#   persist (gemm_split3_persist_ok): M % 32 == 0, N % 256 == 0, K % 32 == 0, K >= 64, ceil(M / 128) * (N / 256) >= 256
#       -> M = 32 (one ragged row tile), N = 256 * 256 = 65536, K = 64.                                persist/swap: the same rule.
#   persist/128x128 (..._narrow_ok): N % 128 == 0, K % 32 == 0, K >= 96, ceil(M / 128) * (N / 128) >= 256, any M
#       -> N = 256 * 128 = 32768, K = 96; M = 37 (any M <= 128 is one row tile: 37 keeps it ragged and odd).
#   persist/128x128/k<S> (the same rule on (tile, K slice) units): K % (32 S) == 0, K / S >= 96, ceil(M / 128) * (N / 128) * S >= 256;
#       the reduce wants N % 4 == 0 -> S = 2: N = 128 * 128 = 16384, K = 192; S = 4: N = 64 * 128 = 8192, K = 384.
#   tail (split3_rule::choose, csrc/gemm_split3_rule.h): N % 256 == 0; T = ceil(M / 128) * (N / 256) tiles, T % 8 == 0; an XCD's share q = T / 8 holds at least
#       one full round of 32 and a rest of 1 ... 16 -> q = 33, T = 264 -> M = 37 (one row tile), N = 264 * 256 = 67584, K = 32 is admitted
#       by the rule; K = 64 is used (two K tiles: the double buffer turns over once).
RULED_SHAPES = [("persist", (32, 65536, 64)), ("persist", (32, 65536 + 256, 64)),
                ("persist/128x128", (37, 32768, 96)), ("persist/128x128", (37, 32768 + 128, 96)),
                ("persist/128x128/k2", (37, 16384, 192)), ("persist/128x128/k2", (37, 16384 + 128, 192)),
                ("persist/128x128/k4", (37, 8192, 384)),
                ("tail", (37, 67584, 64)), ("tail/w8", (37, 67584, 64))]


def _needs_256_cus(dev):
    if torch.cuda.get_device_properties(dev).multi_processor_count != 256:
        pytest.skip("the persistent / tail decomposition is 8 XCDs x 32 CUs")


@gpu
@pytest.mark.parametrize("variant,shape", RULED_SHAPES, ids=lambda x: x.replace("/", "_") if isinstance(x, str) else "x".join(map(str, x)))
def test_split3_streams_and_tail(built_lib, cuda_dev, variant, shape):
    """tail, persist, persist/128x128 and its split-K forms at ldc = N + 4, epilogues none and bias_resid (also in place): equal to the
    contiguous call, every pad intact — and run twice with a contiguous call in between: the hand-over workspace does not depend on ldc."""
    _needs_256_cus(cuda_dev)
    _exp_or_skip(variant)
    o = operands(cuda_dev, *shape, True)
    fails = []
    for epi in ("none", "bias_resid"):
        for _ in range(2):
            run_fp32_c_case(o, variant, epi, "ld+4", o.N + 4, 0, fails)
            if not torch.equal(o.call(variant, epi, a=o.a, w=o.w, bias=o.bias, resid=o.resid if epi == "bias_resid" else None), o.ref(variant, epi)):
                fails.append(f"{variant} {shape} {epi}: the contiguous call after a strided one differs from the one before")
    run_fp32_c_case(o, variant, "bias_resid", "ld+4", o.N + 4, 0, fails, inplace=True)
    run_fp32_c_case(o, variant, "bias_resid", "plain", o.N, 0, fails, inplace=True)
    report(fails)


# ---- c. thmr_op_gemm_split3_out_split3 ----
OUT_TILE_SHAPES = [(200, 296, 96), (37, 40, 64), (1, 8, 64)]          # N % 8 == 0 (the operator's rule), not % 16: a ragged chunk pair
OUT_CASES = ([(v, s) for v in ("128x256/w8", "128x128/w4") for s in OUT_TILE_SHAPES] +
             [("persist/swap", (32, 65536, 64)), ("persist/128x128", (37, 32768, 96)), ("tail", (37, 67584, 64))])


@gpu
@pytest.mark.parametrize("variant,shape", OUT_CASES, ids=lambda x: x.replace("/", "_") if isinstance(x, str) else "x".join(map(str, x)))
def test_gemm_split3_out_split3_strided(built_lib, cuda_dev, variant, shape):
    """The result as a split3 operand in a guarded int16 buffer, ldcs in {N, N + 8, N + 64}: equal to ops.split3 of the fp32 result of the
    same id, every pad chunk intact."""
    if variant != "128x256/w8" and variant != "128x128/w4":
        _needs_256_cus(cuda_dev)
    ops = _ops()
    o = operands(cuda_dev, *shape, True)
    fp32_id = "persist" if variant == "persist/swap" else variant       # persist/swap has a split3 result only: the same stream, fp32 result
    fails = []
    for epi in ("none", "bias_gelu") if variant == "persist/swap" else ("none", "bias", "bias_gelu", "bias_qscale"):
        want = ops.split3(o.ref(fp32_id, epi))
        if not torch.equal(o.ref(variant, epi, out_split=True), want):
            fails.append(f"{variant} {shape} {epi}: the contiguous split3 result is not the conversion of the fp32 result")
        for ldcs in (o.N, o.N + 8, o.N + 64):
            ctx = f"{variant} {shape} {epi} ldcs {ldcs}"
            c_w, cc = G.guarded_split3(o.M, o.N, ldcs, device=cuda_dev)
            got = o.guarded_call(variant, epi, out_split=True, out=c_w)
            assert got is c_w
            if not torch.equal(c_w, want):
                fails.append(f"{ctx}: differs from split3 of the fp32 result")
            intact(o.checks + [("Cs", cc)], ctx, fails)
    report(fails)


@gpu
@pytest.mark.parametrize("M", [200, 37])
@pytest.mark.parametrize("variant", ["128x256/w8", "128x128/w4"])
def test_row_blocked_result_leaves_its_pad_rows(built_lib, cuda_dev, variant, M):
    """The row-blocked result (+ 1000): rows M ... ceil(M / 32) * 32 - 1 of the last block, and a guard block on either side, keep the
    canary — what ops.gemm_split3 relies on when it allocates that tensor zeroed 'because the kernels never write the pad rows'."""
    ops = _ops()
    o = operands(cuda_dev, M, 296, 96, True)
    fails = []
    for epi in ("none", "bias_gelu"):
        want = o.ref(variant, epi, out_split=True)
        t, ct = G.guarded_blocked(M, o.N, device=cuda_dev)
        got = o.guarded_call(variant, epi, out_split=True, out_blocked=True, out=t)
        assert got is t
        intact(o.checks + [("row-blocked Cs", ct)], f"{variant} M {M} {epi}", fails)      # before unblock: the pad rows as the kernel left them
        if not torch.equal(ops.split3_unblock(t, M), want):
            fails.append(f"{variant} M {M} {epi}: the row-blocked result differs from the row-major one")
    report(fails)


@gpu
@pytest.mark.parametrize("variant", ["128x256/w8", "128x128/w4"])
def test_split3_chain_through_a_strided_hand_over(built_lib, cuda_dev, variant):
    """fc1 -> fc2 as the engine chains them: the guarded ldcs = N + 64 result of one product is the next product's A with lda = N + 64
    (its NaN pad chunks lie between the rows the second product reads).  Bit-equal to the chain through contiguous tensors."""
    ops = _ops()
    M, N1, K, N2 = 200, 296 - 8, 96, 72                               # N1 = 288: the second product's K, a multiple of 32
    o = operands(cuda_dev, M, N1, K, True)
    w2 = ops.split3(_rnd(cuda_dev, N2, N1, seed=21, scale=N1 ** -0.5))
    w2_g, cw2 = G.guarded_split3(N2, N1, N1 + 16, device=cuda_dev, fill=w2)
    hid = ops.gemm_split3(o.a, o.w, o.bias, epi="bias_gelu", variant=variant, out_split=True)
    want = ops.gemm_split3(hid, w2, variant=variant)
    hid_g, ch = G.guarded_split3(M, N1, N1 + 64, device=cuda_dev)
    ops.gemm_split3(o.a_g, o.w_g, o.bias_g, epi="bias_gelu", variant=variant, out_split=True, out=hid_g)
    c_w, cc = G.guarded(M, N2, N2 + 4, device=cuda_dev)
    ops.gemm_split3(hid_g, w2_g, variant=variant, out=c_w)
    fails = []
    if not torch.equal(hid_g, hid):
        fails.append("the strided hand-over differs from the contiguous one")
    if not torch.equal(c_w, want):
        fails.append("the chain through the strided hand-over differs from the contiguous chain")
    intact(o.checks + [("W2", cw2), ("hand-over", ch), ("C", cc)], f"chain {variant}", fails)
    report(fails)


@gpu
@pytest.mark.parametrize("variant", ["128x256/w8", "128x128/w4", "128x128/w4/s3", "auto/k2"])
def test_fc2_form_row_blocked_hand_over_and_residual_in_place(built_lib, cuda_dev, variant):
    """fc2 exactly as the engine runs it: A is fc1's ROW-BLOCKED result (M = 200: the last block's 24 pad rows still hold NaN canaries,
    and so does a guard block on either side), the residual is summed in place (out is resid) at ldc = N and N + 4.  Bit-equal to the
    row-major, out-of-place, contiguous chain."""
    ops = _ops()
    M, N1, K, N2 = 200, 320, 96, 72                                   # N1 = the second product's K: a multiple of 64 for auto/k2
    o = operands(cuda_dev, M, N1, K, True)
    w2, b2, r = ops.split3(_rnd(cuda_dev, N2, N1, seed=21, scale=N1 ** -0.5)), _rnd(cuda_dev, N2, seed=22), _rnd(cuda_dev, M, N2, seed=23)
    w2_g, cw2 = G.guarded_split3(N2, N1, N1 + 16, device=cuda_dev, fill=w2)
    hid = ops.gemm_split3(o.a, o.w, o.bias, epi="bias_gelu", variant="128x256/w8", out_split=True)
    want = ops.gemm_split3(hid, w2, b2, r, epi="bias_resid", variant=variant)
    hid_b, chb = G.guarded_blocked(M, N1, device=cuda_dev)
    ops.gemm_split3(o.a_g, o.w_g, o.bias_g, epi="bias_gelu", variant="128x256/w8", out_split=True, out_blocked=True, out=hid_b)
    fails = []
    if not torch.equal(ops.split3_unblock(hid_b, M), hid):
        fails.append("the row-blocked hand-over differs from the row-major one")
    for ld in (N2, N2 + 4):
        c_w, cc = G.guarded(M, N2, ld, device=cuda_dev, fill=r)
        assert ops.gemm_split3(hid_b, w2_g, b2, c_w, epi="bias_resid", variant=variant, a_blocked_rows=M, out=c_w) is c_w
        if not torch.equal(c_w, want):
            fails.append(f"ldc {ld}: the in-place sum over a row-blocked A differs from the out-of-place row-major chain")
        intact(o.checks + [("W2", cw2), ("row-blocked hand-over", chb), ("C", cc)], f"fc2 form {variant} ldc {ld}", fails)
    report(fails)


@gpu
def test_the_guard_check_bites_on_the_device(cuda_dev):
    """tests/test_guarded_host.py on the device these tests use: one pad element written through torch fails check() and is named; the
    window full of data does not."""
    w, check = G.guarded(37, 31, 36, col0=4, device=cuda_dev)
    check()
    w.zero_()
    check()
    torch.as_strided(w, (1,), (1,), w.storage_offset() + 31).fill_(0.0)      # the element right of the first row
    with pytest.raises(AssertionError, match=r"^1 element\(s\) .* the first is row 2, column 35$"):
        check()
    s, check_s = G.guarded_split3(5, 16, 24, device=cuda_dev)
    s.fill_(1)
    check_s()
    torch.as_strided(s, (1,), (1,), s.storage_offset() - 1).fill_(1)        # the last pad element of the guard row in front
    with pytest.raises(AssertionError, match=r"the first is row 1, column 71$"):
        check_s()
    t, check_t = G.guarded_blocked(37, 16, device=cuda_dev)
    t[:1] = 1
    t[1, :, :, :5] = 1
    check_t()
    t[1, 0, 0, 5, 0] = 1                                                     # row 37: the first pad row
    with pytest.raises(AssertionError, match=r"the first is block 2, chunk 0, piece 0, row 5, element 0$"):
        check_t()


# ---- d. thmr_op_split3 ----
@gpu
@pytest.mark.parametrize("K", [8, 96])
@pytest.mark.parametrize("rows", [1, 37, 200])
def test_split3_conversion_strided(built_lib, cuda_dev, rows, K):
    ops = _ops()
    x = _rnd(cuda_dev, rows, K, seed=31)
    want = ops.split3(x)
    fails = []
    for ld_src in (K, K + 4):
        for ld_dst in (K, K + 8):
            ctx = f"split3 ({rows}, {K}) ld_src {ld_src} ld_dst {ld_dst}"
            x_g, cx = G.guarded(rows, K, ld_src, device=cuda_dev, fill=x)
            d_g, cd = G.guarded_split3(rows, K, ld_dst, device=cuda_dev)
            assert ops.split3(x_g, out=d_g) is d_g
            if not torch.equal(d_g, want):
                fails.append(f"{ctx}: differs from the contiguous conversion")
            intact([("src", cx), ("dst", cd)], ctx, fails)
    report(fails)


# ---- f. attention outputs in guard bands ----
ATTN = ([("fp32", v, B) for v, Bs in (("keysplit", (1, 2)), ("q64", (3,)), ("q192", (3,)), ("persistent", (11, 33))) for B in Bs] +
        [("split3", None, B) for B in (1, 3, 11)] +
        [("b16", (qt, out_split), B) for qt in (0, 1, 3) for out_split in (False, True) for B in (1, 3, 33)])
_QKV = {}


def _qkv(dev, B):
    """qkv (B, 192, 3840), q pre-scaled, contiguous and as a window with one whole NaN item (192 rows) before and after"""
    if B not in _QKV:
        q = _rnd(dev, B * 192, 3840, seed=400 + B)
        q[:, :1280] *= 80 ** -0.5
        q_g, cq = G.guarded(B * 192, 3840, 3840, before=192, after=192, device=dev, fill=q)
        _QKV.clear()
        _QKV[B] = (q.view(B, 192, 3840), q_g.view(B, 192, 3840), cq)
    return _QKV[B]


@gpu
@pytest.mark.parametrize("kind,arg,B", sorted(ATTN, key=lambda c: c[2]), ids=lambda x: str(x).replace(" ", ""))
def test_attention_output_in_guard_bands(built_lib, cuda_dev, kind, arg, B):
    """Each attention kernel writes into a window with one whole item (192 rows) of canary before and after, reading qkv from a window
    between NaN items: equal to the unguarded call, every guard row intact."""
    ops = _ops()
    q, q_g, cq = _qkv(cuda_dev, B)
    split = kind == "split3" or (kind == "b16" and arg[1])
    if split:
        o_g, co = G.guarded(B * 192, 3840, 3840, before=192, after=192, dtype=torch.int16, device=cuda_dev)
        out = o_g.view(B * 192, 160, 3, 8)
    else:
        o_g, co = G.guarded(B * 192, 1280, 1280, before=192, after=192, device=cuda_dev)
        out = o_g.view(B, 192, 1280)
    assert out.is_contiguous() and q_g.is_contiguous()
    if kind == "fp32":
        want, got = ops.vit_attention(q, variant=arg), ops.vit_attention(q_g, variant=arg, out=out)
    elif kind == "split3":
        want, got = ops.vit_attention_split3(q), ops.vit_attention_split3(q_g, out=out)
    else:
        want, got = ops.vit_attention_b16(q, out_split=arg[1], qt=arg[0]), ops.vit_attention_b16(q_g, out_split=arg[1], qt=arg[0], out=out)
    assert got is out
    fails = []
    if not torch.equal(out, want):
        fails.append("differs from the unguarded call")
    intact([("qkv", cq), ("out", co)], f"{kind} {arg} B {B}", fails)
    report(fails)


# ---- refusals: the wrappers and the operator ----
@gpu
def test_strided_refusals(built_lib, cuda_dev):
    """thmr_op_gemm with ldc = N - 1 raises EngineError and leaves the output buffer alone; the wrappers refuse what the ABI cannot
    express: a residual whose row stride is not the result's, rows of non-unit stride, a row stride below the columns."""
    import ctypes as C
    from tokenhmr_amd import ops, _cabi
    M, N, K = 37, 32, 64
    o = operands(cuda_dev, M, N, K, False)
    c_w, cc = G.guarded(M, N, N + 4, device=cuda_dev)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    L = _cabi.load()
    for bad, word in ((dict(ldc=N - 1), "ldc"), (dict(M=0), "M, N, K"), (dict(N=0), "M, N, K"), (dict(K=0), "M, N, K"), (dict(M=-3), "M, N, K")):
        a = dict(ldc=N + 4, M=M, N=N, K=K)
        a.update(bad)
        with torch.cuda.device(cuda_dev):
            rc = L.thmr_op_gemm(p(o.a), K, p(o.w), None, None, p(c_w), a["ldc"], a["M"], a["N"], a["K"], 0, 1.0, 0, -1, None)
        assert rc < 0 and word in (L.thmr_last_error(None) or b"").decode(), (bad, rc, L.thmr_last_error(None))
        with pytest.raises(_cabi.EngineError):
            _cabi.check(rc, None, L)
    torch.cuda.synchronize()
    cc()
    assert is_canary(c_w)
    r_w, _ = G.guarded(M, N, N + 8, device=cuda_dev, fill=o.resid)
    with pytest.raises(ValueError, match="row stride"):
        ops.gemm(o.a_g, o.w, o.bias, r_w, epi="bias_resid", out=c_w)                  # ldr != ldc
    with pytest.raises(ValueError, match="row stride"):
        ops.gemm(o.a_g, o.w, o.bias, r_w, epi="bias_resid")                           # a fresh result has ldc = N
    with pytest.raises(ValueError):
        ops.gemm(o.a.t()[:, :K], o.w)                                                 # stride(1) != 1
    with pytest.raises(ValueError):
        ops.gemm(o.a_g, o.w, out=torch.empty(M, 2 * N, device=cuda_dev)[:, ::2])      # stride(1) != 1
    with pytest.raises(ValueError):
        ops.gemm(o.a_g, o.w, out=torch.empty(M, N, device=cuda_dev, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.gemm(o.a_g.cpu(), o.w)
    with pytest.raises(ValueError):
        ops.gemm(torch.as_strided(o.a, (M, K), (K - 1, 1)), o.w)                      # overlapping rows: stride(0) < columns
    with pytest.raises(ValueError):
        ops.gemm(torch.as_strided(o.a_g, (M, K), (K + 6, 1)), o.w)                    # lda % 4 != 0
    s = operands(cuda_dev, M, N, K, True)
    with pytest.raises(ValueError):
        ops.gemm_split3(s.a_g[:, :, :, ::2], s.w)
    with pytest.raises(ValueError):
        ops.gemm_split3(s.a, s.w, out=torch.empty(M, N, device=cuda_dev), out_split=True)
    with pytest.raises(ValueError):
        ops.split3(o.a, out=torch.empty(M, K // 8, 3, 8, device=cuda_dev, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.vit_attention(torch.zeros(1, 192, 3840, device=cuda_dev), out=torch.empty(1, 192, 2560, device=cuda_dev)[:, :, ::2])
    with pytest.raises(ValueError):
        ops.vit_attention(torch.zeros(1, 192, 3840, device=cuda_dev), out=torch.empty(2, 192, 1280, device=cuda_dev))
    cc()
    assert is_canary(c_w)
