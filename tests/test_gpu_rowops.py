"""Per-kernel parity (-m gpu) of the row, glue and head kernels (csrc/rowops.hip, head.hip, hmr2_head.hip), each called alone through its
stateless entry point and compared with a plain torch statement written here: fp64 where there is arithmetic, exact fp32 / integer indexing
where the kernel only moves or adds.  Three kinds of assertion, named in every test:

  (E) exact      torch.equal — data movement, single fp32 additions in a fixed order, integer results.
  (B) bound      derived from the operation, formula at the check.
  (C) class      of torch's own fp32: err_hip <= max(4 * err_torch_fp32, floor), both against the same fp64 statement on the same inputs
                 (the convention of test_gpu_ops.py::test_vit_attention_keysplit / _b16; `_in_class` below prints both errors).  The floor is
                 the tolerance the project already uses for that operation (LayerNorm: atol 5e-6, rtol 1e-5; attention: 5e-6, peaked 2e-5);
                 for the softmax probabilities, where none existed, 4 x the measured error of torch's fp32 CPU statement (see there).

Shapes are the smallest that reach the edge in question: these kernels work on groups of four rows (one wave each), so 1 row, a partial last
group and a group boundary; every tie pattern of the two arg-reductions is constructed, not hoped for."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32
LN_FLOOR = dict(atol=5e-6, rtol=1e-5)          # test_gpu_ops.py::test_layernorm


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _in_class(tag, out, ref64, ref32, atol, rtol=0.0):
    """(C): True when `out` is in the class of torch's fp32 statement `ref32`, both measured against `ref64`."""
    out, ref32 = out.cpu().double(), ref32.double()
    err_hip, err_cpu = (out - ref64).abs().max().item(), (ref32 - ref64).abs().max().item()
    print(f"[{tag}] max|err| vs fp64: kernel {err_hip:.2e}, torch fp32 {err_cpu:.2e}")
    return bool(torch.isfinite(out).all()) and (err_hip <= 4 * err_cpu or bool(((out - ref64).abs() <= atol + rtol * ref64.abs()).all()))


def _ln64(x, g, b, eps):
    return F.layer_norm(x.double(), x.shape[-1:], g.double(), b.double(), eps)


def _first_index_of(values, target):
    """lowest column at which each row of `values` equals its `target` — stated without argmax / argmin"""
    n = values.shape[-1]
    cols = torch.arange(n).expand_as(values)
    return torch.where(values == target, cols, torch.full_like(cols, n)).min(-1).values.to(torch.int32)


# ------------------------------------------------------------------------------------------------ splitk_resid_ln
D = 1280


@functools.lru_cache(maxsize=None)
def _sk_inputs(rows, S, low_variance=False):
    """partials of scale 1 with outlier channels, residual of scale 3 (low_variance: a sum of standard deviation ~0.05, so that eps is
    not negligible beside the variance 2.5e-3).  The partial buffer holds one spare row behind the S slabs."""
    buf = _rand(S * rows * D + D, seed=10 * rows + S)
    part = buf[:S * rows * D].view(S, rows, D)
    bias, resid = _rand(D, seed=2), _rand(rows, D, seed=3, scale=3.0)
    if low_variance:         # var = S a^2 + 0.01^2 + r^2 = 2.5e-3
        part *= (8e-4 / S) ** 0.5
        bias, resid = bias * 0.01, resid * (0.04 / 3.0)
    else:
        part[:, :, ::7] *= 30
    gamma, beta = 1 + 0.1 * _rand(D, seed=4), 0.1 * _rand(D, seed=5)
    acc = part[0].clone()
    for s in range(1, S):          # the kernel's written order: (((p0 + p1) + p2) + ...), then + bias, then resid + (...)
        acc = acc + part[s]
    xref = resid + (acc + bias)
    return part, bias, resid, gamma, beta, xref, buf


def _sk_dev(t, dev):
    part, bias, resid, gamma, beta, _, buf = t
    big = buf.to(dev)          # the whole buffer, spare row included
    return big[:part.numel()].view(part.shape), bias.to(dev), resid.to(dev), gamma.to(dev), beta.to(dev)


@pytest.mark.parametrize("S", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("rows", [1, 7, 193])
def test_splitk_resid_ln(built_lib, cuda_dev, rows, S):
    """The fused split-K reduce + bias + residual + LayerNorm of the ViT residual stream: the ST = 2, ST = 4 and runtime-S instantiations,
    at one wave of a row group, a partial last group and a group boundary.
    xout (E) against the fp32 additions in the kernel's order; y (C) with the LayerNorm floor against fp64 LayerNorm of the kernel's own
    xout; split3 y (E) ops.split3 of the fp32 y; the engine's in-place call (resid is xout) (E) the out-of-place one; repeat (E).
    Observed on the MI355X, max|err| of y against fp64 over the 15 cases: kernel 5.0e-7 ... 1.7e-6, torch fp32 5.0e-7 ... 2.2e-6."""
    from tokenhmr_amd import ops
    t = _sk_inputs(rows, S)
    part, bias, resid, gamma, beta = _sk_dev(t, cuda_dev)
    xout, y = ops.splitk_resid_ln(part, bias, resid, gamma, beta, 1e-6)
    assert torch.equal(xout.cpu(), t[5])                                                              # (E)
    xk = xout.cpu()
    assert _in_class(f"splitk_resid_ln rows={rows} S={S}", y, _ln64(xk, t[3], t[4], 1e-6), F.layer_norm(xk, (D,), t[3], t[4], 1e-6), **LN_FLOOR)
    x2, y2 = ops.splitk_resid_ln(part, bias, resid, gamma, beta, 1e-6)
    assert torch.equal(x2, xout) and torch.equal(y2, y)                                               # repeat (E)
    r_in = resid.clone()
    x3, y3 = ops.splitk_resid_ln(part, bias, r_in, gamma, beta, 1e-6, inplace=True)
    assert x3.data_ptr() == r_in.data_ptr() and torch.equal(x3, xout) and torch.equal(y3, y)          # in place (E)
    if S in (2, 4):
        ys = ops.split3(y)
        x4, y4 = ops.splitk_resid_ln(part, bias, resid, gamma, beta, 1e-6, y_split3=True)
        assert torch.equal(x4, xout) and torch.equal(y4, ys)                                          # split3 y (E)
        r_in = resid.clone()
        x5, y5 = ops.splitk_resid_ln(part, bias, r_in, gamma, beta, 1e-6, y_split3=True, inplace=True)
        assert torch.equal(x5, xout) and torch.equal(y5, ys)


@pytest.mark.parametrize("S", [1, 2, 3, 4, 8])
def test_splitk_resid_ln_rows_do_not_depend_on_the_launch(built_lib, cuda_dev, S):
    """(E) the first 7 rows of a 193-row launch equal those 7 rows launched alone.  The slab stride rows * D differs between the two
    calls: a stride taken from anything but this launch's row count shows here."""
    from tokenhmr_amd import ops
    part, bias, resid, gamma, beta = _sk_dev(_sk_inputs(193, S), cuda_dev)
    p7 = torch.empty(S * 7 * D + D, device=cuda_dev)[:S * 7 * D].view(S, 7, D)          # one spare row behind the slabs here too
    p7.copy_(part[:, :7])
    r7 = resid[:7].contiguous()
    for split in ((False, True) if S in (2, 4) else (False,)):
        xa, ya = ops.splitk_resid_ln(part, bias, resid, gamma, beta, 1e-6, y_split3=split)
        xb, yb = ops.splitk_resid_ln(p7, bias, r7, gamma, beta, 1e-6, y_split3=split)
        assert torch.equal(xa[:7], xb) and torch.equal(ya[:7], yb), split


@pytest.mark.parametrize("S", [2, 3])
def test_splitk_resid_ln_tells_eps_1e6_from_1e5(built_lib, cuda_dev, S):
    """Rows of variance ~2.5e-3: eps 1e-6 against 1e-5 moves the result by ~1.8e-3 relative.  The eps = 1e-6 launch is (C) in class against
    the fp64 statement with eps = 1e-6 and NOT in class against the one with eps = 1e-5, so this file can tell the two apart.
    Observed on the MI355X (S = 2 / 3): kernel 3.7e-7 / 3.9e-7, torch fp32 3.7e-7 / 5.2e-7; against the eps = 1e-5 statement 6.9e-3 / 8.9e-3."""
    from tokenhmr_amd import ops
    t = _sk_inputs(7, S, low_variance=True)
    part, bias, resid, gamma, beta = _sk_dev(t, cuda_dev)
    xout, y = ops.splitk_resid_ln(part, bias, resid, gamma, beta, 1e-6)
    assert torch.equal(xout.cpu(), t[5])                                                              # (E)
    xk = xout.cpu()
    assert 2e-3 < xk.var(-1, unbiased=False).mean().item() < 3e-3
    assert _in_class(f"splitk_resid_ln low variance S={S} eps 1e-6", y, _ln64(xk, t[3], t[4], 1e-6), F.layer_norm(xk, (D,), t[3], t[4], 1e-6), **LN_FLOOR)
    assert not _in_class(f"splitk_resid_ln low variance S={S} against eps 1e-5", y, _ln64(xk, t[3], t[4], 1e-5),
                         F.layer_norm(xk, (D,), t[3], t[4], 1e-5), **LN_FLOOR)


def test_layernorm_1280_tells_eps_1e6_from_1e5(built_lib, cuda_dev):
    """The same check for ops.layernorm at D = 1280 (the one-wave-per-row kernel): (C) in class for the eps it was given, not for the other.
    Observed on the MI355X: kernel 8.2e-7, torch fp32 7.1e-7; against the eps = 1e-5 statement 7.8e-3."""
    from tokenhmr_amd import ops
    x = _rand(7, D, seed=31, scale=0.05) + 0.3
    g, b = 1 + 0.1 * _rand(D, seed=4), 0.1 * _rand(D, seed=5)
    y = ops.layernorm(x.to(cuda_dev), g.to(cuda_dev), b.to(cuda_dev), 1e-6)
    assert _in_class("layernorm 1280 low variance eps 1e-6", y, _ln64(x, g, b, 1e-6), F.layer_norm(x, (D,), g, b, 1e-6), **LN_FLOOR)
    assert not _in_class("layernorm 1280 low variance against eps 1e-5", y, _ln64(x, g, b, 1e-5), F.layer_norm(x, (D,), g, b, 1e-5), **LN_FLOOR)


# ------------------------------------------------------------------------------------------------ add_ln64
@pytest.mark.parametrize("rows", [1, 6, 161])
def test_add_ln64(built_lib, cuda_dev, rows):
    """MixerLayer's layernorm2(x + y): s (E) x + y; z (C) with the LayerNorm floor against fp64 LayerNorm (eps 1e-5) of that sum.
    Observed on the MI355X (1 / 6 / 161 rows): kernel 2.0e-7 / 2.7e-7 / 5.1e-7, torch fp32 1.9e-7 / 3.5e-7 / 5.1e-7."""
    from tokenhmr_amd import ops
    x, y = _rand(rows, 64, seed=40, scale=3.0) + 0.7, _rand(rows, 64, seed=41)
    g, b = 1 + 0.1 * _rand(64, seed=42), 0.1 * _rand(64, seed=43)
    s, z = ops.add_ln64(x.to(cuda_dev), y.to(cuda_dev), g.to(cuda_dev), b.to(cuda_dev), 1e-5)
    sref = x + y
    assert torch.equal(s.cpu(), sref)                                                                 # (E)
    assert _in_class(f"add_ln64 rows={rows}", z, _ln64(sref, g, b, 1e-5), F.layer_norm(sref, (64,), g, b, 1e-5), **LN_FLOOR)


# ------------------------------------------------------------------------------------------------ softmax + argmax over 2048
# Column 4 * (i * 64 + lane) + e lives in lane `lane`, register slot (i, e).  (columns holding the row maximum, expected index)
TIES = [((8, 10), 8),                # inside one lane's four consecutive values
        ((8, 12), 8),                # two lanes of the same wave
        ((8, 8 + 256), 8),           # two register groups of one lane
        ((2047, 0), 0),              # the last column and the first
        ((2047,), 2047),             # the maximum at 2047 only
        ((12, 256), 12),             # the LARGER index sits in the LOWER lane (256: lane 0, 12: lane 3): the cross-lane step must compare indices
        ((256, 12, 8 + 256), 12),
        (tuple(range(2048)), 0)]     # an all-equal row


def _tie_rows(fill, peak):
    rows = torch.empty(len(TIES), 2048)
    for r, (cols, _) in enumerate(TIES):
        rows[r] = fill - torch.rand(2048, generator=torch.Generator().manual_seed(50 + r))          # every other value strictly worse
        rows[r, list(cols)] = peak
    return rows, torch.tensor([w for _, w in TIES], dtype=torch.int32)


@pytest.mark.parametrize("rows", [1, 5, 640])
def test_softmax_argmax_index_is_the_first_maximum(built_lib, cuda_dev, rows):
    """idx (E) the first index attaining the row maximum of the input logits, no exclusions; probs=None and idx=None give the same other
    output (E); repeat (E)."""
    from tokenhmr_amd import ops
    logits = _rand(rows, 2048, seed=60 + rows)
    logits[:, 1000] = logits[:, 3]                    # duplicates that are the maximum only by chance
    d = logits.to(cuda_dev)
    probs, idx = ops.softmax_argmax(d)
    assert torch.equal(idx.cpu(), _first_index_of(logits, logits.max(-1, keepdim=True).values))      # (E)
    p_only, none_i = ops.softmax_argmax(d, idx=False)
    none_p, i_only = ops.softmax_argmax(d, probs=False)
    assert none_i is None and none_p is None and torch.equal(p_only, probs) and torch.equal(i_only, idx)
    p2, i2 = ops.softmax_argmax(d)
    assert torch.equal(p2, probs) and torch.equal(i2, idx)


def test_softmax_argmax_exact_ties_take_the_lowest_index(built_lib, cuda_dev):
    """thmr_outputs.token_idx: "lowest index on ties" — (E) on constructed exact ties: within a lane, across lanes, across register groups,
    2047 against 0, an all-equal row, and a larger index in a lower lane."""
    from tokenhmr_amd import ops
    logits, want = _tie_rows(0.0, 5.0)
    assert torch.equal(_first_index_of(logits, logits.max(-1, keepdim=True).values), want)
    _, idx = ops.softmax_argmax(logits.to(cuda_dev), probs=False)
    assert torch.equal(idx.cpu(), want), idx.cpu().tolist()
    # the same rows at another position of the four-row group, and among random rows
    both = torch.cat([_rand(3, 2048, seed=59), logits, _rand(2, 2048, seed=58)])
    _, idx = ops.softmax_argmax(both.to(cuda_dev), probs=False)
    assert torch.equal(idx.cpu()[3:3 + len(TIES)], want)


# floor of the softmax probabilities: no tolerance existed.  torch's fp32 CPU softmax against fp64 on these inputs measures 9.0e-10
# (scale 1, probabilities <= 0.01) and 6.4e-8 (scale 30, probabilities up to 1): the floor is 4 x that.
@pytest.mark.parametrize("scale,floor", [(1.0, 4 * 9.0e-10), (30.0, 4 * 6.4e-8)])
def test_softmax_probs(built_lib, cuda_dev, scale, floor):
    """probs (C) against fp64 softmax at logits of scale 1 and 30 (peaked); every row sums to 1 within 1e-5 (B): at most 32 sequential
    plus 6 tree additions per lane in front of the divide, <= ~40 * 2^-24 = 2.4e-6, with margin.
    Observed on the MI355X (the torch figures are the same there as on the development host): scale 1 kernel 5.7e-10, torch fp32 9.05e-10;
    scale 30 kernel 1.2e-7, torch fp32 6.4e-8."""
    from tokenhmr_amd import ops
    logits = _rand(5, 2048, seed=70, scale=scale)
    probs, _ = ops.softmax_argmax(logits.to(cuda_dev))
    assert _in_class(f"softmax probs scale={scale}", probs, logits.double().softmax(-1), logits.softmax(-1), atol=floor)
    assert (probs.cpu().double().sum(-1) - 1).abs().max().item() <= 1e-5                              # (B)


def test_softmax_probs_of_a_one_hot_row_are_exact(built_lib, cuda_dev):
    """A row whose entries other than one are -inf gives exactly 1.0 there and 0.0 elsewhere (E); so do the tie rows sum to 1 (B)."""
    from tokenhmr_amd import ops
    logits = torch.full((6, 2048), float("-inf"))
    hot = torch.tensor([0, 3, 255, 256, 1029, 2047])
    logits[torch.arange(6), hot] = torch.tensor([0.0, -3.5, 80.0, 1e4, -1e4, 2.0])
    probs, idx = ops.softmax_argmax(logits.to(cuda_dev))
    assert torch.equal(probs.cpu(), F.one_hot(hot, 2048).float()) and torch.equal(idx.cpu(), hot.int())     # (E)
    ties, _ = _tie_rows(0.0, 5.0)
    probs, _ = ops.softmax_argmax(ties.to(cuda_dev))
    assert (probs.cpu().double().sum(-1) - 1).abs().max().item() <= 1e-5
    assert torch.equal(probs[-1].cpu(), torch.full((2048,), 1.0 / 2048))          # the all-equal row: 1 / 2048 is exact


# ------------------------------------------------------------------------------------------------ vq_argmin_rows, code_norm
@pytest.mark.parametrize("rows", [1, 6, 161])
def test_vq_argmin_rows(built_lib, cuda_dev, rows):
    """dist (B): |dist - fp64| <= 16 * 2^-24 * (|x|^2 + 2 |dot| + cnorm) elementwise — the row norm is a 4-term sum plus a 6-level tree,
    then two more roundings.  idx (E) the first index attaining the minimum of the kernel's OWN dist row, no exclusions; dist=None gives
    the same idx (E)."""
    from tokenhmr_amd import ops
    x, cb = _rand(rows, 256, seed=80 + rows), _rand(2048, 256, seed=81)
    cb[700] = cb[5]                                   # a duplicated code: equal distances wherever the arithmetic is the same
    dot, cnorm = x @ cb.t(), (cb * cb).sum(-1)
    idx, dist = ops.vq_argmin_rows(x.to(cuda_dev), dot.to(cuda_dev), cnorm.to(cuda_dev))
    dist = dist.cpu()
    xn = (x.double() ** 2).sum(-1, keepdim=True)
    ref = (xn - 2 * dot.double()) + cnorm.double()
    bound = 16 * U * (xn + 2 * dot.double().abs() + cnorm.double())
    assert ((dist.double() - ref).abs() <= bound).all(), ((dist.double() - ref).abs() / bound).max()  # (B)
    assert torch.equal(idx.cpu(), _first_index_of(dist, dist.min(-1, keepdim=True).values))           # (E)
    idx2, none = ops.vq_argmin_rows(x.to(cuda_dev), dot.to(cuda_dev), cnorm.to(cuda_dev), want_dist=False)
    assert none is None and torch.equal(idx2, idx)


def test_vq_argmin_exact_ties_take_the_lowest_index(built_lib, cuda_dev):
    """vq_argmin_kernel: "lowest-index tie-break" — x = 0 and dot = 0 make dist == cnorm (E), and cnorm is a table with its minimum
    duplicated at the same index patterns as the softmax ties; the lowest index wins (E), with and without the dist output."""
    from tokenhmr_amd import ops
    tables, want = _tie_rows(0.0, 5.0)          # _tie_rows marks the maximum: mirror it into a minimum of 2 under values in [7, 8)
    tables = 7.0 - tables
    x, dot = torch.zeros(5, 256, device=cuda_dev), torch.zeros(5, 2048, device=cuda_dev)
    for r, (cols, w) in enumerate(TIES):
        cn = tables[r]
        assert _first_index_of(cn[None], cn.min()).item() == w == want[r].item() and (cn[list(cols)] == cn.min()).all()
        idx, dist = ops.vq_argmin_rows(x, dot, cn.to(cuda_dev))
        assert torch.equal(dist.cpu(), cn.expand(5, 2048)), cols                                      # (E)
        assert idx.cpu().tolist() == [w] * 5, (cols, idx.cpu().tolist())                              # (E)
        idx2, _ = ops.vq_argmin_rows(x, dot, cn.to(cuda_dev), want_dist=False)
        assert torch.equal(idx2, idx)


@pytest.mark.parametrize("ncode", [5, 2048])
def test_code_norm(built_lib, cuda_dev, ncode):
    """(B) |cn - fp64| <= 10 * 2^-24 * sum(c^2): one rounding per square, a 4-term sum and a 6-level tree."""
    from tokenhmr_amd import ops
    cb = _rand(ncode, 256, seed=90, scale=0.3)
    cn = ops.code_norm(cb.to(cuda_dev)).cpu().double()
    ref = (cb.double() ** 2).sum(-1)
    assert ((cn - ref).abs() <= 10 * U * ref).all(), ((cn - ref).abs() / ref).max()


# ------------------------------------------------------------------------------------------------ cross_attn
def _cross_attn_ref(q, kv, koff):
    B = q.shape[0]
    k = kv[:, koff:koff + 512].reshape(B, 192, 8, 64)
    v = kv[:, koff + 512:koff + 1024].reshape(B, 192, 8, 64)
    a = (torch.einsum("bhd,bjhd->bhj", q.reshape(B, 8, 64), k) * 0.125).softmax(-1)
    return torch.einsum("bhj,bjhd->bhd", a, v).reshape(B, 512)


@pytest.mark.parametrize("ldkv,koff", [(6 * 1024, 0), (6 * 1024, 5 * 1024), (1024, 0)])
@pytest.mark.parametrize("B", [1, 3])
def test_cross_attn(built_lib, cuda_dev, B, ldkv, koff):
    """One-query cross attention over the 192 context rows, with the engine's strides (six layers' K | V side by side, first and last
    layer) and the smallest legal one.  Everything outside the addressed 1024 columns is NaN, so a wrong stride or offset reads it.
    (C) with the attention floors (5e-6; peaked scores, q and k x 6: 2e-5); finite; repeat (E); crop 0 alone (E) crop 0 of the batch.
    Observed on the MI355X, the same for every stride (B = 1 / 3): scale 1 kernel 1.1e-7 / 1.6e-7, torch fp32 1.5e-7 / 2.2e-7; peaked
    kernel 3.1e-6 / 1.6e-5, torch fp32 1.2e-6 / 1.6e-5."""
    from tokenhmr_amd import ops
    for scale, floor in ((1.0, 5e-6), (6.0, 2e-5)):
        q = _rand(B, 512, seed=100 + B) * scale
        kv = torch.full((B * 192, ldkv), float("nan"))
        kv[:, koff:koff + 1024] = _rand(B * 192, 1024, seed=101 + B)
        kv[:, koff:koff + 512] *= scale
        dq, dkv = q.to(cuda_dev), kv.to(cuda_dev)
        out = ops.cross_attn(dq, dkv, koff)
        assert _in_class(f"cross_attn B={B} ldkv={ldkv} koff={koff} scale={scale}", out, _cross_attn_ref(q.double(), kv.double(), koff),
                         _cross_attn_ref(q, kv, koff), atol=floor)
        assert torch.equal(ops.cross_attn(dq, dkv, koff), out)
        assert torch.equal(ops.cross_attn(dq[:1].contiguous(), dkv[:192].contiguous(), koff), out[:1])


# ------------------------------------------------------------------------------------------------ transpose
@pytest.mark.parametrize("shape", [(3, 160, 64), (2, 64, 160), (1, 33, 31), (1, 2048, 256)])
def test_transpose(built_lib, cuda_dev, shape):
    """(E) on an arange input (any index error shows) into a NaN-filled output (any unwritten element shows)."""
    from tokenhmr_amd import ops
    Bn, R, C = shape
    x = torch.arange(Bn * R * C, dtype=torch.float32).reshape(Bn, R, C)
    out = torch.full((Bn, C, R), float("nan"), device=cuda_dev)
    assert ops.transpose(x.to(cuda_dev), out=out) is out
    assert torch.equal(out.cpu(), x.transpose(1, 2).contiguous())


# ------------------------------------------------------------------------------------------------ im2col_patch
@pytest.mark.parametrize("B", [1, 2])
def test_im2col_patch(built_lib, cuda_dev, B):
    """The patch-embed operand: (E) F.unfold of the zero-padded SLICED window on an image whose pixels are all distinct and non-zero
    (1 ... B * 196608, exact in fp32); the split3 form (E) ops.split3 of the fp32 form.  Spelled out: the two leading pad columns of patch
    column 0 and pad rows of patch row 0 are zero and nothing else is (the right-hand pad is never reached: patch column 11 ends at window
    column 189), the window's neighbours (image columns 30, 31, 224, 225) and the last two image rows (254, 255: 16 patches of the
    260 padded rows use rows -2 ... 253) never appear."""
    from tokenhmr_amd import ops
    img = (torch.arange(B * 3 * 256 * 256, dtype=torch.float32) + 1).reshape(B, 3, 256, 256)
    ref = F.unfold(F.pad(img[:, :, :, 32:-32], (2, 2, 2, 2)), 16, stride=16).transpose(1, 2).reshape(B * 192, 768).contiguous()
    d = img.to(cuda_dev)
    A = ops.im2col_patch(d)
    assert torch.equal(A.cpu(), ref)                                                                  # (E)
    assert torch.equal(ops.im2col_patch(d, out_split=True), ops.split3(A))                            # (E)
    a = A.cpu().reshape(B, 16, 12, 3, 16, 16)          # b, py, px, c, ky, kx
    zero = torch.zeros(B, 16, 12, 3, 16, 16, dtype=torch.bool)
    zero[:, :, 0, :, :, :2] = True
    zero[:, 0, :, :, :2, :] = True
    assert torch.equal(a == 0, zero)
    seen = torch.zeros(B * 3 * 256 * 256 + 1, dtype=torch.bool)
    seen[A.cpu().long().flatten()] = True
    seen = seen[1:].reshape(B, 3, 256, 256)
    want = torch.zeros(256, 256, dtype=torch.bool)
    want[:254, 32:222] = True                          # rows 0 ... 253, window columns 0 ... 189
    assert torch.equal(seen, want.expand(B, 3, 256, 256))


# ------------------------------------------------------------------------------------------------ conv gathers and repacks
def _nearest_table(tin, tout):
    """nn.Upsample(size, mode="nearest") source indices, built as the engine's build_idx_tables does (fp32 scale, floor, clamp)"""
    scale = torch.tensor(tin, dtype=torch.float32) / torch.tensor(tout, dtype=torch.float32)
    return torch.clamp(torch.floor(torch.arange(tout, dtype=torch.float32) * scale).to(torch.int32), max=tin - 1)


def _conv3_gather_ref(x, src, Tout, dil, prerelu):
    Bn, _, C = x.shape
    f = F.relu(x) if prerelu else x
    src = torch.arange(Tout) if src is None else src.long()
    out = torch.zeros(Bn, Tout, 3, C)
    for dk in range(3):
        tp = torch.arange(Tout) + (dk - 1) * dil
        ok = (tp >= 0) & (tp < Tout)
        out[:, ok, dk] = f[:, src[tp[ok]]]
    return out.reshape(Bn, Tout, 3 * C)


def _conv_gather_ref(x, src, Tsrc, Tout, Cp, ks, stride, pad):
    Bn, _, C = x.shape
    src = torch.arange(Tsrc) if src is None else src.long()
    out = torch.zeros(Bn, Tout, ks, Cp)
    for kk in range(ks):
        tp = torch.arange(Tout) * stride - pad + kk
        ok = (tp >= 0) & (tp < Tsrc)
        out[:, ok, kk, :C] = x[:, src[tp[ok]]]
    return out.reshape(Bn, Tout, ks * Cp)


@pytest.mark.parametrize("prerelu", [False, True])
@pytest.mark.parametrize("dil", [1, 3, 9, 27])
@pytest.mark.parametrize("table", ["none", "identity", "upsample"])
def test_conv3_gather(built_lib, cuda_dev, table, dil, prerelu):
    """(E) against the indexing statement, into a NaN-filled output: Bn = 2, C = 8, Tout = 10; no table, the identity table, the nearest
    up-sampling table 5 -> 10; every dilation of the decoder (27 >= Tout: both side taps are all zero); pre-ReLU on and off."""
    from tokenhmr_amd import ops
    Tin, Tout = (5, 10) if table == "upsample" else (10, 10)
    src = None if table == "none" else _nearest_table(Tin, Tout)
    if table == "upsample":
        assert src.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    x = _rand(2, Tin, 8, seed=110)
    out = torch.full((2, Tout, 24), float("nan"), device=cuda_dev)
    ops.conv3_gather(x.to(cuda_dev), Tout, None if src is None else src.to(cuda_dev), dil, prerelu, out=out)
    ref = _conv3_gather_ref(x, src, Tout, dil, prerelu)
    assert torch.equal(out.cpu(), ref)
    if dil == 27:
        assert not ref[:, :, :8].any() and not ref[:, :, 16:].any()


# (C, Cp, ks, stride, pad, Tin, Tsrc, Tout, table): the encoder's two real configurations, and the strided one behind a resampling table
CONV_GATHER_CASES = [(6, 32, 3, 1, 1, 10, 10, 10, False), (8, 8, 4, 2, 1, 20, 20, 10, False), (8, 8, 4, 2, 1, 10, 20, 10, True)]


@pytest.mark.parametrize("case", CONV_GATHER_CASES)
def test_conv_gather(built_lib, cuda_dev, case):
    """(E) against the indexing statement, into a NaN-filled output (the padded channels C ... Cp - 1 must be written as zeros)."""
    from tokenhmr_amd import ops
    C, Cp, ks, stride, pad, Tin, Tsrc, Tout, table = case
    src = _nearest_table(Tin, Tsrc) if table else None
    x = _rand(2, Tin, C, seed=120)
    out = torch.full((2, Tout, ks * Cp), float("nan"), device=cuda_dev)
    ops.conv_gather(x.to(cuda_dev), Tout, ks, stride, pad, Cp=Cp, src=None if src is None else src.to(cuda_dev), Tsrc=Tsrc, out=out)
    assert torch.equal(out.cpu(), _conv_gather_ref(x, src, Tsrc, Tout, Cp, ks, stride, pad))


def _repack_ref(w, cp):
    co, ci, kk = w.shape
    out = torch.zeros(co, kk, cp)
    out[:, :, :ci] = w.permute(0, 2, 1)
    return out.reshape(co, kk * cp)


@pytest.mark.parametrize("co,ci,cp,kk", [(16, 32, 32, 3), (5, 8, 8, 4), (16, 6, 32, 3), (3, 5, 7, 1)])
def test_conv_repack(built_lib, cuda_dev, co, ci, cp, kk):
    """(E) against w.permute(0, 2, 1), zero-padded to cp channels."""
    from tokenhmr_amd import ops
    w = _rand(co, ci, kk, seed=130)
    assert torch.equal(ops.conv_repack(w.to(cuda_dev), cp).cpu(), _repack_ref(w, cp))


@pytest.mark.parametrize("case", ["k3/d1", "k3/d3", "k3/d9", "k3/d27", "k4/s2", "k3/pad6to32"])
def test_gather_and_repack_make_a_conv1d(built_lib, cuda_dev, case):
    """The layout contract BETWEEN gather and repack: gemm(gather(x), repack(w), bias) is F.conv1d in fp64 (channels-last against
    channels-first handled here), at the GEMM tolerance of test_gpu_ops.py (atol 3e-5, rtol 1e-5).  K = ks * Cp is a multiple of 32."""
    from tokenhmr_amd import ops
    co, Bn = 16, 2
    if case.startswith("k3/d"):
        dil, C, T = int(case[4:]), 32, 10
        x, w = _rand(Bn, T, C, seed=140), _rand(co, C, 3, seed=141, scale=0.1)
        a = ops.conv3_gather(x.to(cuda_dev), T, None, dil)
        conv = dict(padding=dil, dilation=dil)
        wp = ops.conv_repack(w.to(cuda_dev))
    elif case == "k4/s2":
        C, T = 8, 10
        x, w = _rand(Bn, 2 * T, C, seed=142), _rand(co, C, 4, seed=143, scale=0.2)
        a = ops.conv_gather(x.to(cuda_dev), T, 4, 2, 1)
        conv = dict(stride=2, padding=1)
        wp = ops.conv_repack(w.to(cuda_dev))
    else:
        C, T = 6, 10
        x, w = _rand(Bn, T, C, seed=144), _rand(co, C, 3, seed=145, scale=0.2)
        a = ops.conv_gather(x.to(cuda_dev), T, 3, 1, 1, Cp=32)
        conv = dict(padding=1)
        wp = ops.conv_repack(w.to(cuda_dev), 32)
    bias = _rand(co, seed=146)
    assert a.shape[-1] == wp.shape[1] and wp.shape[1] % 32 == 0
    out = ops.gemm(a.reshape(Bn * T, -1), wp, bias.to(cuda_dev), epi="bias").cpu().reshape(Bn, T, co)
    ref = F.conv1d(x.double().transpose(1, 2), w.double(), bias.double(), **conv).transpose(1, 2)
    assert ref.shape == out.shape
    assert torch.allclose(out.double(), ref, atol=3e-5, rtol=1e-5), (out.double() - ref).abs().max()


# ------------------------------------------------------------------------------------------------ head_finish, decoder_init
FOCAL, IMG = 5000.0, 256.0
HEADS = {"token": (32, slice(6, 16), slice(16, 19)), "hmr2": (160, slice(144, 154), slice(154, 157))}      # ldro, shape columns, cam columns


def _head_inputs(kind, B, degenerate):
    ld = HEADS[kind][0]
    ro, bpose = _rand(B, ld, seed=150 + B), (_rand(B, 126, seed=151) if kind == "token" else None)
    ip, ib, ic = _rand(144, seed=152), _rand(10, seed=153), _rand(3, seed=154) + 2.0
    ro[0, HEADS[kind][2].start] = -ic[0]                    # crop 0: cam0 == 0 exactly, the 1e-9 guard alone divides
    if degenerate:                                          # joint 3 of every crop: a1 == 0 exactly
        if kind == "token":
            bpose[:, 12:15] = -ip[18:21]
        else:
            ro[:, 18:21] = -ip[18:21]
    return ro, bpose, ip, ib, ic


def _pose6d_ref(kind, ro, bpose, ip):
    return (torch.cat([ro[:, :6], bpose, ro[:, 19:31]], 1) if kind == "token" else ro[:, :144]) + ip


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("kind", ["token", "hmr2"])
def test_head_finish(built_lib, cuda_dev, kind, B):
    """The finish behind the read-out GEMM, both heads, with the engine's ldro (32 / 160) and a read-out whose columns are all distinct:
    pose6d, betas, cam (E) the fp32 additions with the column map of the kernel comments; rotmat within 1e-6 of the oracle's
    rot6d_to_rotmat(pose6d) (test_rot6d's tolerance), orthonormal with det 1 to 1e-5; cam_t (B) rtol 1e-6 against the fp64 formula,
    cam0 == 0 included (the 1e-9 guard gives a finite 1e13); focal (E); the optional outputs passed as null leave the others unchanged (E)."""
    from tokenhmr_amd import ops
    from oracle import tokenhmr_oracle as O
    ro, bpose, ip, ib, ic = _head_inputs(kind, B, False)
    dev = lambda t: None if t is None else t.to(cuda_dev)
    o = ops.head_finish(kind, dev(ro), dev(ip), dev(ib), dev(ic), bpose=dev(bpose), focal_length=FOCAL, img_size=IMG)
    p6 = _pose6d_ref(kind, ro, bpose, ip)
    assert torch.equal(o["pose6d"].cpu(), p6)                                                         # (E)
    assert torch.equal(o["betas"].cpu(), ro[:, HEADS[kind][1]] + ib)                                  # (E)
    cam = ro[:, HEADS[kind][2]] + ic
    assert torch.equal(o["cam"].cpu(), cam) and cam[0, 0] == 0                                        # (E)
    R = o["rotmat"].cpu()
    assert torch.allclose(R, O.rot6d_to_rotmat(p6).reshape(B, 24, 3, 3), atol=1e-6)
    assert torch.allclose(R @ R.transpose(-1, -2), torch.eye(3).expand_as(R), atol=1e-5)
    assert torch.allclose(torch.linalg.det(R), torch.ones(B, 24), atol=1e-5)
    c = cam.double()
    cam_t = torch.stack([c[:, 1], c[:, 2], 2 * FOCAL / (IMG * c[:, 0] + 1e-9)], 1)
    got = o["cam_t"].cpu()
    assert torch.isfinite(got).all() and ((got.double() - cam_t).abs() <= 1e-6 * cam_t.abs()).all()   # (B)
    assert torch.equal(o["focal"].cpu(), torch.full((B, 2), FOCAL))                                   # (E)
    bare = ops.head_finish(kind, dev(ro), dev(ip), dev(ib), dev(ic), bpose=dev(bpose), focal_length=FOCAL, img_size=IMG,
                           want_pose6d=False, want_cam_t=False, want_focal=False)
    assert bare["pose6d"] is None and bare["cam_t"] is None and bare["focal"] is None
    for k in ("rotmat", "betas", "cam"):
        assert torch.equal(bare[k], o[k]), k


@pytest.mark.parametrize("kind", ["token", "hmr2"])
def test_head_finish_degenerate_joint(built_lib, cuda_dev, kind):
    """A joint whose first 6D vector is exactly zero follows F.normalize's eps (b1 = 0 / 1e-12 = 0, b3 = 0): finite, and equal to the
    oracle within 1e-6; the other joints stay orthonormal."""
    from tokenhmr_amd import ops
    from oracle import tokenhmr_oracle as O
    ro, bpose, ip, ib, ic = _head_inputs(kind, 2, True)
    dev = lambda t: None if t is None else t.to(cuda_dev)
    o = ops.head_finish(kind, dev(ro), dev(ip), dev(ib), dev(ic), bpose=dev(bpose), focal_length=FOCAL, img_size=IMG)
    p6 = _pose6d_ref(kind, ro, bpose, ip)
    assert torch.equal(o["pose6d"].cpu(), p6) and not p6.reshape(2, 24, 6)[:, 3, :3].any()
    R = o["rotmat"].cpu()
    assert torch.isfinite(R).all()
    assert torch.allclose(R, O.rot6d_to_rotmat(p6).reshape(2, 24, 3, 3), atol=1e-6)
    assert not R[:, 3, 0].any() and not R[:, 3, 2].any()
    keep = [j for j in range(24) if j != 3]
    assert torch.allclose(R[:, keep] @ R[:, keep].transpose(-1, -2), torch.eye(3).expand(2, 23, 3, 3), atol=1e-5)


@pytest.mark.parametrize("B,E", [(3, 100), (1, 1024), (5, 1024)])
def test_decoder_init(built_lib, cuda_dev, B, E):
    """(E) bias + pos broadcast over the crops; B * E = 300 is no multiple of the 256-thread block."""
    from tokenhmr_amd import ops
    bias, pos = _rand(E, seed=160), _rand(E, seed=161)
    assert torch.equal(ops.decoder_init(bias.to(cuda_dev), pos.to(cuda_dev), B).cpu(), (bias + pos).expand(B, E))
