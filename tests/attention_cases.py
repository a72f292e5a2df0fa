"""Structured inputs, the float64 reference and the per-element metric for the ViT attention kernels (tests/test_attention_cases_host.py
on the CPU, tests/test_gpu_attention_edges.py on the device).  A plain module: no fixtures, no pytest hooks, importable without a GPU.

One crop is q, k of shape (16 heads, 192, 80), q ALREADY scaled (the qkv GEMM's epilogue does that in the engine; the kernels apply no
scale).  Seven constructions put the structure the kernels are built around where it carries weight: 16-key score tiles and 96-key halves
(fp32 MFMA kernels), 48 keys per wave (key-split kernel), three 64-key blocks under a running maximum and 32-key k-steps (bf16-pipe kernel).

The output dimension is 80, so three one-hot V settings (`probe_v`) read the whole 192 x 192 probability matrix out of a kernel through
its own P.V path: out[i, h*80 + d] = P[i, 80 c + d].  1.0 is a single bf16 piece, so a three-piece kernel reads out exactly too.

Metric: with s64 the float64 scores, m_i their row maximum, P64 = softmax(s64), A_i = max_j sum_d |q_id k_jd| (what a dot product's
rounding scales with) and t_ij = (s64_ij - m_i) log2 e (what an exponent argument's rounding scales with),

    u_ij = |P - P64| / (P64 (A_i + |t_ij| + 1)) 2^24        wherever P64 >= 2^-100;

below that the kernel's value must be <= 2^-99 in magnitude.  At most 1 % of a case may lie below: `reference` asserts it on the float64
side, so nothing passes by masking.  An element passes if

    |P - P64| <= P64 2^-24 max(4, mult u_ref (A_i + |t_ij| + 1))

with u_ref the largest u of the plain fp32 statement (q @ k^T).softmax(-1) ON THE SAME BITS — the shape of tests/stage_bounds.py."""
import math

import torch

NH, NTOK, HD = 16, 192, 80
CASES = ("gauss", "peaked", "rising", "falling", "edge_onehot", "uniform", "zero_q")
# one key on each side of every boundary the three kernels have: 16-key tiles, 48-key wave slices, 64-key blocks, the 96-key half
EDGE = (0, 15, 16, 47, 48, 63, 64, 95, 96, 127, 128, 143, 144, 191)

ULP = 2.0 ** -24
P_MIN = 2.0 ** -100            # the metric is taken where P64 >= P_MIN ...
P_BELOW_MAX = 2.0 ** -99       # ... and below it the kernel's value is held to this, absolutely
MASK_CAP = 0.01                # share of a case that may lie below P_MIN
FLOOR_UNITS = 4.0              # no element needs to be closer than 4 units
MULT_MAX = 4.0                 # what the older attention tests grant (4 * err_cpu); tests/test_attention_cases_host.py holds the mutants to fail AT this
ROWSUM_ULPS = 32               # V = 1: |out - 1| <= 32 ulp.  torch's normalise-first statement is 4 ... 26 ulp off (26 on `uniform`: 192 x fl(1/192))
ONEHOT_V_UNITS = 4             # V side on `edge_onehot`: three-piece v, the accumulate, the reciprocal product, one to spare


def _gauss(seed):
    """One crop's q, k, v ~ N(0,1), each (16, 192, 80), from the seed alone."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(NTOK, 3, NH, HD, generator=g).permute(1, 2, 0, 3).contiguous()
    return t[0], t[1], t[2]


def crop(name, seed):
    """q, k (16, 192, 80) of one case."""
    q, k, _ = _gauss(seed)
    q = q * HD ** -0.5
    j = torch.arange(NTOK)
    if name == "gauss":
        pass
    elif name == "peaked":                     # scores x 9: 0.003 % of the probabilities below 2^-100 (x 36, as the older tests use, puts 77 % there)
        q, k = 3.0 * q, 3.0 * k
    elif name in ("rising", "falling"):        # every 16-key tile's maximum 3 above (below) the previous tile's
        ramp = 3.0 * (j // 16).float()
        q[:, :, 0] = 1.0
        k[:, :, 0] = ramp if name == "rising" else ramp.flip(0)
    elif name == "edge_onehot":                # +49 on exactly one key per query, the key on a boundary, the assignment turned per head
        q[:, :, :14] = 0.0
        k[:, :, :14] = 0.0
        for h in range(NH):
            for c, e in enumerate(EDGE):
                q[h, c::14, (c + h) % 14] = 7.0
                k[h, e, (c + h) % 14] = 7.0
    elif name == "uniform":                    # P = 1/192 exactly: any key-dependent error stands alone
        k = k[:, :1].expand(NH, NTOK, HD).contiguous()
    elif name == "zero_q":                     # P = 1/192 by another route
        q = torch.zeros_like(q)
    else:
        raise KeyError(name)
    return q.contiguous(), k.contiguous()


def gauss_v(seed):
    """The V of the older tests: N(0,1), (16, 192, 80)."""
    return _gauss(seed)[2]


def wide_v(seed):
    """V = randn * logspace(-3, 3, 80)[d] * (-1)^j, (16, 192, 80): six decades across the output columns, alternating sign along the keys."""
    g = torch.Generator().manual_seed(7000 + seed)
    sign = 1.0 - 2.0 * (torch.arange(NTOK) % 2).float()
    return torch.randn(NH, NTOK, HD, generator=g) * torch.logspace(-3, 3, HD) * sign[:, None]


def probe_v(c):
    """(192, 80): v[j, d] = 1 if j == 80 c + d.  The third setting carries keys in d < 32 only; its columns d >= 32 are all zero."""
    v = torch.zeros(NTOK, HD)
    n = min(HD, NTOK - HD * c)
    v[HD * c + torch.arange(n), torch.arange(n)] = 1.0
    return v


def pack(q, k, v):
    """q, k (B, 16, 192, 80) and v ((B, 16, 192, 80), or anything that broadcasts to it) -> qkv (B, 192, 3840) = [q | k | v]."""
    B = q.shape[0]
    v = v.expand(B, NH, NTOK, HD) if torch.is_tensor(v) else torch.full((B, NH, NTOK, HD), float(v))
    return torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B, NTOK, 3 * NH * HD).contiguous()


def unpack(out):
    """(B, 192, 1280) -> (B, 16, 192, 80)."""
    return out.reshape(out.shape[0], NTOK, NH, HD).permute(0, 2, 1, 3)


def read_out(run, q, k):
    """The probability matrix as `run` (qkv (B,192,3840) -> out (B,192,1280), CPU tensors) computes it: P (B, 16, 192, 192), and the 48
    columns of the third probe that carry no key, (B, 16, 192, 48) — sums of exact zeros."""
    o = [unpack(run(pack(q, k, probe_v(c)))) for c in range(3)]
    return torch.cat([o[0], o[1], o[2][..., :NTOK - 2 * HD]], -1), o[2][..., NTOK - 2 * HD:]


def statement32(q, k):
    """The plain fp32 statement whose own error sets the scale."""
    return (q @ k.transpose(-2, -1)).softmax(-1)


class Reference:
    """float64 side of one crop (or a stack of crops): P64, A (..., 192, 1), t (..., 192, 192) >= 0, ok = P64 >= 2^-100, masked share."""

    def __init__(self, q, k):
        q64, k64 = q.double(), k.double()
        s = q64 @ k64.transpose(-2, -1)
        self.P64 = s.softmax(-1)
        self.A = (q64.abs() @ k64.abs().transpose(-2, -1)).amax(-1, keepdim=True)
        self.t = (s.amax(-1, keepdim=True) - s) * math.log2(math.e)
        self.ok = self.P64 >= P_MIN
        self.masked = 1.0 - self.ok.double().mean().item()
        assert self.masked <= MASK_CAP, f"{self.masked:.3g} of the probabilities lie below 2^-100: the case would be judged on what is left"
        self.scale = self.P64 * (self.A + self.t + 1.0)

    def units(self, P):
        """max u_ij over the judged elements (nan if any of them is not finite)."""
        u = (P.double() - self.P64).abs() / self.scale / ULP
        u = u[self.ok]
        return float("nan") if not torch.isfinite(u).all() else u.max().item()

    def below_max(self, P):
        """max |P| where P64 < 2^-100 (0 if there is no such element)."""
        return P[~self.ok].abs().max().item() if not self.ok.all() else 0.0

    def out_of_rule(self, P, u_ref, mult):
        """How many judged elements are outside |P - P64| <= P64 2^-24 max(4, mult u_ref (A + |t| + 1)); a nan counts as outside."""
        tol = ULP * torch.maximum(FLOOR_UNITS * self.P64, mult * u_ref * self.scale)
        return int((~((P.double() - self.P64).abs() <= tol) & self.ok).sum())


def check_P(tag, P, ref, P32, mult):
    """The rule on one probability matrix.  Prints the figures, returns (ok, figures): the device's and the fp32 statement's units, their
    ratio, the elements out of the rule and the largest value where P64 < 2^-100."""
    u_ref, u = ref.units(P32), ref.units(P)
    bad, below = ref.out_of_rule(P, u_ref, mult), ref.below_max(P)
    fig = dict(units=u, units_ref=u_ref, ratio=u / u_ref, out_of_rule=bad, below_max=below, masked=ref.masked)
    print(f"{tag}: {u:.2f} units, fp32 statement's own {u_ref:.2f} (ratio {u / u_ref:.2f}), {bad} elements out of the rule at x{mult:g}, "
          f"largest value below 2^-100: {below:.1e} (masked share {ref.masked:.1e})")
    return bad == 0 and below <= P_BELOW_MAX and u == u, fig


def rowsum_ulps(out_ones):
    """V = 1: every output element is sum(e) * (1 / sum(e)); its largest distance from 1 in ulp of 1."""
    return ((out_ones.double() - 1.0).abs().max() / ULP).item()


def v_units(out, ref, v):
    """max |out - P64 @ v| / (P64 @ |v|) 2^24 for an output (…, 192, 80) on values v."""
    v64 = v.double()
    r = (out.double() - ref.P64 @ v64).abs() / (ref.P64 @ v64.abs()) / ULP
    return float("nan") if not torch.isfinite(r).all() else r.max().item()
