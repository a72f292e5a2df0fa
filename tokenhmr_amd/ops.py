"""Stateless operator wrappers over the C ABI (thmr_op_*), used for per-kernel parity tests and
micro-benchmarks.  Inputs/outputs are contiguous fp32 CUDA tensors; no CPU path exists.  The GEMM family (`gemm`, `gemm_split3`, `split3`)
also takes what its ABI takes: row-strided operands and a caller's `out=` (see `_ld`, `_ld_s3`)."""
import ctypes as C

import torch

from . import _cabi

# Variant ids of thmr_op_gemm beyond the ones the engine uses (include/tokenhmr_hip.h lists those): A/B material kept for the per-kernel tests
# and scripts/ — 0 / 1 = register-staged 128x128 / 128x160 tiles (lost to the LDS-DMA tiles 7 / 8 in round 1), 12 / 13 = 64x128 / 128x64 tiles
# (faster stand-alone, slower in the pipeline: round 3), 110 + j = the ring kernel 8-deep (ring depth A/B), 31-53 = timing-only ablations
# of builds with -DTHMR_GEMM_ABLATION.  thmr_op_gemm_split3: 1 = 128x256 on 4 waves, 4 = 256x256, 100-102 = ring kernel on split3 operands,
# 20 / 22 / 310-312 = the round-4 first versions on v_mfma_f32_32x32x16_bf16, 3 / 31-37 = schedule experiments; thmr_op_gemm_split3_out_split3:
# 1, 4, 100, 301 (persistent kernel, LDS epilogue), 311 / 312 — all of these exist in the experiments build only (SPLIT3_EXP_ONLY below).
EPI = {"none": 0, "bias": 1, "bias_gelu": 2, "bias_relu": 3, "bias_resid": 4, "bias_qscale": 5, "bias_pos": 6}
VARIANT = {"auto": -1, "128x128reg": 0, "128x160reg": 1, "skinny": 2, "128x128": 7, "128x160": 8, "64x64": 9, "128x96": 10, "tiny": 11, "64x128": 12, "128x64": 13, "ring16": 120}
# small-M ring kernel: "ring4" / "ring8" = LDS ring depth, optional "/k<S>" = split-K factor (1, 2, 4, 8, 16)
VARIANT.update({f"ring{r}" + (f"/k{1 << j}" if j else ""): 100 + (10 if r == 8 else 0) + j for r in (4, 8) for j in range(5)})
# split-K on the big LDS-DMA tiles (mid-size batches): "<tile>/k2", "<tile>/k4", "auto/k2", "auto/k4"
VARIANT.update({f"{t}/k{k}": 100 * k + c for t, c in (("auto", 0), ("128x128", 7), ("128x160", 8), ("128x96", 10), ("64x128", 12), ("128x64", 13)) for k in (2, 4)})
# (timing-only ablation kernels 31-53 exist only in builds with -DTHMR_GEMM_ABLATION, see gemm_f32.hip)


_EXP = None      # None: the shipped library (or THMR_LIB=exp); True: the experiments build (variants that lost their A/B, knobs)


class experiments_build:
    """`with ops.experiments_build(): ...` — the wrappers below call the -DTHMR_EXPERIMENTS library inside the block (tests / scripts)."""

    def __enter__(self):
        global _EXP
        self._old, _EXP = _EXP, True
        return self

    def __exit__(self, *a):
        global _EXP
        _EXP = self._old
        return False


def _L():
    return _cabi.load(exp=_EXP)


def _check(rc):
    _cabi.check(rc, None, _L())


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _s(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _req(*ts):
    for t in ts:
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("ops need contiguous float32 CUDA tensors")


def _ld(t, what, mult=1):
    """Row stride (the ABI's lda / ldc / ld_src, in elements) of a 2-D fp32 operand: rows of unit stride, `stride(0) >= columns` and a
    multiple of `mult`.  Anything else is refused: the ABI cannot express it."""
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] > 0 and t.stride(1) == 1):
        raise ValueError(f"{what}: a 2-D float32 CUDA tensor whose rows have unit stride")
    ld = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])
    if ld < t.shape[1] or ld % mult:
        raise ValueError(f"{what}: row stride {ld} must be >= {t.shape[1]} columns" + (f" and a multiple of {mult}" if mult > 1 else ""))
    return ld


def _ld_s3(t, what):
    """Row stride in fp32-EQUIVALENTS (the ABI's lda / ldw / ldcs / ld_dst: a row is 6 * ld bytes) of a row-major split3 operand: int16
    (R, K/8, 3, 8), contiguous or the (R, K/8, 3, 8) view of a wider operand (strides (3 * ld, 24, 8, 1), ld % 8 == 0)."""
    if not (t.is_cuda and t.dtype == torch.int16 and t.dim() == 4 and t.shape[1] > 0 and t.shape[2:] == (3, 8) and t.stride()[1:] == (24, 8, 1)):
        raise ValueError(f"{what}: a split3 operand is int16 (R, K/8, 3, 8) with dense rows")
    s0 = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), 24 * t.shape[1])
    if s0 < 24 * t.shape[1] or s0 % 24:
        raise ValueError(f"{what}: row stride {s0} int16 must be a multiple of 24 and >= {24 * t.shape[1]}")
    return s0 // 3


def _ldc_of(out, resid, M, N):
    """ldc of an fp32 result: `out`'s row stride, N for a fresh one.  The C ABI reads the residual with C's row stride."""
    if out is not None and tuple(out.shape) != (M, N):
        raise ValueError(f"out must be ({M}, {N})")
    ldc = _ld(out, "out") if out is not None else N
    if resid is not None:
        if tuple(resid.shape) != (M, N):
            raise ValueError(f"resid must be ({M}, {N})")
        if _ld(resid, "resid") != ldc:
            raise ValueError(f"resid has row stride {_ld(resid, 'resid')}, the result {ldc}: the operator reads both with one stride (ldr = ldc)")
    return ldc


def gemm(a, w, bias=None, resid=None, epi="none", qscale=1.0, qcols=0, variant="auto", out=None):
    """C = epilogue(a @ w.T);  a (M,K), w (N,K) — torch.nn.Linear layout.  `a` may be row-strided (lda = its row stride, a multiple of 4);
    `w` is dense (the operator has no ldw).  `out`: write into this (M,N) tensor, row-strided or not (ldc = its row stride, any value >= N);
    it may be `resid` itself (the sum in place).  `resid` (epi "bias_resid") must have the result's row stride."""
    _req(w, bias)
    M, K = a.shape
    N = w.shape[0]
    lda = _ld(a, "a", 4)
    if w.dim() != 2 or w.shape[1] != K:
        raise ValueError("K mismatch")
    if epi == "bias_pos":
        _req(resid)                               # the position table (193, N), not a residual
        ldc = _ldc_of(out, None, M, N)
    else:
        ldc = _ldc_of(out, resid, M, N)
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32)
    with torch.cuda.device(a.device):
        _check(_L().thmr_op_gemm(_p(a), lda, _p(w), _p(bias), _p(resid), _p(out), ldc, M, N, K, EPI[epi],
                                             float(qscale), int(qcols), VARIANT[variant], _s(a)))
    return out


SPLIT3_VARIANT = {"auto": -1, "128x256/w8": 0, "tail": 5,        # tail: the 128x256 grid with its ragged last round as 128x128 half tiles (qualifying shapes only)
                   "128x128/w8": 6, "tail/w8": 7, "128x128/w4/s3": 8, "128x128/w8/s3": 9, "128x256/w8/front": 10, "128x128/w4/s3/front": 11,   # front: every copy of a K tile issued right behind the barrier
                      # s3: the four-wave tile with a three-stage K ring
                                   # round 6: the 128x128 tile / the tail's half tiles on eight waves of 64x32 (measured slower / equal: not the rule's choice)
                   "128x256/w4": 1, "128x128/w4": 2, "256x256/w4": 4, "ring": 100, "ring/k2": 101, "ring/k4": 102, "auto/k2": 202, "auto/k4": 204,
                  # 256 persistent workgroups over a tile stream (csrc/gemm_split16.hip; host side csrc/gemm_split3_dispatch.hip; M % 32 == 0, N % 256 == 0, >= 256 tiles):
                  # fp32 output / split3 output through the LDS transposition / split3 output through swapped operand roles
                  "persist": 300, "persist/swap": 302, "persist/128x128": 320, "persist/128x128/k2": 322, "persist/128x128/k4": 324,      # 320: the stream over 128x128 tiles, three-stage ring (round 6)
                  # round-4 first versions on v_mfma_f32_32x32x16_bf16 (the product kernels moved to 16x16x32, csrc/gemm_split16.hip): experiments build
                  "old/128x256/w8": 20, "old/128x128/w4": 22, "old/persist": 310, "old/persist/lds": 311, "old/persist/swap": 312,
                  # schedule experiments (epilogue "none" only; the abl/* ones are timing-only, their results are garbage)
                  "exp/reads-every-2nd": 3, "abl/no-copies": 31, "abl/no-barrier": 32, "abl/no-reads": 34, "abl/none": 37}


# variants that exist only in the experiments build (measured slower or timing-only; csrc/gemm_split3_exp.hip): asking
# for one of them routes THAT call to libtokenhmr_hip_exp.so
SPLIT3_EXP_ONLY = {"128x128/w4/s3/front", "128x128/w8", "128x128/w8/s3", "tail/w8", "128x256/w4", "256x256/w4", "ring", "ring/k2", "ring/k4", "exp/reads-every-2nd", "abl/no-copies",
                   "abl/no-barrier", "abl/no-reads", "abl/none", "old/128x256/w8", "old/128x128/w4", "old/persist", "old/persist/lds", "old/persist/swap"}


def _L_for(exp_only):
    return _cabi.load(exp=True) if exp_only else _L()


def split3(x, out=None):
    """fp32 (R,K) -> the "split3" operand of gemm_split3: every element as three bf16 pieces h + m + l, laid out [R][K/8][3][8]
    (returned as an int16 tensor of shape (R, K/8, 3, 8); see csrc/split3_convert.hip).  K % 8 == 0.  `x` may be row-strided (ld_src = its row
    stride, a multiple of 4); `out`: write into this (R, K/8, 3, 8) operand, which may be a view of a wider one (ld_dst, `_ld_s3`)."""
    R, K = x.shape
    ld_src = _ld(x, "x", 4)
    if out is None:
        out = torch.empty(R, K // 8, 3, 8, device=x.device, dtype=torch.int16)
    elif tuple(out.shape) != (R, K // 8, 3, 8):
        raise ValueError("out must be (R, K/8, 3, 8)")
    with torch.cuda.device(x.device):
        _check(_L().thmr_op_split3(_p(x), ld_src, _p(out), _ld_s3(out, "out"), R, K, _s(x)))
    return out


def split3_block(x_s):
    """row-major split3 operand (R, K/8, 3, 8) -> the ROW-BLOCKED form (ceil(R/32), K/8, 3, 32, 8) the engine uses between fc1 and fc2
    (csrc/common.h GemmArgs::a_blk): 32-row panels of 512 contiguous bytes per 16-byte chunk; rows past R are zero."""
    R, G = x_s.shape[0], x_s.shape[1]
    Rp = (R + 31) // 32 * 32
    pad = torch.zeros(Rp, G, 3, 8, device=x_s.device, dtype=x_s.dtype)
    pad[:R] = x_s
    return pad.view(Rp // 32, 32, G, 3, 8).permute(0, 2, 3, 1, 4).contiguous()


def split3_unblock(x_b, R):
    """inverse of split3_block: (ceil(R/32), K/8, 3, 32, 8) -> (R, K/8, 3, 8)"""
    nb, G = x_b.shape[0], x_b.shape[1]
    return x_b.permute(0, 3, 1, 2, 4).reshape(nb * 32, G, 3, 8)[:R].contiguous()


def gemm_split3(a_s, w_s, bias=None, resid=None, epi="none", qscale=1.0, qcols=0, variant="128x256/w8", out_split=False,
                a_blocked_rows=None, out_blocked=False, out=None):
    """C = epilogue(a @ w.T) for split3 operands (`split3(a)`, `split3(w)`) on the bf16 matrix pipe with fp32-grade results: six
    bf16 products per element pair, fp32 accumulation.  `out_split`: the result as a split3 operand (what the engine's fc1 hands fc2);
    `out_blocked`: that operand in the row-blocked form (`split3_block`).  `a_blocked_rows=M`: `a_s` IS in the row-blocked form and has M rows.
    What the engine runs for its ViT GEMMs in the default mode (`Engine.set_vit_gemm("split3")`, the creation default since ABI 4).
    Row-major operands may be views of wider ones (lda / ldw = their row strides, `_ld_s3`).  `out`: write into this tensor — fp32 (M,N),
    row-strided or not (ldc; may be `resid` itself, and `resid` must share its row stride); with `out_split` an (M, N/8, 3, 8) operand or
    view (ldcs); with `out_blocked` the contiguous (ceil(M/32), N/8, 3, 32, 8) tensor, whose pad rows the kernels leave alone."""
    _req(bias)
    if a_blocked_rows is not None:
        if not (a_s.is_cuda and a_s.dtype == torch.int16 and a_s.is_contiguous() and a_s.dim() == 5 and a_s.shape[2:] == (3, 32, 8)):
            raise ValueError("a row-blocked split3 operand is int16 (ceil(R/32), K/8, 3, 32, 8)")
        M, K = int(a_blocked_rows), a_s.shape[1] * 8
    else:
        M, K = a_s.shape[0], a_s.shape[1] * 8
    ldw = _ld_s3(w_s, "w_s")
    lda = K if a_blocked_rows is not None else _ld_s3(a_s, "a_s")
    N = w_s.shape[0]
    if w_s.shape[1] * 8 != K:
        raise ValueError("K mismatch")
    lib = _L_for(variant in SPLIT3_EXP_ONLY)
    code = SPLIT3_VARIANT[variant]
    if (out_blocked or a_blocked_rows is not None) and code < 0:
        raise ValueError("name the kernel (not 'auto') with a row-blocked operand")
    if out_split:
        ldcs = N
        if out_blocked:
            shape = ((M + 31) // 32, N // 8, 3, 32, 8)
            if out is None:
                alloc = torch.empty if M % 32 == 0 else torch.zeros            # the kernels never write the pad rows of the last block
                out = alloc(*shape, device=a_s.device, dtype=torch.int16)
            elif not (out.is_cuda and out.dtype == torch.int16 and out.is_contiguous() and tuple(out.shape) == shape):
                raise ValueError(f"out must be a contiguous int16 {shape}")
        elif out is None:
            out = torch.empty(M, N // 8, 3, 8, device=a_s.device, dtype=torch.int16)
        else:
            if tuple(out.shape) != (M, N // 8, 3, 8):
                raise ValueError("out must be (M, N/8, 3, 8)")
            ldcs = _ld_s3(out, "out")
        with torch.cuda.device(a_s.device):
            _cabi.check(lib.thmr_op_gemm_split3_out_split3(_p(a_s), lda, _p(w_s), ldw, _p(bias), _p(out), ldcs, M, N, K, EPI[epi],
                                                           float(qscale), int(qcols), code + (1000 if out_blocked else 0), _s(a_s)), None, lib)
        return out
    if epi == "bias_pos":
        _req(resid)                               # the position table (193, N), not a residual
        ldc = _ldc_of(out, None, M, N)
    else:
        ldc = _ldc_of(out, resid, M, N)
    if out is None:
        out = torch.empty(M, N, device=a_s.device, dtype=torch.float32)
    with torch.cuda.device(a_s.device):
        _cabi.check(lib.thmr_op_gemm_split3(_p(a_s), lda, _p(w_s), ldw, _p(bias), _p(resid), _p(out), ldc, M, N, K, EPI[epi],
                                            float(qscale), int(qcols), code + (1000 if a_blocked_rows is not None else 0), _s(a_s)), None, lib)
    return out


def layernorm(x, gamma, beta, eps, relu=False):
    _req(x, gamma, beta)
    rows, D = x.shape
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _check(_L().thmr_op_layernorm(_p(x), _p(gamma), _p(beta), _p(y), rows, D, float(eps), int(relu), _s(x)))
    return y


ATTN_VARIANT = {"auto": 0, "q64": 1, "q192": 3, "persistent": 5, "q16x12": 12, "keysplit": 6, "keysplit/q16": 61, "keysplit/q32": 62, "keysplit/q48": 63}


def _attn_out(out, shape, dtype, device):
    if out is None:
        return torch.empty(*shape, device=device, dtype=dtype)
    if not (out.is_cuda and out.dtype == dtype and out.is_contiguous() and tuple(out.shape) == shape):
        raise ValueError(f"out must be a contiguous {dtype} CUDA tensor of shape {shape}")
    return out


def vit_attention(qkv, variant="auto", out=None):
    """qkv (B,192,3840) with q pre-scaled -> (B,192,1280).  variant: "auto" (batch-size rule) or a forced kernel, see ATTN_VARIANT.
    `out`: write into this contiguous (B,192,1280) tensor."""
    _req(qkv)
    B = qkv.shape[0]
    out = _attn_out(out, (B, 192, 1280), torch.float32, qkv.device)
    with torch.cuda.device(qkv.device):
        if variant == "auto":
            _check(_L().thmr_op_vit_attention(_p(qkv), _p(out), B, _s(qkv)))
        else:
            lib = _L_for(variant == "q16x12")           # 12 waves of 16 queries: measured no faster, experiments build only
            _cabi.check(lib.thmr_op_vit_attention_variant(_p(qkv), _p(out), B, ATTN_VARIANT[variant], _s(qkv)), None, lib)
    return out


def vit_attention_split3(qkv, out=None):
    """vit_attention with the output as a split3 operand (int16 (B*192, 160, 3, 8)): what the engine's split3 mode hands the proj GEMM.
    `out`: write into this contiguous tensor of that shape."""
    _req(qkv)
    B = qkv.shape[0]
    out = _attn_out(out, (B * 192, 160, 3, 8), torch.int16, qkv.device)
    with torch.cuda.device(qkv.device):
        _check(_L().thmr_op_vit_attention_split3(_p(qkv), _p(out), B, _s(qkv)))
    return out


def vit_attention_b16(qkv, out_split=False, qt=0, out=None):
    """The attention on the bf16 matrix pipe (three bf16 pieces per operand, six products, fp32 accumulate: csrc/attention_b16.hip).
    out_split: the result as a split3 operand (int16 (B*192, 160, 3, 8)) instead of fp32 (B,192,1280); qt: 0 = batch-size rule, 1 / 3 = forced.
    `out`: write into this contiguous tensor of the result's shape and type."""
    _req(qkv)
    B = qkv.shape[0]
    out = (_attn_out(out, (B * 192, 160, 3, 8), torch.int16, qkv.device) if out_split
           else _attn_out(out, (B, 192, 1280), torch.float32, qkv.device))
    with torch.cuda.device(qkv.device):
        _check(_L().thmr_op_vit_attention_b16(_p(qkv), _p(out), B, int(out_split), int(qt), _s(qkv)))
    return out


def rot6d_to_rotmat(x):
    """geometry.py:64-84 rot6d_to_rotmat == rotation_utils.py:510-531 rotation_6d_to_matrix: (..., 6) -> (n,3,3).  Differentiable: under
    torch.is_grad_enabled(), an x that requires grad gets a graph whose backward is thmr_op_rot6d_backward."""
    _req(x)
    if torch.is_grad_enabled() and x.requires_grad:
        return _Rot6dFn.apply(x.reshape(-1, 6))      # the reshape carries the gradient back to x's own shape
    return _rot6d(x.reshape(-1, 6).contiguous())


def _rot6d(x2):
    n = x2.shape[0]
    R = torch.empty(n, 3, 3, device=x2.device, dtype=torch.float32)
    with torch.cuda.device(x2.device):
        _check(_L().thmr_op_rot6d(_p(x2), _p(R), n, _s(x2)))
    return R


def rot6d_backward(x, grad_R, out=None):
    """thmr_op_rot6d_backward: x (n,6), grad_R (n,3,3) -> the gradient by x, (n,6); `out` receives it when given (no allocation)."""
    _req(x, grad_R)
    g = torch.empty_like(x) if out is None else out
    with torch.cuda.device(x.device):
        _check(_L().thmr_op_rot6d_backward(_p(x), _p(grad_R), _p(g), x.shape[0], _s(x)))
    return g


class _Rot6dFn(torch.autograd.Function):
    """rot6d_to_rotmat under autograd: backward = thmr_op_rot6d_backward (csrc/head.hip rot6d_backward_kernel), once differentiable."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        ctx.save_for_backward(x)
        return _rot6d(x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gR):
        x, = ctx.saved_tensors
        return rot6d_backward(x, gR.to(torch.float32).contiguous())


def aa_to_rotmat(theta):
    """geometry.py:5-44 aa_to_rotmat: (n,3) axis-angle -> (n,3,3)."""
    _req(theta)
    if torch.is_grad_enabled() and theta.requires_grad:
        return _AaToRotmatFn.apply(theta.reshape(-1, 3))      # the reshape carries the gradient back to theta's own shape
    return _aa_to_rotmat(theta.reshape(-1, 3).contiguous())


def _aa_to_rotmat(x):
    n = x.shape[0]
    R = torch.empty(n, 3, 3, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _check(_L().thmr_op_aa_to_rotmat(_p(x), _p(R), n, _s(x)))
    return R


class _AaToRotmatFn(torch.autograd.Function):
    """aa_to_rotmat under autograd: backward = thmr_op_aa_to_rotmat_backward (csrc/body_model.hip rodrigues_backward_kernel), once
    differentiable."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        ctx.save_for_backward(x)
        return _aa_to_rotmat(x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gR):
        x, = ctx.saved_tensors
        gR = gR.to(torch.float32).contiguous()
        g = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _check(_L().thmr_op_aa_to_rotmat_backward(_p(x), _p(gR), _p(g), x.shape[0], _s(x)))
        return g


# ---- the row, glue and head kernels (csrc/rowops.hip, head.hip, hmr2_head.hip), each as the engine launches it ----
def _req_i32(*ts):
    for t in ts:
        if t is not None and not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
            raise ValueError("index tables are contiguous int32 CUDA tensors")


def splitk_resid_ln(part, bias, resid, gamma, beta, eps, y_split3=False, inplace=False):
    """part (S, rows, 1280) split-K partial sums -> (xout, y): xout = resid + ((((part[0] + part[1]) + ...) + bias), y = LayerNorm(xout).
    y_split3: y as a split3 operand (int16 (rows, 160, 3, 8)) instead of fp32.  inplace: xout IS resid (what the engine passes; resid is
    overwritten)."""
    _req(part, bias, resid, gamma, beta)
    S, rows, D = part.shape
    if resid.shape != (rows, D):
        raise ValueError("resid is (rows, D)")
    xout = resid if inplace else torch.empty(rows, D, device=part.device, dtype=torch.float32)
    y = (torch.empty(rows, D // 8, 3, 8, device=part.device, dtype=torch.int16) if y_split3
         else torch.empty(rows, D, device=part.device, dtype=torch.float32))
    with torch.cuda.device(part.device):
        _check(_L().thmr_op_splitk_resid_ln(_p(part), S, rows, D, _p(bias), _p(resid), _p(xout), _p(gamma), _p(beta), _p(y), float(eps),
                                            int(y_split3), _s(part)))
    return xout, y


def add_ln64(x, y, gamma, beta, eps):
    """(rows, 64) x, y -> (s, z): s = x + y, z = LayerNorm64(s)."""
    _req(x, y, gamma, beta)
    if x.shape != y.shape or x.shape[-1] != 64:
        raise ValueError("add_ln64 needs two (rows, 64) tensors")
    s, z = torch.empty_like(x), torch.empty_like(x)
    with torch.cuda.device(x.device):
        _check(_L().thmr_op_add_ln64(_p(x), _p(y), _p(gamma), _p(beta), _p(s), _p(z), x.numel() // 64, float(eps), _s(x)))
    return s, z


def transpose(x, out=None):
    """(Bn, R, C) -> (Bn, C, R); `out`: write into this tensor (the tests pre-fill it)."""
    _req(x, out)
    Bn, R, Cc = x.shape
    if out is None:
        out = torch.empty(Bn, Cc, R, device=x.device, dtype=torch.float32)
    elif out.shape != (Bn, Cc, R):
        raise ValueError("out must be (Bn, C, R)")
    with torch.cuda.device(x.device):
        _check(_L().thmr_op_transpose(_p(x), _p(out), Bn, R, Cc, _s(x)))
    return out


def softmax_argmax(logits, probs=True, idx=True):
    """logits (rows, 2048) -> (probs (rows, 2048) or None, idx (rows) int32 or None): softmax and the lowest index of the row maximum."""
    _req(logits)
    rows = logits.shape[0]
    if logits.shape != (rows, 2048):
        raise ValueError("softmax_argmax needs (rows, 2048) logits")
    p = torch.empty_like(logits) if probs else None
    i = torch.empty(rows, device=logits.device, dtype=torch.int32) if idx else None
    with torch.cuda.device(logits.device):
        _check(_L().thmr_op_softmax_argmax(_p(logits), _p(p), _p(i), rows, _s(logits)))
    return p, i


def cross_attn(q, kv, koff=0):
    """q (B, 512), kv (B * 192, ldkv) with K | V of this layer at columns koff ... koff + 1023 -> (B, 512)."""
    _req(q, kv)
    B = q.shape[0]
    if q.shape != (B, 512) or kv.dim() != 2 or kv.shape[0] != B * 192:
        raise ValueError("cross_attn needs q (B, 512) and kv (B * 192, ldkv)")
    out = torch.empty(B, 512, device=q.device, dtype=torch.float32)
    with torch.cuda.device(q.device):
        _check(_L().thmr_op_cross_attn(_p(q), _p(kv), kv.shape[1], int(koff), _p(out), B, _s(q)))
    return out


def im2col_patch(img, out_split=False):
    """img (B, 3, 256, 256) -> the patch-embed A operand (B * 192, 768) fp32, or (out_split) int16 (B * 192, 96, 3, 8)."""
    _req(img)
    B = img.shape[0]
    if img.shape != (B, 3, 256, 256):
        raise ValueError("im2col_patch needs (B, 3, 256, 256)")
    out = (torch.empty(B * 192, 96, 3, 8, device=img.device, dtype=torch.int16) if out_split
           else torch.empty(B * 192, 768, device=img.device, dtype=torch.float32))
    with torch.cuda.device(img.device):
        _check(_L().thmr_op_im2col_patch(_p(img), _p(out), B, int(out_split), _s(img)))
    return out


def conv3_gather(x, Tout, src=None, dil=1, prerelu=False, out=None):
    """x (Bn, Tin, C) channels-last -> (Bn, Tout, 3 * C): the A operand of Conv1d(k 3, padding = dilation = dil) on the signal resampled
    through `src` ((Tout) int32, None = identity).  `out`: write into this tensor."""
    _req(x, out)
    _req_i32(src)
    Bn, Tin, Cc = x.shape
    if src is not None and src.numel() != Tout:
        raise ValueError("src holds one index per output position")
    if out is None:
        out = torch.empty(Bn, Tout, 3 * Cc, device=x.device, dtype=torch.float32)
    elif out.shape != (Bn, Tout, 3 * Cc):
        raise ValueError("out must be (Bn, Tout, 3 C)")
    with torch.cuda.device(x.device):
        _check(_L().thmr_op_conv3_gather(_p(x), _p(out), _p(src), Bn, Tin, int(Tout), Cc, int(dil), int(prerelu), _s(x)))
    return out


def conv_gather(x, Tout, ks, stride, pad, Cp=None, src=None, Tsrc=None, out=None):
    """x (Bn, Tin, C) channels-last -> (Bn, Tout, ks * Cp): the A operand of Conv1d(ks, stride, pad) with the channels zero-padded to Cp,
    on the signal of length Tsrc (default Tin) resampled through `src` ((Tsrc) int32, None = identity)."""
    _req(x, out)
    _req_i32(src)
    Bn, Tin, Cc = x.shape
    Cp = Cc if Cp is None else int(Cp)
    Tsrc = (Tin if src is None else src.numel()) if Tsrc is None else int(Tsrc)
    if src is not None and src.numel() != Tsrc:
        raise ValueError("src holds one index per resampled position")
    if out is None:
        out = torch.empty(Bn, Tout, ks * Cp, device=x.device, dtype=torch.float32)
    elif out.shape != (Bn, Tout, ks * Cp):
        raise ValueError("out must be (Bn, Tout, ks Cp)")
    with torch.cuda.device(x.device):
        _check(_L().thmr_op_conv_gather(_p(x), _p(out), _p(src), Bn, Tin, Tsrc, int(Tout), Cc, Cp, int(ks), int(stride), int(pad), _s(x)))
    return out


def conv_repack(w, cp=None):
    """Conv1d weight (co, ci, kk) -> (co, kk * cp), [o][k * cp + i] = w[o][i][k], zero for ci <= i < cp (cp defaults to ci)."""
    _req(w)
    co, ci, kk = w.shape
    cp = ci if cp is None else int(cp)
    out = torch.empty(co, kk * cp, device=w.device, dtype=torch.float32)
    with torch.cuda.device(w.device):
        _check(_L().thmr_op_conv_repack(_p(w), _p(out), co, ci, cp, kk, _s(w)))
    return out


def vq_argmin_rows(x, dot, cnorm, want_dist=True):
    """x (rows, 256), dot = x @ codebook.T (rows, 2048), cnorm (2048) -> (idx (rows) int32, dist (rows, 2048) or None)."""
    _req(x, dot, cnorm)
    rows = x.shape[0]
    if x.shape != (rows, 256) or dot.shape != (rows, 2048) or cnorm.shape != (2048,):
        raise ValueError("vq_argmin_rows needs x (rows, 256), dot (rows, 2048), cnorm (2048)")
    idx = torch.empty(rows, device=x.device, dtype=torch.int32)
    dist = torch.empty(rows, 2048, device=x.device, dtype=torch.float32) if want_dist else None
    with torch.cuda.device(x.device):
        _check(_L().thmr_op_vq_argmin_rows(_p(x), _p(dot), _p(cnorm), _p(idx), _p(dist), rows, _s(x)))
    return idx, dist


def code_norm(cb):
    """codebook (ncode, 256) -> squared norms (ncode)."""
    _req(cb)
    n = cb.shape[0]
    if cb.shape != (n, 256):
        raise ValueError("code_norm needs (ncode, 256)")
    cn = torch.empty(n, device=cb.device, dtype=torch.float32)
    with torch.cuda.device(cb.device):
        _check(_L().thmr_op_code_norm(_p(cb), _p(cn), n, _s(cb)))
    return cn


def head_finish(kind, ro, init_pose, init_betas, init_cam, bpose=None, focal_length=5000.0, img_size=256.0,
                want_pose6d=True, want_cam_t=True, want_focal=True):
    """The finish of the SMPL head behind the read-out GEMM.  kind "token": ro (B, ld >= 31) + bpose (B, 126); "hmr2": ro (B, ld >= 157).
    Returns a dict: rotmat (B, 24, 3, 3), betas (B, 10), cam (B, 3) and — unless switched off, then None — pose6d (B, 144), cam_t (B, 3),
    focal (B, 2)."""
    _req(ro, init_pose, init_betas, init_cam, bpose)
    B, ld = ro.shape
    if init_pose.numel() != 144 or init_betas.numel() != 10 or init_cam.numel() != 3 or (bpose is not None and bpose.shape != (B, 126)):
        raise ValueError("head_finish: init_pose (144), init_betas (10), init_cam (3), bpose (B, 126)")
    new = lambda *s: torch.empty(*s, device=ro.device, dtype=torch.float32)
    o = {"rotmat": new(B, 24, 3, 3), "betas": new(B, 10), "cam": new(B, 3), "pose6d": new(B, 144) if want_pose6d else None,
         "cam_t": new(B, 3) if want_cam_t else None, "focal": new(B, 2) if want_focal else None}
    with torch.cuda.device(ro.device):
        _check(_L().thmr_op_head_finish({"token": 0, "hmr2": 1}[kind], _p(ro), ld, _p(bpose), _p(init_pose), _p(init_betas), _p(init_cam),
                                        _p(o["pose6d"]), _p(o["rotmat"]), _p(o["betas"]), _p(o["cam"]), _p(o["cam_t"]), _p(o["focal"]),
                                        float(focal_length), float(img_size), B, _s(ro)))
    return o


def decoder_init(bias, pos, B):
    """bias, pos (E) -> x (B, E) = bias + pos for every crop."""
    _req(bias, pos)
    E = bias.numel()
    if pos.numel() != E:
        raise ValueError("bias and pos have the same length")
    x = torch.empty(B, E, device=bias.device, dtype=torch.float32)
    with torch.cuda.device(bias.device):
        _check(_L().thmr_op_decoder_init(_p(bias), _p(pos), _p(x), int(B), E, _s(bias)))
    return x


# ---- the tokenizer round trip's own kernels (csrc/tokenizer.hip) ----
def vq_stats(x, codebook, idx, code_count=None, accumulate=False):
    """What QuantizeEMAReset.forward returns beside the codes (quantize_cnn.py:38-47,118-121): x (rows, 256), codebook (2048, 256),
    idx (rows) int32 -> (commit_loss, perplexity, code_count): two 0-dim device floats and the (2048) int32 histogram.  code_count given:
    written in place — overwritten, or added to with accumulate=True (the perplexity is then that of the summed counts)."""
    _req(x, codebook)
    _req_i32(idx, code_count)
    rows = x.shape[0]
    if x.shape != (rows, 256) or codebook.shape != (2048, 256) or idx.shape != (rows,) or (code_count is not None and code_count.shape != (2048,)):
        raise ValueError("vq_stats needs x (rows, 256), codebook (2048, 256), idx (rows), code_count (2048)")
    if code_count is None:
        if accumulate:
            raise ValueError("accumulate=True needs the caller's code_count")
        code_count = torch.empty(2048, device=x.device, dtype=torch.int32)
    partial = torch.empty((rows + 31) // 32, device=x.device, dtype=torch.float32)
    out = torch.empty(2, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _check(_L().thmr_op_vq_stats(_p(x), _p(codebook), _p(idx), rows, _p(code_count), int(bool(accumulate)), _p(partial),
                                     C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 4), _s(x)))
    return out[0], out[1], code_count


def rotmat_to_aa(R):
    """matrix_to_axis_angle (tokenization/models/rotation_utils.py:428-441): (..., 3, 3) -> (n, 3), n = the number of matrices."""
    _req(R)
    m = R.reshape(-1, 3, 3).contiguous()
    n = m.shape[0]
    aa = torch.empty(n, 3, device=R.device, dtype=torch.float32)
    with torch.cuda.device(R.device):
        _check(_L().thmr_op_rotmat_to_aa(_p(m), _p(aa), n, _s(R)))
    return aa


# ---- the forward value of the loss (csrc/loss.hip) ----
VAL_LOSS_TAPS = ("kp2d_err", "angle_err", "valid2d", "weak2d", "valid_rot", "weak_rot", "conf2d_used", "conf3d_used", "has_betas_used")


def _val_loss_inputs(who, ins, loose, valid_3d, kp2d_thresh, angle_thresh, weights):
    """The checks val_loss and val_loss_grad share, on the eleven inputs in the order of thmr_val_loss_in -> (B, gt_pose_is_rotmat)."""
    _req(*ins, valid_3d, kp2d_thresh, angle_thresh)
    B, gt_pose = ins[0].shape[0], ins[6]
    if gt_pose.shape == (B, 72):
        is_rotmat = 0
    elif gt_pose.shape == (B, 24, 3, 3):
        is_rotmat = 1
    else:
        raise ValueError(f"{who}: gt_pose is (B,72) axis-angle or (B,24,3,3) matrices, got {tuple(gt_pose.shape)}")
    want = [(B, 44, 2), (B, 44, 3), (B, 24, 3, 3), (B, 10), (B, 44, 3), (B, 44, 4), tuple(gt_pose.shape), (B, 10), (B,), (B,), (B,)]
    for t, w in zip(ins, want):
        if tuple(t.shape) != w:
            raise ValueError(f"{who}: a tensor of shape {tuple(t.shape)} where {w} is expected")
    if loose:
        if valid_3d is None or kp2d_thresh is None or angle_thresh is None:
            raise ValueError(f"{who}: the loose mode needs valid_3d, kp2d_thresh and angle_thresh")
        if tuple(valid_3d.shape) != (B,) or tuple(kp2d_thresh.shape) != (44,) or tuple(angle_thresh.shape) != (24,):
            raise ValueError(f"{who}: valid_3d (B), kp2d_thresh (44), angle_thresh (24)")
    if len(weights) != 5:
        raise ValueError(f"{who}: five weights (2D, 3D, global_orient, body_pose, betas)")
    return B, is_rotmat


def _val_loss_structs(ins, weights, loose, loose_weight, valid_3d, kp2d_thresh, angle_thresh, pelvis_id, is_rotmat):
    """(thmr_val_loss_desc, thmr_val_loss_in) of checked inputs."""
    w = [float(x) for x in weights]
    desc = _cabi.ValLossDesc(*w, float(loose_weight), int(pelvis_id), _cabi.VAL_LOSS_LOOSE if loose else _cabi.VAL_LOSS_PLAIN, is_rotmat, 0)
    ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    return desc, _cabi.ValLossIn(*[ptr(t) for t in ins], ptr(valid_3d), ptr(kp2d_thresh), ptr(angle_thresh))


def val_loss(pred_kp2d, pred_kp3d, pred_rotmat, pred_betas, gt_kp2d, gt_kp3d, gt_pose, gt_betas, has_global_orient, has_body_pose,
             has_betas, weights, loose=False, loose_weight=0.0, valid_3d=None, kp2d_thresh=None, angle_thresh=None, pelvis_id=39,
             taps=True, running=None, workspace=None, losses=None, out=None):
    """thmr_val_loss: compute_loss (tokenhmr.py:190-277) for B items.  pred_kp2d (B,44,2), pred_kp3d (B,44,3), pred_rotmat (B,24,3,3),
    pred_betas (B,10), gt_kp2d (B,44,3), gt_kp3d (B,44,4), gt_pose (B,72) axis-angle or (B,24,3,3) matrices, gt_betas (B,10), has_* (B);
    weights: the five LOSS_WEIGHTS in the order 2D, 3D, global_orient, body_pose, betas.  loose: valid_3d (B), kp2d_thresh (44),
    angle_thresh (24).  Returns a dict of device tensors: 'losses' (6, the reference's dict order), 'per_item' (B,5) and — loose with
    taps — VAL_LOSS_TAPS.  running: a (7) float64 device tensor that the call adds its six losses and a count of 1 to.  out: a dict of preallocated
    tensors for 'per_item' and the taps (a caller that must not allocate); what it lacks is allocated.  No host synchronisation; nothing
    is written into an input."""
    ins = [pred_kp2d, pred_kp3d, pred_rotmat, pred_betas, gt_kp2d, gt_kp3d, gt_pose, gt_betas, has_global_orient, has_body_pose, has_betas]
    _req(workspace, losses)
    B, is_rotmat = _val_loss_inputs("val_loss", ins, loose, valid_3d, kp2d_thresh, angle_thresh, weights)
    if running is not None and not (running.is_cuda and running.dtype == torch.float64 and running.shape == (7,) and running.is_contiguous()):
        raise ValueError("val_loss: running is a contiguous (7) float64 CUDA tensor")
    dev = pred_kp2d.device
    new = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)      # noqa: E731

    def pick(k, *shape):
        t = out.get(k) if out is not None else None
        if t is None:
            return new(*shape)
        _req(t)
        if tuple(t.shape) != shape:
            raise ValueError(f"val_loss: out['{k}'] is {shape}, got {tuple(t.shape)}")
        return t

    res = {"losses": losses if losses is not None else new(6), "per_item": pick("per_item", B, 5)}
    if res["losses"].shape != (6,):
        raise ValueError("val_loss: losses is a (6) tensor")
    if loose and taps:
        res.update({k: pick(k, B) if k == "has_betas_used" else pick(k, B, 44 if "2d" in k or "3d" in k else 24) for k in VAL_LOSS_TAPS})
    need = _cabi.VAL_LOSS_WS_PER_ITEM * B
    if workspace is None:
        workspace = new(need)
    elif workspace.numel() < need:
        raise ValueError(f"val_loss: the workspace holds {workspace.numel()} floats, {need} are needed")
    desc, cin = _val_loss_structs(ins, weights, loose, loose_weight, valid_3d, kp2d_thresh, angle_thresh, pelvis_id, is_rotmat)
    ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    cout = _cabi.ValLossOut(**{k: ptr(res.get(k)) for k in _cabi.VAL_LOSS_OUT_FIELDS if k != "running"}, running=ptr(running))
    with torch.cuda.device(dev):
        _check(_L().thmr_val_loss(C.byref(desc), C.byref(cin), B, C.byref(cout), _p(workspace), _s(pred_kp2d)))
    return res


# ---- its gradient (csrc/loss.hip) ----
LOSS_GRAD_SLOTS = ("kp2d", "kp3d", "joints", "cam", "rotmat", "betas")          # header: THMR_LOSS_GRAD_*, in slot order


def val_loss_grad(pred_kp2d, pred_kp3d, pred_rotmat, pred_betas, gt_kp2d, gt_kp3d, gt_pose, gt_betas, has_global_orient, has_body_pose,
                  has_betas, weights, loose=False, loose_weight=0.0, valid_3d=None, kp2d_thresh=None, angle_thresh=None, pelvis_id=39,
                  pred_cam=None, focal_length=5000.0, image_size=256.0, want=None, out=None):
    """thmr_val_loss_grad: the gradient of val_loss's total (a sum over the B items) — inputs, weights and mode as val_loss takes them.
    Returns a dict of device tensors keyed by LOSS_GRAD_SLOTS: 'kp2d' (B,44,2), 'kp3d' (B,44,3), 'rotmat' (B,24,3,3), 'betas' (B,10) — the
    plain partial derivatives by the four predictions — and, with pred_cam (B,3), 'joints' (B,44,3) = 'kp3d' + the projection's adjoint
    of 'kp2d' (what the body model's backward takes) and 'cam' (B,3).  want: the slots to compute (default: every slot the arguments
    allow); out: a dict of preallocated tensors to write into.  One launch, no host synchronisation."""
    ins = [pred_kp2d, pred_kp3d, pred_rotmat, pred_betas, gt_kp2d, gt_kp3d, gt_pose, gt_betas, has_global_orient, has_body_pose, has_betas]
    B, is_rotmat = _val_loss_inputs("val_loss_grad", ins, loose, valid_3d, kp2d_thresh, angle_thresh, weights)
    _req(pred_cam)
    if pred_cam is not None and tuple(pred_cam.shape) != (B, 3):
        raise ValueError(f"val_loss_grad: pred_cam is (B,3), got {tuple(pred_cam.shape)}")
    if want is None:
        want = [k for k in LOSS_GRAD_SLOTS if pred_cam is not None or k not in ("joints", "cam")]
    unknown = [k for k in want if k not in LOSS_GRAD_SLOTS]
    if unknown or not want:
        raise ValueError(f"val_loss_grad: want names slots of {LOSS_GRAD_SLOTS}, at least one; got {list(want)}")
    if pred_cam is None and ("joints" in want or "cam" in want):
        raise ValueError("val_loss_grad: 'joints' and 'cam' need pred_cam")
    shapes = {"kp2d": (B, 44, 2), "kp3d": (B, 44, 3), "joints": (B, 44, 3), "cam": (B, 3), "rotmat": (B, 24, 3, 3), "betas": (B, 10)}
    dev = pred_kp2d.device
    res = {}
    for k in want:
        t = out.get(k) if out is not None else None
        if t is None:
            t = torch.empty(shapes[k], device=dev, dtype=torch.float32)
        _req(t)
        if tuple(t.shape) != shapes[k]:
            raise ValueError(f"val_loss_grad: out['{k}'] is {shapes[k]}, got {tuple(t.shape)}")
        res[k] = t
    desc, cin = _val_loss_structs(ins, weights, loose, loose_weight, valid_3d, kp2d_thresh, angle_thresh, pelvis_id, is_rotmat)
    table = (C.c_void_p * _cabi.LOSS_GRAD_SLOTS)(*[res[k].data_ptr() if k in res else None for k in LOSS_GRAD_SLOTS])
    with torch.cuda.device(dev):
        _check(_L().thmr_val_loss_grad(C.byref(desc), C.byref(cin), _p(pred_cam), float(focal_length), float(image_size), B, table,
                                       _s(pred_kp2d)))
    return res


def token_ce(x, target, out=None, workspace=None):
    """thmr_op_token_ce: TokenLoss (losses.py:230-252), CrossEntropyLoss in mean reduction over the rows of x (rows, 2048) fp32 with int32
    targets (rows) -> a 0-dim device float (or `out`).  The per-row losses are left in `workspace` (rows floats).  A target outside
    [0, 2048) makes its row, and the mean, NaN."""
    _req(x, out, workspace)
    _req_i32(target)
    rows = x.shape[0]
    if x.shape != (rows, 2048) or target.shape != (rows,):
        raise ValueError(f"token_ce needs x (rows, 2048) and target (rows), got {tuple(x.shape)} and {tuple(target.shape)}")
    out = out if out is not None else torch.empty((), device=x.device, dtype=torch.float32)
    need = _cabi.TOKEN_CE_WS_PER_ROW * rows
    if workspace is None:
        workspace = torch.empty(need, device=x.device, dtype=torch.float32)
    elif workspace.numel() < need:
        raise ValueError(f"token_ce: the workspace holds {workspace.numel()} floats, {need} are needed")
    with torch.cuda.device(x.device):
        _check(_L().thmr_op_token_ce(_p(x), _p(target), rows, _p(out), _p(workspace), _s(x)))
    return out
