"""Guard bands for the row, glue, head, loss, metric and body-model operators and for the engine's own outputs (-m gpu).

The per-kernel parity files look only at the tensor a kernel is supposed to fill, their outputs come from torch.empty and their inputs are
plain contiguous tensors — so a store one row past the end, a load past the end of an input, and an output element that is never written
are all invisible to them.  Here every stateless entry point of the C ABI outside the GEMM and attention operators (those have
tests/test_gpu_strided.py), the two body models' forward passes, the engine's sub-paths and the engine's own outputs run with EVERY buffer
as a window between canaries, through the one calling convention of tests/guarded_call.py: nothing outside a window written, every output
element written and finite, every input left as it was, every output bit-equal to the same call on plain contiguous tensors (the form the
parity files hold to float64).  Integer inputs are padded with an in-range value that changes the result: an unused target class / code /
joint, or an index that points at a source row full of canaries.  An over-read whose value is never used is out of reach of the method.

`CASES` is the table: entry point -> the parameter sets, each the smallest shape that reaches the edge in question (four rows per
workgroup: 1, 4, 5 rows; 256 elements per workgroup: 1, 255, 256, 257; 32 x 32 transpose tiles; 32 rows per partial sum; 1024-element
spans of the reconstruction loss; `cg` crops per pass of the skinning kernels).  It is importable without a GPU:
tests/test_guarded_host.py holds it, together with `EXEMPT`, against every prototype of include/tokenhmr_hip.h.

Bit-equality with the plain call says nothing about a value that is wrong in both calls, and most of these shapes (the ragged tails) are
ones no parity file runs.  So `STATEMENTS` puts a float64 or exact statement beside the guarded call of 24 entry points, at every case, with
the bound of the parity test of the same operation, named at each statement — (E) exact, (B) bound, (C) class in the convention of
tests/test_gpu_rowops.py; no tolerance is new.  The other 14 entry points have none: `COVERED_BY` names, for each, the parity tests
that hold the same shapes (or, for the engine's sub-paths, the same kernels) to their reference.

Measured on the MI355X: the whole file, 318 cases, takes 4.8 s of wall time (the slowest case, the first launch of the process, 0.5 s; an engine
forward 0.3 s).  No guard bit when the file was written."""
import ctypes as C
import itertools

import pytest
import torch
import torch.nn.functional as F

from tests import guarded as G
from tests.guarded_call import In, InOut, Out, Struct, Ws, guarded_call
from tests.test_gpu_eval import NV
from tests.test_gpu_rowops import (CONV_GATHER_CASES, LN_FLOOR, _conv3_gather_ref, _conv_gather_ref, _first_index_of, _in_class, _ln64,
                                   _nearest_table, _repack_ref)

gpu = pytest.mark.gpu
STREAM = object()          # stands for the current stream in an argument list
D = 1280


def _r(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _ri(n, hi, seed):
    return torch.randint(0, hi, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)


def _rotations(*lead, seed, scale=1.0):
    """exact-enough rotation matrices (..., 3, 3) in fp32: exp of a random skew matrix (axis-angle ~ scale * N(0, 1)), computed in fp64"""
    w = scale * torch.randn(*lead, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    K = torch.zeros(*lead, 3, 3, dtype=torch.float64)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 2] = -w[..., 2], w[..., 1], -w[..., 0]
    K[..., 1, 0], K[..., 2, 0], K[..., 2, 1] = w[..., 2], -w[..., 1], w[..., 0]
    return torch.linalg.matrix_exp(K).float()


def _prod(**axes):
    return [dict(zip(axes, v)) for v in itertools.product(*axes.values())]


# ================================================================================================ the builders
# Each takes the case's parameters and returns the argument list of its entry point, in the header's order.
def b_layernorm(rows, D, relu):
    return [In("x", _r(rows, D, seed=1) + 0.3), In("gamma", 1 + 0.1 * _r(D, seed=2)), In("beta", 0.1 * _r(D, seed=3)), Out("y", (rows, D)),
            rows, D, 1e-6, relu, STREAM]


def b_splitk_resid_ln(rows, S, split3, inplace):
    part, bias, resid = In("part", _r(S, rows, D, seed=10 + S)), In("bias", _r(D, seed=2)), _r(rows, D, seed=3, scale=3.0)
    r = InOut("resid == xout", resid) if inplace else In("resid", resid)
    xout = r if inplace else Out("xout", (rows, D))
    y = Out("y", (rows, D // 8, 3, 8), torch.int16) if split3 else Out("y", (rows, D))
    return [part, S, rows, D, bias, r, xout, In("gamma", 1 + 0.1 * _r(D, seed=4)), In("beta", 0.1 * _r(D, seed=5)), y, 1e-6, int(split3),
            STREAM]


def b_add_ln64(rows):
    return [In("x", _r(rows, 64, seed=40, scale=3.0) + 0.7), In("y", _r(rows, 64, seed=41)), In("gamma", 1 + 0.1 * _r(64, seed=42)),
            In("beta", 0.1 * _r(64, seed=43)), Out("s_out", (rows, 64)), Out("z_out", (rows, 64)), rows, 1e-5, STREAM]


def b_softmax_argmax(rows, outs):
    return [In("logits", _r(rows, 2048, seed=60 + rows)), Out("probs", (rows, 2048)) if "probs" in outs else None,
            Out("idx", (rows,), torch.int32) if "idx" in outs else None, rows, STREAM]


def b_vq_argmin_rows(rows, dist):
    x, cb = _r(rows, 256, seed=80 + rows), _r(2048, 256, seed=81)
    return [In("x", x), In("dot", x @ cb.t()), In("cnorm", (cb * cb).sum(-1)), Out("idx", (rows,), torch.int32),
            Out("dist", (rows, 2048)) if dist else None, rows, STREAM]


def b_code_norm(ncode):
    return [In("cb", _r(ncode, 256, seed=90, scale=0.3)), Out("cn", (ncode,)), ncode, STREAM]


def b_token_ce(rows):
    """targets in [0, 2047); the pad is class 2047, which no row names"""
    from tokenhmr_amd import _cabi
    return [In("x", _r(rows, 2048, seed=300 + rows)), In("target", _ri(rows, 2047, 301), pad=2047), rows, Out("out", ()),
            Ws("workspace", _cabi.TOKEN_CE_WS_PER_ROW * rows), STREAM]


def b_rot6d(n):
    return [In("x", _r(n, 6, seed=200 + n)), Out("R", (n, 3, 3)), n, STREAM]


def b_rot6d_backward(n):
    return [In("x", _r(n, 6, seed=200 + n)), In("grad_R", _r(n, 3, 3, seed=201)), Out("grad_x", (n, 6)), n, STREAM]


def b_aa_to_rotmat(n):
    return [In("aa", _r(n, 3, seed=210 + n, scale=0.6)), Out("R", (n, 3, 3)), n, STREAM]


def b_aa_to_rotmat_backward(n):
    return [In("aa", _r(n, 3, seed=210 + n, scale=0.6)), In("grad_R", _r(n, 3, 3, seed=211)), Out("grad_aa", (n, 3)), n, STREAM]


def b_rotmat_to_aa(n):
    """angles ~ 0.6 * |N(0, 1)^3|: below pi, where the result is well conditioned"""
    return [In("R", _rotations(n, seed=220 + n, scale=0.6)), Out("aa", (n, 3)), n, STREAM]


def b_decoder_init(B, E):
    return [In("bias", _r(E, seed=160)), In("pos", _r(E, seed=161)), Out("x", (B, E)), B, E, STREAM]


def b_conv_repack(co, ci, cp, kk):
    return [In("w", _r(co, ci, kk, seed=130)), Out("wp", (co, kk * cp)), co, ci, cp, kk, STREAM]


def _src(table, Tin):
    """the resampling table as an input whose pad is index Tin: for the last item of the batch the row behind its signal, which holds
    canaries; for an earlier item the next item's first row, which is real data — another row than any the table names, so the result
    changes either way"""
    return None if table is None else In("src", table, pad=Tin)


def b_conv3_gather(table, dil, Bn):
    Tin, Tout, Cc = (5, 10, 8) if table == "upsample" else (10, 10, 8)
    src = None if table == "none" else _nearest_table(Tin, Tout)
    return [In("in", _r(Bn, Tin, Cc, seed=110)), Out("out", (Bn, Tout, 3 * Cc)), _src(src, Tin), Bn, Tin, Tout, Cc, dil, 0, STREAM]


def b_conv_gather(case):
    Cc, Cp, ks, stride, pad, Tin, Tsrc, Tout, table = case
    src = _nearest_table(Tin, Tsrc) if table else None
    return [In("in", _r(2, Tin, Cc, seed=120)), Out("out", (2, Tout, ks * Cp)), _src(src, Tin), 2, Tin, Tsrc, Tout, Cc, Cp, ks, stride,
            pad, STREAM]


def b_im2col_patch(split3):
    img = (torch.arange(3 * 256 * 256, dtype=torch.float32) + 1).reshape(1, 3, 256, 256)
    return [In("img", img), Out("A", (192, 96, 3, 8), torch.int16) if split3 else Out("A", (192, 768)), 1, int(split3), STREAM]


def b_transpose(shape):
    Bn, R, Cc = shape
    return [In("in", torch.arange(Bn * R * Cc, dtype=torch.float32).reshape(Bn, R, Cc)), Out("out", (Bn, Cc, R)), Bn, R, Cc, STREAM]


def b_cross_attn(B, ldkv, koff):
    """everything outside the addressed 1024 columns is NaN, as in test_cross_attn; (6144, 5120): the last V column is the last element
    of its row, and of the window"""
    kv = torch.full((B * 192, ldkv), float("nan"))
    kv[:, koff:koff + 1024] = _r(B * 192, 1024, seed=101 + B)
    return [In("q", _r(B, 512, seed=100 + B)), In("kv", kv), ldkv, koff, Out("out", (B, 512)), B, STREAM]


HEAD_COLS = {"token": 31, "hmr2": 157}


def b_head_finish(kind, B, wide, optional):
    """ro (B, ldro): ldro exactly the columns the kind reads, or 8 more — those pad columns hold canaries.  optional: which of pose6d,
    cam_t and focal are given ("+"-joined; the others are NULL) — all, none, and each one alone, so that a kernel that guards one
    optional pointer with another's null test is caught"""
    cols = HEAD_COLS[kind]
    ldro = cols + (8 if wide else 0)
    ro = G._canary_buffer((B, ldro), torch.float32, "cpu")
    ro[:, :cols] = _r(B, cols, seed=150 + B)
    opt = lambda name, *s: Out(name, s) if name in optional.split("+") else None      # noqa: E731
    return [{"token": 0, "hmr2": 1}[kind], In("ro", ro), ldro, In("bpose", _r(B, 126, seed=151)) if kind == "token" else None,
            In("init_pose", _r(144, seed=152)), In("init_betas", _r(10, seed=153)), In("init_cam", _r(3, seed=154) + 2.0),
            opt("pose6d", B, 144), Out("rotmat", (B, 24, 3, 3)), Out("betas", (B, 10)), Out("cam", (B, 3)), opt("cam_t", B, 3),
            opt("focal", B, 2), 5000.0, 256.0, B, STREAM]


def b_vq_stats(rows, accumulate):
    """codes in [0, 2047): the pad is code 2047, which no row uses — consumed, it shows in code_count[2047]"""
    cc = InOut("code_count", _ri(2048, 50, 7)) if accumulate else Out("code_count", (2048,), torch.int32)
    return [In("x", _r(rows, 256, seed=400 + rows)), In("codebook", _r(2048, 256, seed=401)), In("idx", _ri(rows, 2047, 402), pad=2047), rows,
            cc, int(accumulate), Ws("partial_scratch", (rows + 31) // 32), Out("commit", ()), Out("perplexity", ()), STREAM]


def b_mean_row_dist(B, n, lo, hi):
    from tokenhmr_amd import _cabi
    return [In("a", _r(B, n, 3, seed=500 + n)), In("b", _r(B, n, 3, seed=501 + n)), n, lo, hi, B, Out("out", (1,)),
            Ws("workspace", _cabi.MEAN_ROW_DIST_WS), STREAM]


VAL_WEIGHTS, VAL_LOOSE_WEIGHT = (0.01, 0.05, 0.001, 0.001, 0.0005), 0.3
VAL_TAPS = {"kp2d_err": 44, "angle_err": 24, "valid2d": 44, "weak2d": 44, "valid_rot": 24, "weak_rot": 24, "conf2d_used": 44, "conf3d_used": 44}


def b_val_loss(B, loose, gt_rotmat):
    from tokenhmr_amd import _cabi
    conf = lambda *s, seed: (torch.rand(*s, generator=torch.Generator().manual_seed(seed)) > 0.3).float()      # noqa: E731
    pk2, pk3 = _r(B, 44, 2, seed=600, scale=0.3), _r(B, 44, 3, seed=601, scale=0.3)
    gk2 = torch.cat([pk2 + _r(B, 44, 2, seed=602, scale=0.05), conf(B, 44, 1, seed=603)], -1)
    gk3 = torch.cat([pk3 + _r(B, 44, 3, seed=604, scale=0.05), conf(B, 44, 1, seed=605)], -1)
    pose = _rotations(B, 24, seed=607) if gt_rotmat else _r(B, 72, seed=607, scale=0.5)
    ins = dict(pred_keypoints_2d=In("pred_keypoints_2d", pk2), pred_keypoints_3d=In("pred_keypoints_3d", pk3),
               pred_rotmat=In("pred_rotmat", _rotations(B, 24, seed=606)), pred_betas=In("pred_betas", _r(B, 10, seed=608)),
               gt_keypoints_2d=In("gt_keypoints_2d", gk2), gt_keypoints_3d=In("gt_keypoints_3d", gk3), gt_pose=In("gt_pose", pose),
               gt_betas=In("gt_betas", _r(B, 10, seed=609)), has_global_orient=In("has_global_orient", conf(B, seed=610)),
               has_body_pose=In("has_body_pose", conf(B, seed=611)), has_betas=In("has_betas", conf(B, seed=612)),
               valid_3d=None, kp2d_thresh=None, angle_thresh=None)
    outs = dict(losses=Out("losses", (6,)), per_item=Out("per_item", (B, 5)),
                running=InOut("running", torch.arange(7, dtype=torch.float64) * 0.25 + 1.0), has_betas_used=None, **{k: None for k in VAL_TAPS})
    if loose:
        ins.update(valid_3d=In("valid_3d", conf(B, seed=613)), kp2d_thresh=In("kp2d_thresh", _r(44, seed=614).abs() * 0.01),
                   angle_thresh=In("angle_thresh", _r(24, seed=615).abs() * 0.5))
        outs.update({k: Out(k, (B, n)) for k, n in VAL_TAPS.items()}, has_betas_used=Out("has_betas_used", (B,)))
    desc = _cabi.ValLossDesc(*VAL_WEIGHTS, VAL_LOOSE_WEIGHT, 39, _cabi.VAL_LOSS_LOOSE if loose else _cabi.VAL_LOSS_PLAIN, int(gt_rotmat), 0)
    return [C.byref(desc), Struct(_cabi.ValLossIn, **ins), B, Struct(_cabi.ValLossOut, **outs), Ws("workspace", _cabi.VAL_LOSS_WS_PER_ITEM * B),
            STREAM]


RECON_KINDS = {"l1": 0, "l2": 1, "l1_smooth": 2, "wt_l2": 3}


def b_tok_recon_loss(B, mesh, lo, hi, joints=True):
    from tokenhmr_amd import tokenizer_loss as TL          # WS_BASE, WS_PER_ITEM: the header's THMR_TOK_RECON_WS_*, held by tests/test_cabi_header.py
    def pair(name, *s, seed):
        gt = _r(*s, seed=seed)
        return In("pred_" + name, gt + _r(*s, seed=seed + 1, scale=0.7)), In("gt_" + name, gt)
    (pr, gr), (pv, gv) = pair("rotmat", B, 21, 3, 3, seed=700), pair("verts", B, 6890, 3, seed=702)
    pj, gj = pair("joints", B, 73, 3, seed=704) if joints else (None, None)
    vw = In("vert_weights", _r(6890, 3, seed=706).abs()) if mesh == "wt_l2" else None
    return [pr, gr, pv, gv, pj, gj, vw, In("commit", torch.tensor([0.37])), RECON_KINDS["l2"], RECON_KINDS[mesh], RECON_KINDS["l1_smooth"], lo, hi,
            20.0, 100.0, 100.0, 0.5, 2.0, B, Out("losses", (4,)), Out("grad_rotmat", (B, 21, 3, 3)), Out("grad_verts", (B, 6890, 3)),
            Out("grad_joints", (B, 73, 3)) if joints else None, Ws("workspace", TL.WS_BASE + TL.WS_PER_ITEM * B), STREAM]


EVAL_NJ = 70


def b_eval_pose(n_kp, gt_stride, pelvis_mode, n_verts, B):
    """the keypoint list is n_kp distinct joints of [0, 69); its pad is joint 69, which the list never names"""
    gt = _r(B, EVAL_NJ, gt_stride, seed=800) * torch.tensor([0.3, 0.2, 0.1, 1.0][:gt_stride])
    pred = gt[..., :3] * 1.1 + 0.05 + _r(B, EVAL_NJ, 3, seed=801, scale=0.02)
    kp = torch.randperm(EVAL_NJ - 1, generator=torch.Generator().manual_seed(802))[:n_kp].to(torch.int32)
    verts = [In("pred_verts", _r(B, n_verts, 3, seed=803)), In("gt_verts", _r(B, n_verts, 3, seed=804))] if n_verts else [None, None]
    return [In("pred_joints", pred), In("gt_joints", gt), EVAL_NJ, gt_stride, In("kp_list", kp, pad=EVAL_NJ - 1), n_kp, 3, pelvis_mode, *verts,
            n_verts, B, Out("mpjpe_mm", (B,)), Out("re_mm", (B,)), Out("pve_mm", (B,)) if n_verts else None, Out("pelvis_scratch", (B, 6)), STREAM]


def b_regress_joints(nj, nv, B):
    return [In("J", _r(nj, nv, seed=810).abs() / nv), In("verts", _r(B, nv, 3, seed=811)), nj, nv, B, Out("out", (B, nj, 3)), STREAM]


RECORD = [("pred_vertices", 20670), ("pred_keypoints_3d", 132), ("pred_keypoints_2d", 88), ("rotmat", 216), ("betas", 10), ("pred_cam", 3),
          ("pred_cam_t", 3)]


def b_pack_records(B):
    from tokenhmr_amd import _cabi
    f = {name: In(name, _r(B, n, seed=900 + n)) for name, n in RECORD}
    f["token_idx"] = In("token_idx", _ri(B * 160, 2047, 901).reshape(B, 160), pad=2047)
    f.update({k: None for k in _cabi.OUTPUT_FIELDS if k not in f})
    return [Struct(_cabi.Outputs, **f), B, Out("rec", (B, 21282)), STREAM]


POOL = 11          # row b of a body-model batch holds pool item b % 11 (coprime to every crops-per-pass value): 11 float64 references serve any B


def _pool(t, B):
    return t[torch.arange(B) % POOL].contiguous()


def b_smpl_forward(B, pose2rot):
    pose = _r(POOL, 72, seed=1000, scale=0.6) if pose2rot else _rotations(POOL, 24, seed=1000)
    return ["smpl", In("pose", _pool(pose, B)), int(pose2rot), In("betas", _pool(_r(POOL, 10, seed=1001), B)), B, Out("verts", (B, 6890, 3)), Out("joints", (B, 44, 3)),
            STREAM]


def b_smplh_forward(folded, B, transl, joints):
    return ["smplh", In("pose", _pool(_rotations(POOL, 22 if folded else 52, seed=1100), B)), 0, In("betas", _pool(_r(POOL, 10, seed=1101), B)),
            In("transl", _pool(_r(POOL, 3, seed=1102), B)) if transl else None, int(folded), B, Out("verts", (B, 6890, 3)),
            Out("joints", (B, 73, 3)) if joints else None, STREAM]


# ---- the engine's sub-paths: the first argument is the engine ("token" / "hmr2"), the rest as above
def _outputs(B, hmr2=False, **skip):
    from tokenhmr_amd import _cabi
    shapes = dict(pred_cam=(B, 3), rotmat=(B, 24, 3, 3), betas=(B, 10), cls_logits_softmax=(B, 160, 2048), pred_cam_t=(B, 3), focal_length=(B, 2),
                  pred_keypoints_3d=(B, 44, 3), pred_vertices=(B, 6890, 3), pred_keypoints_2d=(B, 44, 2), token_idx=(B, 160),
                  vit_features=(B, 192, 1280), token_out=(B, 1024), cls_logits=(B, 160, 2048), pose6d=(B, 144))
    drop = set(skip) | ({"token_idx", "cls_logits_softmax", "cls_logits"} if hmr2 else set())
    return Struct(_cabi.Outputs, **{k: None if k in drop else Out(k, shapes[k], torch.int32 if k == "token_idx" else torch.float32)
                                    for k in _cabi.OUTPUT_FIELDS})


def b_forward(head, B, vit_gemm):
    return [head, In("img", _r(B, 3, 256, 256, seed=1200 + B)), B, _outputs(B, head == "hmr2"), STREAM]


def b_vit_forward(B):
    return ["token", In("img", _r(B, 3, 256, 256, seed=1200 + B)), B, Out("feats", (B, 192, 1280)), STREAM]


def b_head_forward(head, B):
    return [head, In("ctx", _r(B, 192, 1280, seed=1210 + B)), B, _outputs(B, head == "hmr2", vit_features=1), STREAM]


def b_lbs_forward(B, cam):
    return ["token", In("rotmat", _rotations(B, 24, seed=1220)), In("betas", _r(B, 10, seed=1221)), In("cam", _r(B, 3, seed=1222) + 2.0) if cam else None,
            B, Out("verts", (B, 6890, 3)), Out("joints", (B, 44, 3)), Out("cam_t", (B, 3)) if cam else None,
            Out("kp2d", (B, 44, 2)) if cam else None, STREAM]


def b_vq_argmin(rows, dist):
    return ["token", In("x", _r(rows, 256, seed=1230 + rows)), rows, Out("idx", (rows,), torch.int32), Out("dist", (rows, 2048)) if dist else None,
            STREAM]


def _pose6d(B):
    return _rotations(B, 21, seed=1240 + B)[..., :2, :].reshape(B, 21, 6).contiguous()


def b_encode_tokens(B, latent):
    return ["token", In("pose", _pose6d(B)), B, Out("idx", (B, 160), torch.int32), Out("latent", (B, 160, 256)) if latent else None, STREAM]


def b_vq_decode(B):
    return ["token", In("probs", _r(B, 160, 2048, seed=1250).softmax(-1)), B, Out("pose6d", (B, 21, 6)), STREAM]


def b_vq_decode_idx(B):
    """the pad is code 2047, which no position names: in range (nothing is clamped, no error flag), and another code row if consumed"""
    return ["token", In("idx", _ri(B * 160, 2047, 1260).reshape(B, 160), pad=2047), B, Out("pose6d", (B, 21, 6)), STREAM]


def b_tokenizer_roundtrip(B, accumulate):
    from tokenhmr_amd import _cabi
    cc = InOut("code_count", _ri(2048, 50, 8)) if accumulate else Out("code_count", (2048,), torch.int32)
    out = Struct(_cabi.TokenizerOut, idx=Out("idx", (B, 160), torch.int32), latent=Out("latent", (B, 160, 256)), pose6d=Out("pose6d", (B, 21, 6)),
                 rotmat=Out("rotmat", (B, 21, 3, 3)), aa=Out("aa", (B, 21, 3)), commit_loss=Out("commit_loss", ()),
                 perplexity=Out("perplexity", ()), code_count=cc, accumulate_counts=int(accumulate), reserved=0)
    return ["token", In("pose6d_in", _pose6d(B)), B, out, STREAM]


# ================================================================================================ the table
ROWS4 = [1, 4, 5]                # one wave per row, four rows per 256-thread workgroup
N256 = [1, 255, 256, 257]        # one element per thread, 256 per workgroup
CASES = {
    "thmr_op_layernorm": (b_layernorm, _prod(rows=ROWS4, D=[1280, 1024, 100], relu=[0, 1])),
    "thmr_op_splitk_resid_ln": (b_splitk_resid_ln, _prod(rows=ROWS4, S=[1, 2, 3, 4], split3=[False], inplace=[False, True]) +
                                _prod(rows=ROWS4, S=[2, 4], split3=[True], inplace=[False, True])),
    "thmr_op_add_ln64": (b_add_ln64, _prod(rows=ROWS4)),
    "thmr_op_softmax_argmax": (b_softmax_argmax, _prod(rows=ROWS4, outs=["probs", "idx", "probs+idx"])),
    "thmr_op_vq_argmin_rows": (b_vq_argmin_rows, _prod(rows=ROWS4, dist=[False, True])),
    "thmr_op_code_norm": (b_code_norm, _prod(ncode=[1, 5])),
    "thmr_op_token_ce": (b_token_ce, _prod(rows=ROWS4)),
    "thmr_op_rot6d": (b_rot6d, _prod(n=N256)),
    "thmr_op_rot6d_backward": (b_rot6d_backward, _prod(n=N256)),
    "thmr_op_aa_to_rotmat": (b_aa_to_rotmat, _prod(n=N256)),
    "thmr_op_aa_to_rotmat_backward": (b_aa_to_rotmat_backward, _prod(n=N256)),
    "thmr_op_rotmat_to_aa": (b_rotmat_to_aa, _prod(n=N256)),
    "thmr_op_decoder_init": (b_decoder_init, [dict(B=3, E=100), dict(B=1, E=1024)]),
    "thmr_op_conv_repack": (b_conv_repack, [dict(co=co, ci=ci, cp=cp, kk=kk) for co, ci, cp, kk in ((16, 32, 32, 3), (5, 8, 8, 4), (16, 6, 32, 3), (3, 5, 7, 1))]),
    "thmr_op_conv3_gather": (b_conv3_gather, _prod(table=["none", "identity", "upsample"], dil=[1, 27], Bn=[1, 2])),
    "thmr_op_conv_gather": (b_conv_gather, _prod(case=CONV_GATHER_CASES)),
    "thmr_op_im2col_patch": (b_im2col_patch, _prod(split3=[False, True])),
    "thmr_op_transpose": (b_transpose, _prod(shape=[(1, 33, 31), (2, 32, 64), (1, 1, 1)])),
    "thmr_op_cross_attn": (b_cross_attn, [dict(B=B, ldkv=ld, koff=k) for B in (1, 3) for ld, k in ((6144, 5120), (1024, 0))]),
    "thmr_op_head_finish": (b_head_finish, _prod(kind=["token", "hmr2"], B=[1, 5], wide=[False, True], optional=["pose6d+cam_t+focal", "none"]) +
                            _prod(kind=["token", "hmr2"], B=[5], wide=[False], optional=["pose6d", "cam_t", "focal"])),
    "thmr_op_vq_stats": (b_vq_stats, _prod(rows=[1, 32, 33], accumulate=[False, True])),
    "thmr_op_mean_row_dist": (b_mean_row_dist, [dict(B=1, n=1, lo=0, hi=1), dict(B=2, n=73, lo=1, hi=22), dict(B=3, n=63, lo=0, hi=63)]),
    "thmr_val_loss": (b_val_loss, _prod(B=[1, 4, 5], loose=[False, True], gt_rotmat=[False, True])),
    "thmr_tok_recon_loss": (b_tok_recon_loss, [dict(B=1, mesh="l1", lo=1, hi=22), dict(B=3, mesh="l2", lo=0, hi=73),
                                               dict(B=1, mesh="l1_smooth", lo=0, hi=73), dict(B=3, mesh="wt_l2", lo=1, hi=22),
                                               dict(B=3, mesh="l2", lo=1, hi=22, joints=False)]),
    "thmr_eval_pose": (b_eval_pose, _prod(n_kp=[2, 14, 64], gt_stride=[3, 4], pelvis_mode=[0, 1], n_verts=[0, NV[0], NV[4]], B=[1, 3])),
    "thmr_regress_joints": (b_regress_joints, _prod(nj=[1, 24], nv=[NV[0], NV[4]], B=[1, 3])),
    "thmr_pack_records": (b_pack_records, _prod(B=[1, 5])),
    # launch_lbs (csrc/body_model.hip) on a handle of max_batch 72: cg 1; a second pass; cg 2 with a ragged last pass
    "thmr_smpl_forward": (b_smpl_forward, _prod(B=[1, 33, 65], pose2rot=[False, True])),
    "thmr_smplh_forward": (b_smplh_forward, _prod(folded=[False, True], B=[1, 9], transl=[False, True], joints=[True, False])),
    "thmr_forward": (b_forward, _prod(head=["token"], B=[1, 3], vit_gemm=["f32", "split3"]) + [dict(head="hmr2", B=3, vit_gemm="split3")]),
    "thmr_vit_forward": (b_vit_forward, _prod(B=[1, 3])),
    "thmr_head_forward": (b_head_forward, _prod(head=["token", "hmr2"], B=[1, 3])),
    "thmr_lbs_forward": (b_lbs_forward, _prod(B=[1, 3], cam=[False, True])),
    "thmr_vq_argmin": (b_vq_argmin, _prod(rows=ROWS4, dist=[False, True])),
    "thmr_encode_tokens": (b_encode_tokens, _prod(B=[1, 3], latent=[False, True])),
    "thmr_vq_decode": (b_vq_decode, _prod(B=[1, 3])),
    "thmr_vq_decode_idx": (b_vq_decode_idx, _prod(B=[1, 3])),
    "thmr_tokenizer_roundtrip": (b_tokenizer_roundtrip, _prod(B=[1, 3], accumulate=[False, True])),
}

# every other entry point of the header that takes a device output pointer, and why it has no case here
_STRIDED, _GRAD = "covered by tests/test_gpu_strided.py", "covered by tests/test_gpu_smpl_grad.py"
_CODEC = "a codec handle, with canary tests of its own"
_OUT_OF_SCOPE = "cropper and renderer: out of scope here, they have edge files of their own"
EXEMPT = {
    "thmr_op_gemm": _STRIDED, "thmr_op_split3": _STRIDED, "thmr_op_gemm_split3": _STRIDED, "thmr_op_gemm_split3_out_split3": _STRIDED,
    "thmr_op_vit_attention": _STRIDED, "thmr_op_vit_attention_variant": _STRIDED, "thmr_op_vit_attention_split3": _STRIDED,
    "thmr_op_vit_attention_b16": _STRIDED,
    "thmr_smpl_backward": _GRAD, "thmr_smplh_backward": "covered by tests/test_gpu_smplh_grad.py",
    "thmr_jpeg_decode_batch": _CODEC, "thmr_png_decode_batch": _CODEC,
    "thmr_cropper_run": _OUT_OF_SCOPE, "thmr_cropper_run_frames": _OUT_OF_SCOPE, "thmr_renderer_run": _OUT_OF_SCOPE,
    "thmr_renderer_sheet": _OUT_OF_SCOPE,
    "thmr_allgather_records": "a collective: needs a communicator",
    "thmr_create": "takes the two arenas, which the engine owns from then on: they are no call's output (tests/test_gpu_arena_layout.py)",
}


def _params():
    for entry, (_, cases) in CASES.items():
        for i, kw in enumerate(cases):
            yield pytest.param(entry, i, id=entry[5:] + "-" + "-".join(f"{k}={v}" for k, v in kw.items()).replace(" ", ""))


# ================================================================================================ handles, made once
class _Handles:
    def __init__(self):
        self.made = {}

    def get(self, key, dev):
        if key not in self.made:
            self.made[key] = getattr(self, "_" + key)(dev)
        return self.made[key]

    @staticmethod
    def _smpl(dev):
        from tokenhmr_amd.smpl import SMPL
        from tokenhmr_amd.smpl_assets import make_synthetic_smpl
        c = make_synthetic_smpl(seed=0)
        c["update_hips"] = True
        return SMPL(c, max_batch=72, device=dev)

    @staticmethod
    def _smplh(dev):
        from tokenhmr_amd.smplh import SMPLHLayer
        from tokenhmr_amd.smpl_assets import make_synthetic_smplh
        m = SMPLHLayer(make_synthetic_smplh(0), max_batch=16, device=dev)
        m._handle()
        return m

    @staticmethod
    def _engine(dev, head):
        from tokenhmr_amd import weights as W
        from tokenhmr_amd.config import HMRConfig
        from tokenhmr_amd.engine import Engine
        from tokenhmr_amd.smpl_assets import make_synthetic_smpl
        cfg = HMRConfig(vit_depth=1, dec_depth=1, head=head) if head else HMRConfig(vit_depth=1, dec_depth=1)
        eng = Engine(cfg, max_batch=8, device=dev)
        if head:
            eng.load_state(W.make_synthetic_state(cfg, 0))
        else:
            eng.load_state(W.make_synthetic_state(cfg, 0), dict(W.make_synthetic_tokenizer(cfg, 0), **W.make_synthetic_encoder(cfg, 0)))
        eng.load_smpl(make_synthetic_smpl(cfg, 0))
        eng.finalize()
        return eng

    def _token(self, dev):
        return self._engine(dev, None)

    def _hmr2(self, dev):
        return self._engine(dev, "hmr2")

    def close(self):
        for h in self.made.values():
            h.close()
        self.made.clear()


@pytest.fixture(scope="module")
def handles():
    h = _Handles()
    yield h
    h.close()


# ================================================================================================ the float64 / exact statements
def _st_layernorm(kw, r):
    x, g, b = (r.plain[k].cpu() for k in ("x", "gamma", "beta"))
    ref64, ref32 = _ln64(x, g, b, 1e-6), F.layer_norm(x, x.shape[-1:], g, b, 1e-6)
    if kw["relu"]:
        ref64, ref32 = ref64.relu(), ref32.relu()
    assert _in_class(f"layernorm {kw}", r.guarded["y"], ref64, ref32, **LN_FLOOR)                     # (C)


def _st_add_ln64(kw, r):
    x, y, g, b = (r.plain[k].cpu() for k in ("x", "y", "gamma", "beta"))
    assert torch.equal(r.guarded["s_out"].cpu(), x + y)                                               # (E)
    assert _in_class(f"add_ln64 {kw}", r.guarded["z_out"], _ln64(x + y, g, b, 1e-5), F.layer_norm(x + y, (64,), g, b, 1e-5), **LN_FLOOR)


def _st_decoder_init(kw, r):
    assert torch.equal(r.guarded["x"].cpu(), (r.plain["bias"] + r.plain["pos"]).cpu().expand(kw["B"], kw["E"]))          # (E)


def _st_conv_repack(kw, r):
    assert torch.equal(r.guarded["wp"].cpu(), _repack_ref(r.plain["w"].cpu(), kw["cp"]))              # (E)


def _st_conv3_gather(kw, r):
    src = r.plain["src"].cpu() if "src" in r.plain else None
    assert torch.equal(r.guarded["out"].cpu(), _conv3_gather_ref(r.plain["in"].cpu(), src, 10, kw["dil"], False))       # (E)


def _st_conv_gather(kw, r):
    _, Cp, ks, stride, pad, _, Tsrc, Tout, _ = kw["case"]
    src = r.plain["src"].cpu() if "src" in r.plain else None
    assert torch.equal(r.guarded["out"].cpu(), _conv_gather_ref(r.plain["in"].cpu(), src, Tsrc, Tout, Cp, ks, stride, pad))      # (E)


def _st_transpose(kw, r):
    assert torch.equal(r.guarded["out"].cpu(), r.plain["in"].cpu().transpose(1, 2).contiguous())      # (E)


def _st_code_norm(kw, r):
    ref = (r.plain["cb"].cpu().double() ** 2).sum(-1)
    assert ((r.guarded["cn"].cpu().double() - ref).abs() <= 10 * 2.0 ** -24 * ref).all()              # (B) test_code_norm's bound


def _st_pack_records(kw, r):
    want = torch.cat([r.plain[n].view(torch.float32).reshape(kw["B"], -1) for n, _ in RECORD + [("token_idx", 160)]], 1)
    assert torch.equal(r.guarded["rec"].view(torch.int32), want.view(torch.int32))                    # (E) raw words


def _st_vq_stats(kw, r):
    idx = r.plain["idx"].cpu().long()
    hist = torch.bincount(idx, minlength=2048).int() + (_ri(2048, 50, 7) if kw["accumulate"] else 0)
    assert torch.equal(r.guarded["code_count"].cpu(), hist)                                           # (E)


def _st_splitk_resid_ln(kw, r):
    part, acc = r.plain["part"].cpu(), r.plain["part"][0].cpu().clone()
    for s in range(1, kw["S"]):          # the kernel's written order: (((p0 + p1) + p2) + ...), then + bias, then resid + (...)
        acc = acc + part[s]
    xref = _r(kw["rows"], D, seed=3, scale=3.0) + (acc + r.plain["bias"].cpu())
    xout = r.guarded["resid == xout" if kw["inplace"] else "xout"].cpu()
    assert torch.equal(xout, xref)                                                                    # (E)
    if not kw["split3"]:
        g, b = r.plain["gamma"].cpu(), r.plain["beta"].cpu()
        assert _in_class(f"splitk_resid_ln {kw}", r.guarded["y"], _ln64(xout, g, b, 1e-6), F.layer_norm(xout, (D,), g, b, 1e-6), **LN_FLOOR)


def _st_softmax_argmax(kw, r):
    logits = r.plain["logits"].cpu()
    if "idx" in kw["outs"]:
        assert torch.equal(r.guarded["idx"].cpu(), _first_index_of(logits, logits.max(-1, keepdim=True).values))         # (E)
    if "probs" in kw["outs"]:
        assert (r.guarded["probs"].cpu().double().sum(-1) - 1).abs().max().item() <= 1e-5             # (B) test_softmax_probs' bound


def _st_vq_argmin_rows(kw, r):
    if kw["dist"]:
        dist = r.guarded["dist"].cpu()
        assert torch.equal(r.guarded["idx"].cpu(), _first_index_of(dist, dist.min(-1, keepdim=True).values))            # (E)


def _st_head_finish(kw, r):
    ro, ip, B = r.plain["ro"].cpu(), r.plain["init_pose"].cpu(), kw["B"]
    shape, cam = (slice(6, 16), slice(16, 19)) if kw["kind"] == "token" else (slice(144, 154), slice(154, 157))
    assert torch.equal(r.guarded["betas"].cpu(), ro[:, shape] + r.plain["init_betas"].cpu())         # (E)
    assert torch.equal(r.guarded["cam"].cpu(), ro[:, cam] + r.plain["init_cam"].cpu())               # (E)
    if "pose6d" in r.guarded:
        p6 = (torch.cat([ro[:, :6], r.plain["bpose"].cpu(), ro[:, 19:31]], 1) if kw["kind"] == "token" else ro[:, :144]) + ip
        assert torch.equal(r.guarded["pose6d"].cpu(), p6)                                             # (E)
    if "focal" in r.guarded:
        assert torch.equal(r.guarded["focal"].cpu(), torch.full((B, 2), 5000.0))                      # (E)
    if "cam_t" in r.guarded:
        c = (ro[:, cam] + r.plain["init_cam"].cpu()).double()
        want = torch.stack([c[:, 1], c[:, 2], 2 * 5000.0 / (256.0 * c[:, 0] + 1e-9)], 1)
        assert ((r.guarded["cam_t"].cpu().double() - want).abs() <= 1e-6 * want.abs()).all()          # (B) test_head_finish's rtol


REL_FLOOR = 1e-5          # tests/test_gpu_val_loss.py::REL_FLOOR (held equal in test_the_floors_are_the_parity_files)
TOL_M = 2e-6              # tests/test_smpl_bounds.py::TOL_M, tests/test_gpu_smplh.py::FLOOR_M: metres


def _st_token_ce(kw, r):
    """(B) test_token_ce_against_fp64's: the mean and the per-row losses left in the workspace, relative to fp64 logsumexp"""
    import numpy as np
    from tests import val_loss_oracle as VO
    x, t = r.plain["x"].cpu().numpy(), r.plain["target"].cpu().numpy()
    ref = VO.token_ce64(x, t)
    assert abs(float(r.guarded["out"]) - ref) <= REL_FLOOR * abs(ref), (float(r.guarded["out"]), ref)
    row64 = np.array([VO.token_ce64(x[i:i + 1], t[i:i + 1]) for i in range(kw["rows"])])
    assert np.abs(r.guarded["workspace"].cpu().double().numpy() - row64).max() <= REL_FLOOR * np.abs(row64).max()


def _st_rot6d(kw, r):
    """test_rot6d's: the oracle within 1e-6, orthonormal with det 1 to 1e-5"""
    from oracle import tokenhmr_oracle as O
    R = r.guarded["R"].cpu()
    assert torch.allclose(R, O.rot6d_to_rotmat(r.plain["x"].cpu()).reshape(-1, 3, 3), atol=1e-6)
    assert torch.allclose(R @ R.transpose(1, 2), torch.eye(3).expand_as(R), atol=1e-5)
    assert torch.allclose(torch.linalg.det(R), torch.ones(kw["n"]), atol=1e-5)


def _st_rot6d_backward(kw, r):
    """test_gpu_rot6d_backward's: float64 autograd of the forward, the device at most 2 x as far from it as fp32 autograd"""
    from tests import smplh_backward_numpy as HB
    from tests import stage_bounds as SB
    x, gR = r.plain["x"].cpu(), r.plain["grad_R"].cpu()

    def truth(dtype):
        t = x.to(dtype).clone().requires_grad_(True)
        return torch.autograd.grad((HB.rot6d_generic(t) * gR.to(dtype)).sum(), t)[0]
    ok, line = SB.check(f"rot6d backward {kw}", r.guarded["grad_x"].cpu(), truth(torch.float32), truth(torch.float64), 2.0)
    assert ok, line


def _st_aa_to_rotmat(kw, r):
    """test_aa_to_rotmat_vs_reference_golden's: fp64 of the reference's formula within 2e-6"""
    from oracle import tokenhmr_oracle as O
    assert (r.guarded["R"].cpu().double() - O.aa_to_rotmat(r.plain["aa"].cpu().double())).abs().max() < 2e-6


def _st_rotmat_to_aa(kw, r):
    """test_rotmat_to_aa_against_the_reference's rule: max(1e-6, 2 x the formula's own fp32-vs-float64 distance), per element"""
    import numpy as np
    from tests import val_loss_oracle as VO
    R = r.plain["R"].cpu().numpy()
    r64, r32 = VO.matrix_to_axis_angle64(R), VO.matrix_to_axis_angle64(R, np.float32)
    d, bound = np.abs(r.guarded["aa"].cpu().double().numpy() - r64).max(), max(1e-6, 2.0 * np.abs(r32.astype(np.float64) - r64).max())
    print(f"rotmat_to_aa {kw}: max|diff| {d:.2e} (bound {bound:.1e})")
    assert d <= bound


def _st_mean_row_dist(kw, r):
    """test_mean_row_dist_against_fp64's: relative error <= 1e-5"""
    from tests import smplh_oracle as S
    ref = S.mean_row_dist64(r.plain["a"].cpu().numpy(), r.plain["b"].cpu().numpy(), kw["lo"], kw["hi"])
    assert abs(float(r.guarded["out"]) - ref) <= 1e-5 * ref, (float(r.guarded["out"]), ref)


def _st_val_loss(kw, r):
    """_check_against_oracle's of tests/test_gpu_val_loss.py: the six losses and the per-item terms at the relative floor against the
    fp64 oracle; has_betas_used (E); `running` (E): one fp64 addition of each fp32 loss, and of 1"""
    import numpy as np
    from tests import val_loss_oracle as VO
    inp = {k: v.cpu().numpy() for k, v in r.plain.items()}
    inp["gt_pose_rotmat" if kw["gt_rotmat"] else "gt_pose_aa"] = inp["gt_pose"]
    thr = dict(kp2d=inp["kp2d_thresh"], global_orient=inp["angle_thresh"][:1], body_pose=inp["angle_thresh"][1:]) if kw["loose"] else None
    want = VO.val_loss64(inp, VAL_WEIGHTS, loose=kw["loose"], loose_weight=VAL_LOOSE_WEIGHT, thresholds=thr, valid_3d=inp.get("valid_3d"),
                         gt_is_axis_angle=not kw["gt_rotmat"])
    losses = r.guarded["losses"].cpu()
    assert (np.abs(losses.double().numpy() - want["losses"]) <= REL_FLOOR * np.abs(want["losses"])).all(), (losses, want["losses"])
    assert (np.abs(r.guarded["per_item"].cpu().double().numpy() - want["per_item"]) <= REL_FLOOR * np.abs(want["per_item"])).all()
    if kw["loose"]:
        assert np.array_equal(r.guarded["has_betas_used"].cpu().double().numpy(), want["has_betas_used"])
    before = torch.arange(7, dtype=torch.float64) * 0.25 + 1.0
    assert torch.equal(r.guarded["running"].cpu(), before + torch.cat([losses.double(), torch.ones(1, dtype=torch.float64)]))      # (E)


def _st_regress_joints(kw, r):
    """test_regress_joints' (B): (ceil(nv / 256) + 10) U sum |J| |verts| per element"""
    from tests.test_gpu_eval import _check_regress
    _check_regress(f"regress {kw}", r.guarded["out"], r.plain["J"].cpu(), r.plain["verts"].cpu())


_BODY_REF = {}


def _smpl_ref(pose2rot):
    """(verts64, joints64, bound_v, bound_j) of the POOL items: the independent fp64 derivation (oracle/lbs_independent.py), and
    max(TOL_M, 2 x the oracle's own fp32 distance to it) — test_gpu_lbs_crop_group_edges' bound and the project's rule"""
    import numpy as np
    from oracle import tokenhmr_oracle as O
    from oracle.lbs_independent import smpl_forward_independent
    from tests import smplh_oracle as S
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    if ("smpl", pose2rot) not in _BODY_REF:
        c = make_synthetic_smpl(seed=0)
        c["update_hips"] = True
        betas = _r(POOL, 10, seed=1001)
        if pose2rot:
            pose = _r(POOL, 72, seed=1000, scale=0.6)
            R64 = S.batch_rodrigues64(pose.double().numpy().reshape(-1, 3)).reshape(POOL, 24, 3, 3)
            v32, j32 = O.smpl_forward_axis_angle(pose[:, :3], pose[:, 3:], betas, c)
        else:
            pose = _rotations(POOL, 24, seed=1000)
            R64 = pose.double().numpy()
            v32, j32 = O.smpl_forward(pose[:, :1], pose[:, 1:], betas, c)
        v64, j64 = smpl_forward_independent(R64, betas.double().numpy(), c)
        _BODY_REF["smpl", pose2rot] = (v64, j64, max(TOL_M, 2 * np.abs(v32.double().numpy() - v64).max()),
                                       max(TOL_M, 2 * np.abs(j32.double().numpy() - j64).max()))
    return _BODY_REF["smpl", pose2rot]


def _st_smpl_forward(kw, r):
    import numpy as np
    v64, j64, bv, bj = _smpl_ref(kw["pose2rot"])
    sel = np.arange(kw["B"]) % POOL
    dv = np.abs(r.guarded["verts"].cpu().double().numpy() - v64[sel]).max()
    dj = np.abs(r.guarded["joints"].cpu().double().numpy() - j64[sel]).max()
    print(f"smpl_forward {kw}: verts {dv:.2e} m (bound {bv:.2e}), joints {dj:.2e} m (bound {bj:.2e})")
    assert dv <= bv and dj <= bj


def _smplh_ref(folded, transl):
    """as _smpl_ref, with tests/smplh_oracle.py's two references: test_full_and_folded_paths_match_independent_derivation's bound"""
    import numpy as np
    from tests import smplh_oracle as S
    from tokenhmr_amd.smpl_assets import make_synthetic_smplh
    if ("smplh", folded, transl) not in _BODY_REF:
        c = make_synthetic_smplh(0)
        R = _rotations(POOL, 22 if folded else 52, seed=1100)
        if folded:
            R = torch.cat([R, torch.eye(3).expand(POOL, 30, 3, 3)], 1)
        betas, t = _r(POOL, 10, seed=1101), _r(POOL, 3, seed=1102) if transl else None
        v64, j64 = S.smplh_forward_independent(R.double().numpy(), betas.double().numpy(), c, None if t is None else t.double().numpy())
        v32, j32 = S.smplh_forward_smplx32(R, betas, c, t)
        _BODY_REF["smplh", folded, transl] = (v64, j64, max(TOL_M, 2 * np.abs(v32.double().numpy() - v64).max()),
                                              max(TOL_M, 2 * np.abs(j32.double().numpy() - j64).max()))
    return _BODY_REF["smplh", folded, transl]


def _st_smplh_forward(kw, r):
    import numpy as np
    v64, j64, bv, bj = _smplh_ref(kw["folded"], kw["transl"])
    sel = np.arange(kw["B"]) % POOL
    dv = np.abs(r.guarded["verts"].cpu().double().numpy() - v64[sel]).max()
    dj = np.abs(r.guarded["joints"].cpu().double().numpy() - j64[sel]).max() if kw["joints"] else 0.0
    print(f"smplh_forward {kw}: verts {dv:.2e} m (bound {bv:.2e}), joints {dj:.2e} m (bound {bj:.2e})")
    assert dv <= bv and dj <= bj


STATEMENTS = {"thmr_op_token_ce": _st_token_ce, "thmr_op_rot6d": _st_rot6d, "thmr_op_rot6d_backward": _st_rot6d_backward,
              "thmr_op_aa_to_rotmat": _st_aa_to_rotmat, "thmr_op_rotmat_to_aa": _st_rotmat_to_aa, "thmr_op_mean_row_dist": _st_mean_row_dist,
              "thmr_val_loss": _st_val_loss, "thmr_regress_joints": _st_regress_joints, "thmr_smpl_forward": _st_smpl_forward,
              "thmr_smplh_forward": _st_smplh_forward,
              "thmr_op_layernorm": _st_layernorm, "thmr_op_splitk_resid_ln": _st_splitk_resid_ln, "thmr_op_softmax_argmax": _st_softmax_argmax,
              "thmr_op_vq_argmin_rows": _st_vq_argmin_rows, "thmr_op_head_finish": _st_head_finish, "thmr_op_add_ln64": _st_add_ln64, "thmr_op_decoder_init": _st_decoder_init,
              "thmr_op_conv_repack": _st_conv_repack, "thmr_op_conv3_gather": _st_conv3_gather, "thmr_op_conv_gather": _st_conv_gather,
              "thmr_op_transpose": _st_transpose, "thmr_op_code_norm": _st_code_norm, "thmr_pack_records": _st_pack_records,
              "thmr_op_vq_stats": _st_vq_stats}


# The entry points WITHOUT a statement here: every shape of their cases is one a parity test already holds to its reference, named here
# (tests/test_guarded_host.py requires every entry point of CASES in exactly one of STATEMENTS and COVERED_BY).
COVERED_BY = {
    "thmr_op_aa_to_rotmat_backward": "tests/test_gpu_smpl_grad.py::test_gpu_aa_to_rotmat_backward: n = 1, 255, 256, 257, against float64 autograd",
    "thmr_op_im2col_patch": "tests/test_gpu_rowops.py::test_im2col_patch[1]: B = 1, fp32 and split3, (E) against F.unfold",
    "thmr_op_cross_attn": "tests/test_gpu_rowops.py::test_cross_attn: B = 1 and 3 at (6144, 5120) and (1024, 0), (C) against fp64",
    "thmr_tok_recon_loss": "tests/test_gpu_tokenizer_loss.py::test_gpu_tok_recon_loss: B = 1 and 3, every kind on every term, both joint ranges, against "
                           "float64 autograd; one term alone (the others absent) in test_gpu_value_and_grad_end_to_end",
    "thmr_eval_pose": "tests/test_gpu_eval.py::test_eval_pose_sizes_modes_strides: 2, 14, 64 keypoints of 70 joints, both pelvis modes and strides; "
                      "test_pve: every n_verts of NV at B = 1 and 3; one wave per crop, test_eval_pose_crops_do_not_interact",
    "thmr_forward": "tests/test_gpu_model.py::test_odd_batch_sizes_vs_oracle (B = 1) and test_gpu_stage_fp64.py (3 crops and more, both modes, every "
                    "tap); tests/test_gpu_hmr2.py::test_full_forward_vs_oracle",
    "thmr_vit_forward": "tests/test_gpu_stage_fp64.py: the ViT stages in both modes; tests/test_gpu_model.py::test_odd_batch_sizes_vs_oracle",
    "thmr_head_forward": "tests/test_gpu_stage_fp64.py: the head stages; tests/test_gpu_hmr2.py for the HMR2 head",
    "thmr_lbs_forward": "tests/test_smpl_bounds.py::test_gpu_lbs_crop_group_edges and the 5-crop bound beside it: the kernels of thmr_smpl_forward, held "
                        "here at B = 1, 33, 65",
    "thmr_vq_argmin": "tests/test_gpu_rowops.py::test_vq_argmin_rows and this file's thmr_op_vq_argmin_rows statement: the same kernel behind the GEMM",
    "thmr_encode_tokens": "tests/test_tokenizer.py and tests/test_gpu_tokenizer_rt.py: encode against the oracle at B = 1 ... 9",
    "thmr_vq_decode": "tests/test_gpu_tokenizer_rt.py::test_hard_decode_is_bit_identical_to_one_hot and tests/test_tokenizer.py: both regimes",
    "thmr_vq_decode_idx": "tests/test_gpu_tokenizer_rt.py::test_hard_decode_is_bit_identical_to_one_hot: B = 2 and 7, (E)",
    "thmr_tokenizer_roundtrip": "tests/test_gpu_tokenizer_rt.py: the round trip against the reference's golden record and the CPU restatement",
}


# ================================================================================================ the tests
@gpu
@pytest.mark.parametrize("entry,i", list(_params()))
def test_guard_bands(built_lib, cuda_dev, handles, entry, i):
    builder, cases = CASES[entry]
    kw = cases[i]
    args = builder(**kw)
    error = lambda: (built_lib.thmr_last_error(None) or b"").decode()      # noqa: E731
    eng = None
    if isinstance(args[0], str):                                        # a handle: the body models, an engine
        h = handles.get(args[0], cuda_dev)
        if args[0] in ("token", "hmr2"):
            eng = h
            if "vit_gemm" in kw:
                eng.set_vit_gemm(kw["vit_gemm"])
            error = lambda: (built_lib.thmr_last_error(eng.h) or b"").decode()      # noqa: E731
        args[0] = h.h
    if entry == "thmr_pack_records":
        error = lambda: (built_lib.thmr_collective_last_error() or b"").decode()      # noqa: E731
    try:
        with torch.cuda.device(cuda_dev):
            args = [C.c_void_p(torch.cuda.current_stream(cuda_dev).cuda_stream) if a is STREAM else a for a in args]
            r = guarded_call(getattr(built_lib, entry), args, device=cuda_dev, label=f"{entry} {kw}", error_text=error)
        if eng is not None:
            eng.status()
    finally:
        if eng is not None:
            eng.set_vit_gemm("split3")          # the engine is shared by the module: a failed f32 case must not leave it in that mode
    if entry in STATEMENTS:
        STATEMENTS[entry](kw, r)


@gpu
@pytest.mark.parametrize("head,B,vit_gemm", [("token", 1, "f32"), ("token", 3, "f32"), ("token", 1, "split3"), ("token", 3, "split3"),
                                              ("hmr2", 3, "split3")])
def test_engine_outputs_in_guard_bands_equal_its_own_allocation(built_lib, cuda_dev, handles, head, B, vit_gemm):
    """Engine.forward(img, taps=True, outputs=...) with every tensor of _alloc_outputs in a guarded window of its own, and
    Engine.vit_forward(out=...): bit-equal to the same call with the engine's own allocation, every canary outside the windows intact,
    every element written."""
    eng = handles.get(head, cuda_dev)
    eng.set_vit_gemm(vit_gemm)
    try:
        img = _r(B, 3, 256, 256, seed=1200 + B).to(cuda_dev)
        own = eng.forward(img, taps=True)
        outs, checks = {}, {}
        for k, t in own.items():
            outs[k], checks[k] = G.guarded_like(t.shape, t.dtype, cuda_dev)
        assert eng.forward(img, taps=True, outputs=outs) is outs
        feats, check_f = G.guarded_like((B, 192, 1280), torch.float32, cuda_dev)
        if head == "token":
            assert eng.vit_forward(img, out=feats) is feats
            outs["vit_forward"], checks["vit_forward"], own["vit_forward"] = feats, check_f, eng.vit_forward(img)
        eng.status()
    finally:
        eng.set_vit_gemm("split3")
    fails = []
    for k in outs:
        try:
            checks[k]()
        except AssertionError as e:
            fails.append(f"{k}: {e}")
        if bool(G.holds_canary(outs[k]).any()):
            fails.append(f"{k}: {int(G.holds_canary(outs[k]).sum())} element(s) were never written")
        if not torch.equal(outs[k].view(torch.int32), own[k].view(torch.int32)):
            fails.append(f"{k}: differs from the call with the engine's own allocation")
    assert not fails, "\n".join(fails)


@gpu
def test_the_new_guards_bite_on_the_device(cuda_dev):
    """tests/test_guarded_host.py on the device these tests use, for the new element types and the N-D helper: one pad element written
    through torch, inside the test's own buffer, fails check() and is named; the window full of data does not."""
    for dtype, value in ((torch.int32, 7), (torch.float64, 0.5), (torch.float32, 1.0)):
        w, check = G.guarded_like((3, 5, 7), dtype, cuda_dev)
        before = w.storage_offset() // 7
        assert w.is_contiguous() and w.data_ptr() % 64 == 0 and bool(G.holds_canary(w).all())
        check()
        w.fill_(value)
        check()
        assert not bool(G.holds_canary(w).any())
        torch.as_strided(w, (1,), (1,), w.storage_offset() + w.numel()).fill_(value)          # the element behind the window
        with pytest.raises(AssertionError, match=rf"^1 element\(s\) .* the first is row {before + 15}, column 0$"):
            check()
    s, check = G.guarded_like((), torch.float64, cuda_dev)
    s.fill_(float("nan"))                                                     # NaN data in the window is not the canary
    check()
    torch.as_strided(s, (1,), (1,), s.storage_offset() - 1).fill_(float("nan"))          # another NaN over the canary in front
    with pytest.raises(AssertionError, match=rf"the first is row {s.storage_offset() - 1}, column 0$"):          # a 0-dim window: rows of one element
        check()
    t, check = G.guarded_like((5,), torch.int32, cuda_dev, fill=torch.arange(5, dtype=torch.int32), pad=9)
    check()
    assert t.tolist() == [0, 1, 2, 3, 4] and int(torch.as_strided(t, (1,), (1,), t.storage_offset() + 5)) == 9
    torch.as_strided(t, (1,), (1,), t.storage_offset() + 5).fill_(8)
    with pytest.raises(AssertionError, match=rf"the first is row {t.storage_offset() // 5 + 1}, column 0$"):
        check()
