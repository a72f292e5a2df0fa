"""The crop kernels (tokenhmr_amd/csrc/crop.hip: rows pass, columns pass, warp, and their frame-table twins) against the oracle at the
affines and blur radii the workload never sends: rotations, flips, shear, 8x scales, sub-texel translations on the fixed-point grid
and on its rounding ties, one tap pair in frame, wholly off-frame and saturated coordinates; blur radius 0, radius wider than the frame,
1-texel-wide frames; every entry (thmr_cropper_run contiguous and with padded rows, thmr_cropper_run_frames on whole frames, on tight
windows and on padded device windows) bit-equal to the others.

Reference: oracle/crop_oracle.py, `warp_affine(gaussian_antialias(frame, sigma, truncate), M, (P, P))` then `finish_patch(numpy1=True)`,
as `vitdet_item` assembles it (an un-blurred crop warps the uint8 frame).

Tolerances, derived and not measured:
  * un-blurred and radius-0 crops: bit-equal.  Integer bilinear (or, radius 0, the identity blur and the same contraction-free fp64
    four-term sum), one rounding to float32, one IEEE float32 subtract and divide.
  * radius >= 1 under the identity normalisation (mean 0, std 1/255: the output IS the float32 rounding of the fp64 result):
    |got - want| <= np.spacing(float32(want)).  The gaussian weights come from the C library's exp there and numpy's here, so the fp64
    sums may differ in their last bits; that moves a float32 rounding by one step at the most, never by two.  No cap on how many.
  * radius >= 1 under the real mean / std: additionally max abs < 2e-6, the bound of test_crop.test_gpu_large_frame_blurred_crops.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from oracle import crop_oracle as CO

IDENT = dict(mean=(0.0, 0.0, 0.0), std=(1 / 255.0,) * 3)
REAL = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
NORMS = {"ident": IDENT, "real": REAL}

# name: H, W, patch, sigmas.  9.0 is a radius of 27 (truncate 3) or 36 (truncate 4): wider than both sides of the 20x31 frame
CONFIGS = {
    "37x53_p24": (37, 53, 24, (0.0, 0.1, 0.6, 2.0)),
    "20x31_p17": (20, 31, 17, (0.0, 0.1, 0.6, 2.0, 9.0)),
    "37x53_p1": (37, 53, 1, (0.0, 0.1, 0.6, 2.0)),
    "1x1_p8": (1, 1, 8, (0.0, 0.1, 2.0)),
    "1x40_p8": (1, 40, 8, (0.0, 0.1, 2.0)),
    "40x1_p8": (40, 1, 8, (0.0, 0.1, 2.0)),
}
TRUNCATES = (3.0, 4.0)
ALL = [(c, t) for c in CONFIGS for t in TRUNCATES]


def radius(sigma, truncate):
    """scipy's kernel radius, or -1 for a crop that is not blurred at all (gaussian_filter skips sigma <= 1e-15)."""
    return int(truncate * sigma + 0.5) if sigma > 1e-15 else -1


def affines(H, W, P):
    """(name, forward 2x3) of every family, for one frame size and patch."""
    g = CO.gen_trans_from_patch_cv
    cx, cy = W / 2.0, H / 2.0
    out = [(f"quarter{rot}", g(cx, cy, 30, 30, P, P, 1.0, rot)) for rot in (90, 180, -90)]
    for rot in (33, -147.5):
        for tag, (x, y) in (("in", (cx, cy)), ("c00", (0.0, 0.0)), ("cWH", (float(W), float(H)))):
            out.append((f"rot{rot}_{tag}", g(x, y, 30, 30, P, P, 1.0, rot)))
    out += [("flip_h", [[-1, 0, 40], [0, 1, -3]]), ("flip_v", [[1, 0, -3], [0, -1, 30]]), ("flip_hv", [[-1, 0, 40], [0, -1, 30]]),
            ("shear", [[0.7, 0.4, -3], [-0.2, 1.3, 2]])]
    for tag, s in (("minify8", 0.125), ("magnify8", 8.0)):          # the patch centre on the frame centre
        out.append((tag, [[s, 0, P / 2.0 - s * cx], [0, s, P / 2.0 - s * cy]]))
    # sub-texel translations: 1/32 is one step of the 5-bit fraction, +-1/64 its rounding tie, 31/32 the last step
    ts = (0.5, 1 / 32, 1 / 64, -1 / 64, 31 / 32)
    for k, t in enumerate(ts):
        out.append((f"subtexel{k}", [[1, 0, t], [0, 1, ts[(k + 2) % 5]]]))
    # one tap pair in frame: source x = x + b.  b = -0.5 puts sx = -1 for output column 0, b = W - 1.5 puts sx = W - 1 for column 1
    for tag, bx, by in (("lo_lo", -0.5, -0.5), ("hi_hi", W - 1.5, H - 1.5), ("lo_hi", -0.5, H - 1.5)):
        out.append((f"border_{tag}", [[1, 0, -bx], [0, 1, -by]]))
    # wholly off-frame by one texel: sx + 1 = -1 at the last column / sx = W at the first, and the same for rows
    out += [("off1_left", [[1, 0, P + 1], [0, 1, 0]]), ("off1_right", [[1, 0, -W], [0, 1, 0]]),
            ("off1_up", [[1, 0, 0], [0, 1, P + 1]]), ("off1_down", [[1, 0, 0], [0, 1, -H]])]
    # far away: the short texel coordinates saturate
    out += [(f"far{k}", [[1, 0, tx], [0, 1, ty]]) for k, (tx, ty) in enumerate(((1e6, 0), (-1e6, 0), (0, 1e6), (1e6, -1e6)))]
    return [(n, np.asarray(M, dtype=np.float64).reshape(2, 3)) for n, M in out]


_ORACLE, _DEVICE = {}, {}


def oracle(cfg, truncate):
    """Frame, crops (every affine at every sigma) and the oracle's patches before normalisation: built once per (cfg, truncate)."""
    key = (cfg, truncate)
    if key not in _ORACLE:
        H, W, P, sigmas = CONFIGS[cfg]
        frame = np.random.default_rng(1000 + 7 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
        names, Ms, sigs = [], [], []
        for n, M in affines(H, W, P):
            for s in sigmas:
                names.append(n); Ms.append(M); sigs.append(s)
        blurred = {s: CO.gaussian_antialias(frame, s, truncate) for s in sigmas if s > 0}
        patches = [CO.warp_affine(frame if s == 0 else blurred[s], M, (P, P)) for M, s in zip(Ms, sigs)]
        w = types.SimpleNamespace(cfg=cfg, truncate=truncate, H=H, W=W, P=P, frame=frame, names=names, M=np.stack(Ms), sig=np.array(sigs),
                                  rad=[radius(s, truncate) for s in sigs], patches=patches, _want={})

        def want(norm, is_bgr=True):
            if (norm, is_bgr) not in w._want:
                mean, std = 255.0 * np.array(NORMS[norm]["mean"]), 255.0 * np.array(NORMS[norm]["std"])
                w._want[norm, is_bgr] = np.stack([CO.finish_patch(p, mean, std, is_bgr, numpy1=True) for p in patches])
            return w._want[norm, is_bgr]

        w.want = want
        _ORACLE[key] = w
    return _ORACLE[key]


def device(dev, cfg, truncate):
    """Cropper.warp on ALL crops of the frame in one call (sigmas mixed: per-crop weight offsets, shared launch grids), under both
    normalisations: the result every other entry is compared with."""
    key = (cfg, truncate)
    if key not in _DEVICE:
        from tokenhmr_amd.preprocess import Cropper
        w = oracle(cfg, truncate)
        cr = Cropper(dev)
        _DEVICE[key] = {k: cr.warp(w.frame, w.M, w.sig, truncate=truncate, patch=w.P, **n).cpu() for k, n in NORMS.items()}
        cr.close()
    return _DEVICE[key]


def border_value(norm):
    """(0 - mean) / std in float32, per output channel."""
    mean, std = NORMS[norm]["mean"], NORMS[norm]["std"]
    return np.array([(np.float32(0) - np.float32(255.0 * m)) / np.float32(255.0 * s) for m, s in zip(mean, std)], dtype=np.float32)


def test_the_cases_hit_the_edges_they_name():
    """No GPU: the oracle's own source coordinates show that every family does what its name says, so the GPU tests cannot pass on
    cases that quietly stayed in the comfortable middle."""
    H, W, P, _ = CONFIGS["37x53_p24"]
    A = dict(affines(H, W, P))
    Mi = {n: CO.invert_affine(M) for n, M in A.items()}
    for n in ("quarter90", "quarter-90"):          # the cross terms carry the whole map
        assert abs(Mi[n][1]) > 1 and abs(Mi[n][3]) > 1 and abs(Mi[n][0]) < 1e-6 and abs(Mi[n][4]) < 1e-6, (n, Mi[n])
    assert Mi["quarter180"][0] < -1 and Mi["quarter180"][4] < -1
    assert all(min(abs(Mi[n][k]) for k in (0, 1, 3, 4)) > 0.1 for n in A if n.startswith("rot") or n == "shear")
    assert Mi["flip_h"][0] == -1 and Mi["flip_v"][4] == -1 and Mi["flip_hv"][0] == Mi["flip_hv"][4] == -1
    assert Mi["minify8"][0] == 8 and Mi["magnify8"][0] == 0.125
    for cfg, (H, W, P, _) in CONFIGS.items():
        A = dict(affines(H, W, P))
        sc = {n: CO.source_coords(M, (P, P)) for n, M in A.items()}
        # one tap pair in frame, for a whole column / row of outputs
        sx, sy, fx, fy = sc["border_lo_lo"]
        assert (sx[:, 0] == -1).all() and (sy[0, :] == -1).all() and (fx[:, 0] == 16).all()
        sx, sy, _, _ = sc["border_hi_hi"]
        if P > 1:
            assert (sx[:, 1] == W - 1).all() and (sy[1, :] == H - 1).all()
        # one texel off: the nearest tap is exactly one texel outside
        assert sc["off1_left"][0].max() + 1 == -1 and sc["off1_right"][0].min() == W
        assert sc["off1_up"][1].max() + 1 == -1 and sc["off1_down"][1].min() == H
        # far away: the coordinate saturates at the ends of short
        assert (sc["far0"][0] == -32768).all() and (sc["far1"][0] == 32767).all() and (sc["far2"][1] == -32768).all()
        # the fixed-point grid and its ties: 1/64 is half a step and rounds up, -1/64 rounds to the step below zero
        assert sc["subtexel1"][2][0, 0] == 31 and sc["subtexel0"][2][0, 0] == 16
        assert set(np.unique(sc["subtexel2"][2])) <= {0, 31} and set(np.unique(sc["subtexel3"][2])) <= {0, 1}
        for t in TRUNCATES:
            w = oracle(cfg, t)
            for i, n in enumerate(w.names):
                if n.startswith(("off1", "far")):
                    assert not np.any(w.patches[i]), (cfg, n)
    # radius 0 is the float path, not the integer one: the oracle's own results differ on every rotated crop of the larger frames
    for cfg in ("37x53_p24", "20x31_p17"):
        w = oracle(cfg, 3.0)
        want = w.want("ident")
        for i, n in enumerate(w.names):
            if w.rad[i] == 0 and (n.startswith("rot") and n.endswith("_in") or n == "shear"):
                i0 = [j for j, m in enumerate(w.names) if m == n and w.rad[j] == -1][0]
                assert not np.array_equal(want[i], want[i0]), (cfg, n)
    w = oracle("20x31_p17", 3.0)
    assert max(w.rad) == 27 and max(oracle("20x31_p17", 4.0).rad) == 36 and 0 in w.rad and -1 in w.rad


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,truncate", ALL)
def test_gpu_warp_equals_the_oracle(built_lib, cuda_dev, cfg, truncate):
    """Cropper.warp, all crops of the frame in one call.  Prints the worst difference in float32 steps and the share of elements that
    differ, over the crops of radius >= 1."""
    w = oracle(cfg, truncate)
    got = {k: v.numpy() for k, v in device(cuda_dev, cfg, truncate).items()}
    want = {k: w.want(k) for k in NORMS}
    assert got["ident"].shape == want["ident"].shape == (len(w.names), 3, w.P, w.P)
    worst, differ, total = 0.0, 0, 0
    for i, (n, r) in enumerate(zip(w.names, w.rad)):
        who = (cfg, truncate, n, float(w.sig[i]), r)
        if r <= 0:
            assert np.array_equal(got["ident"][i], want["ident"][i]) and np.array_equal(got["real"][i], want["real"][i]), who
        else:
            d = np.abs(got["ident"][i].astype(np.float64) - want["ident"][i].astype(np.float64))
            step = np.abs(np.spacing(want["ident"][i])).astype(np.float64)
            worst, differ, total = max(worst, float((d / step).max())), differ + int((d > 0).sum()), total + d.size
            assert (d <= step).all(), who + (float((d / step).max()),)
            assert np.abs(got["real"][i] - want["real"][i]).max() < 2e-6, who
        if n.startswith(("off1", "far")):          # every pixel is the border value
            for k in NORMS:
                assert np.array_equal(got[k][i], np.broadcast_to(border_value(k)[:, None, None], (3, w.P, w.P))), who + (k,)
    print(f"\n[crop edges] {cfg} truncate {truncate}: {len(w.names)} crops, radius >= 1: worst {worst:.3f} float32 steps, "
          f"{differ} of {total} elements differ ({100.0 * differ / max(total, 1):.4f} %)")
    # radius 0 took the float path: wherever the oracle's radius-0 result differs from its un-blurred one, so does the kernel's
    n_float = 0
    for i, (n, r) in enumerate(zip(w.names, w.rad)):
        if r == 0:
            i0 = [j for j, m in enumerate(w.names) if m == n and w.rad[j] == -1][0]
            if not np.array_equal(want["ident"][i], want["ident"][i0]):
                n_float += 1
                assert not np.array_equal(got["ident"][i], got["ident"][i0]), (cfg, n)
    assert n_float > 0


def _padded_rows(a, pad=13):
    """(h, w, 3) uint8 -> (h, w * 3 + pad) with the padding filled with 255."""
    h, w = a.shape[:2]
    out = np.full((h, w * 3 + pad), 255, dtype=np.uint8)
    out[:, :w * 3] = a.reshape(h, w * 3)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,truncate", ALL)
def test_gpu_frame_table_entries_are_bit_equal_to_warp(built_lib, cuda_dev, cfg, truncate):
    """thmr_cropper_run_frames on whole frames, on tight windows, and on tight device windows whose rows are padded by 13 bytes of 255:
    each item bit-equal to the one-frame entry, rotated, flipped and blurred items included."""
    from tokenhmr_amd.preprocess import Cropper, source_window
    w = oracle(cfg, truncate)
    ref = device(cuda_dev, cfg, truncate)["real"]
    n = len(w.names)
    cr = Cropper(cuda_dev)
    for windows in (False, True):
        got = cr.warp_frames([w.frame] * n, w.M, w.sig, truncate=truncate, patch=w.P, windows=windows).cpu()
        bad = [w.names[i] for i in range(n) if not torch.equal(got[i], ref[i])]
        assert not bad, (cfg, truncate, windows, bad)
    wins = [source_window(w.M[i], w.P, w.H, w.W, w.sig[i], truncate) for i in range(n)]
    assert any(x is None for x in wins) and any(x is not None for x in wins)
    parts, offs, total = [], [], 0
    for x in wins:
        offs.append(total)
        if x is not None:
            x0, y0, ww, wh = x
            parts.append(_padded_rows(w.frame[y0:y0 + wh, x0:x0 + ww]).reshape(-1))
            total += parts[-1].size
    buf = torch.as_tensor(np.concatenate(parts)).to(cuda_dev)
    tens = [None if x is None else buf[o:o + x[3] * (x[2] * 3 + 13)] for x, o in zip(wins, offs)]
    strides = [0 if x is None else x[2] * 3 + 13 for x in wins]
    got = cr.warp_device_windows(tens, [(w.H, w.W)] * n, wins, w.M, w.sig, truncate=truncate, patch=w.P, row_strides=strides).cpu()
    cr.close()
    bad = [w.names[i] for i in range(n) if not torch.equal(got[i], ref[i])]
    assert not bad, (cfg, truncate, "device windows", bad)


def _raw_run(cr, frame_dev, H, W, stride, M, sig, truncate, P, norm, is_bgr, out):
    """thmr_cropper_run itself: the wrapper always passes row_stride = W * 3."""
    from tokenhmr_amd import _cabi
    from tokenhmr_amd.preprocess import _scaled
    n = len(sig)
    descs = (_cabi.CropDesc * n)()
    for i in range(n):
        descs[i].M[:] = np.asarray(M[i], dtype=np.float64).reshape(6).tolist()
        descs[i].sigma, descs[i].truncate = float(sig[i]), float(truncate)
    with torch.cuda.device(cr.device):
        return cr.lib.thmr_cropper_run(cr.h, C.c_void_p(frame_dev.data_ptr()), H, W, stride, descs, n, P, int(is_bgr), _scaled(norm["mean"]),
                                       _scaled(norm["std"]), C.c_void_p(out.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream(cr.device).cuda_stream))


@pytest.mark.gpu
def test_gpu_run_with_padded_rows_is_bit_equal_to_contiguous(built_lib, cuda_dev):
    """The frame held in a wider tensor, row_stride = W * 3 + 13, the padding 255: were a row addressed by W * 3 anywhere, or a
    padding byte read as a texel, the result would change."""
    from tokenhmr_amd.preprocess import Cropper
    cr = Cropper(cuda_dev)
    for cfg in CONFIGS:
        w = oracle(cfg, 3.0)
        ref = device(cuda_dev, cfg, 3.0)["real"]
        wide = torch.as_tensor(_padded_rows(w.frame)).to(cuda_dev)
        out = torch.full(ref.shape, float("nan"), device=cuda_dev)
        rc = _raw_run(cr, wide, w.H, w.W, w.W * 3 + 13, w.M, w.sig, 3.0, w.P, REAL, True, out)
        assert rc == 0, cr.lib.thmr_cropper_last_error(cr.h)
        out = out.cpu()
        bad = [w.names[i] for i in range(len(w.names)) if not torch.equal(out[i], ref[i])]
        assert not bad, (cfg, bad)
    cr.close()


@pytest.mark.gpu
def test_gpu_channel_order_on_rotated_and_blurred_crops(built_lib, cuda_dev):
    """is_bgr in both values: channel-reversed copies of each other, and each equal to the oracle's."""
    from tokenhmr_amd.preprocess import Cropper
    w = oracle("37x53_p24", 3.0)
    pick = [i for i, (n, r) in enumerate(zip(w.names, w.rad)) if (n == "rot33_in" and r == -1) or (n == "quarter90" and r == 6)]
    assert len(pick) == 2
    cr = Cropper(cuda_dev)
    a, b = (cr.warp(w.frame, w.M[pick], w.sig[pick], truncate=3.0, patch=w.P, is_bgr=flag, **IDENT).cpu().numpy() for flag in (False, True))
    cr.close()
    assert np.array_equal(b, a[:, ::-1]) and not np.array_equal(a, b)
    assert np.array_equal(b, device(cuda_dev, "37x53_p24", 3.0)["ident"].numpy()[pick])
    assert np.array_equal(a[0], w.want("ident", False)[pick[0]])                        # un-blurred: bit-equal
    assert (np.abs(a[1] - w.want("ident", False)[pick[1]]) <= np.abs(np.spacing(w.want("ident", False)[pick[1]]))).all()


@pytest.mark.gpu
def test_gpu_run_refuses_without_launching(built_lib, cuda_dev):
    """A frame side above 32767 and a blur radius beyond int are refused by the one-frame entry too, before any kernel: the output
    keeps its sentinel.  The 2 x 32768 frame is real, so the read would have been in bounds even were it not refused."""
    from tokenhmr_amd import _cabi
    from tokenhmr_amd.preprocess import Cropper
    cr = Cropper(cuda_dev)
    I = np.array([[[1.0, 0, 0], [0, 1.0, 0]]])
    out = torch.full((1, 3, 8, 8), -7.0, device=cuda_dev)
    wide = torch.zeros(2, 32768, 3, dtype=torch.uint8, device=cuda_dev)
    with pytest.raises(_cabi.EngineError, match="bad frame geometry"):
        cr.warp(wide, I, patch=8, out=out)
    with pytest.raises(_cabi.EngineError, match="bad frame geometry"):
        cr.warp(wide.reshape(32768, 2, 3), I, patch=8, out=out)
    small = torch.zeros(48, 64, 3, dtype=torch.uint8, device=cuda_dev)
    for sigma, truncate in [(1e9, 3.0), (1e10, 3.0), (1e300, 3.0), (1.0, 1e300), (1366.0, 3.0)]:
        with pytest.raises(_cabi.EngineError, match="blur radius too large"):
            cr.warp(small, I, sigmas=[sigma], truncate=truncate, patch=8, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    cr.close()
