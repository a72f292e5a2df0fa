"""Times the crops of an evaluation batch — B items from B different 1920x1080 frames, one crop each, boxes of 300 to 700 px — three ways,
in one process on one GPU, and the device datasets end to end.

    python scripts/eval_dataset_bench.py [--out profiles/eval_dataset.jsonl] [--rounds 7]

Arms (scripts/val_loss_bench.py's method: the arms alternate `rounds` times, a window is `calls` back-to-back calls between two device
events; median [min, max] over the rounds):
  a  B x (Cropper.to_device + thmr_cropper_run with one descriptor): what the library could do before thmr_cropper_run_frames
  b  Cropper.warp_frames(windows=False): one call, whole frames packed into one pinned buffer, one upload
  c  Cropper.warp_frames(windows=True): one call, only the window each crop can touch is packed and uploaded
each "with_h2d" (packing and upload inside the window: what a caller gets) and "kernels" (frames / windows already resident: the
descriptor copy and the launches alone).  The bytes uploaded per batch are recorded.

A second line records ds.batches(32) end to end — in-memory frames (no JPEG decode), a depth-1 model and the evaluator — in items/s
beside the forward-only rate of the same model in the same process.  NOT measured: a real JPEG decode rate, real 3DPW / EMDB assets."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tokenhmr_amd import _cabi  # noqa: E402
from tokenhmr_amd import preprocess as PP  # noqa: E402

H, W, P = 1080, 1920, 256


def make_frames(n, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    return [np.ascontiguousarray(np.roll(base, 37 * i, axis=1)) for i in range(n)]


def make_boxes(n, seed=1):
    rng = np.random.default_rng(seed)
    size = rng.uniform(300, 700, size=n)
    return rng.uniform(350, W - 350, size=n), rng.uniform(350, H - 350, size=n), size


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def med(v):
    return [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]


def resident_call(cropper, frames, T, windows, dev):
    """The frame-table call on data that is already on the device: -> (callable, bytes resident)."""
    n = len(frames)
    wins = [PP.source_window(T[i], P, H, W) if windows else (0, 0, W, H) for i in range(n)]
    offs, total = [], 0
    for x0, y0, w, h in wins:
        offs.append(total)
        total = (total + w * h * 3 + 255) & ~255
    buf = torch.empty(total, dtype=torch.uint8, device=dev)
    items = (_cabi.FrameCrop * n)()
    for i, (x0, y0, w, h) in enumerate(wins):
        buf[offs[i]:offs[i] + w * h * 3] = torch.from_numpy(np.ascontiguousarray(frames[i][y0:y0 + h, x0:x0 + w]).reshape(-1)).to(dev)
        it = items[i]
        it.win_dev, it.row_stride, it.H, it.W = buf.data_ptr() + offs[i], w * 3, H, W
        it.win_x0, it.win_y0, it.win_w, it.win_h = x0, y0, w, h
        it.M[:] = T[i].reshape(6).tolist()
        it.sigma, it.truncate = 0.0, 3.0
    m = (C.c_float * 3)(*[np.float32(255.0 * v) for v in PP.DEFAULT_MEAN])
    s = (C.c_float * 3)(*[np.float32(255.0 * v) for v in PP.DEFAULT_STD])
    out = torch.empty(n, 3, P, P, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call():
        rc = cropper.lib.thmr_cropper_run_frames(cropper.h, items, n, P, 1, m, s, C.c_void_p(out.data_ptr()), stream)
        assert rc == 0
        return out

    call.keep = buf
    return call, total


def crop_arms(B, rounds, dev):
    cropper = PP.Cropper(dev)
    frames = make_frames(B)
    cx, cy, size = make_boxes(B)
    T = np.stack([PP.gen_trans_from_patch_cv(cx[i], cy[i], size[i], size[i], P, P, 1.0, 0) for i in range(B)])
    frames_dev = [cropper.to_device(f) for f in frames]
    outs = torch.empty(B, 3, P, P, device=dev)

    def a(src):
        for i in range(B):
            cropper.warp(src[i], T[i:i + 1], None, truncate=3.0, patch=P, out=outs[i:i + 1])
        return outs

    kb, bytes_b = resident_call(cropper, frames, T, False, dev)
    kc, bytes_c = resident_call(cropper, frames, T, True, dev)
    arms = {"a_with_h2d": lambda: a(frames), "b_with_h2d": lambda: cropper.warp_frames(frames, T, None, patch=P, windows=False),
            "c_with_h2d": lambda: cropper.warp_frames(frames, T, None, patch=P, windows=True),
            "a_kernels": lambda: a(frames_dev), "b_kernels": kb, "c_kernels": kc}
    ref = arms["a_with_h2d"]().clone()
    for n, f in arms.items():
        assert torch.equal(f(), ref), n
    staged = {}
    for n in ("b_with_h2d", "c_with_h2d"):
        arms[n]()
        staged[n] = cropper.last_staged_bytes
    for f in arms.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    raw = {n: [] for n in arms}
    for _ in range(rounds):
        for n, f in arms.items():
            raw[n].append(window_ms(f, 4 if n.endswith("h2d") else 20))
    rec = {"what": "eval_batch_crops", "B": B, "frame": [W, H], "patch": P, "boxes_px": [300, 700], "rounds": rounds,
           "calls_per_window": {"with_h2d": 4, "kernels": 20}, "columns": "[median, min, max] milliseconds per batch",
           "bytes_uploaded_per_batch": {"a": B * H * W * 3, "b": staged["b_with_h2d"], "c": staged["c_with_h2d"]},
           "bytes_resident_kernels_arms": {"b": bytes_b, "c": bytes_c},
           **{n: med(v) for n, v in raw.items()}}
    cropper.close()
    return rec


def end_to_end(rounds, dev, N=256, B=32):
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as Wt
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.model import TokenHMR, ConfigNode
    from tokenhmr_amd.evaluator import Evaluator
    from tokenhmr_amd.datasets import ImageDataset
    from tokenhmr_amd.eval_dp import run_eval
    cfg = HMRConfig(vit_depth=1, dec_depth=1)
    model = TokenHMR.from_state(cfg, Wt.make_synthetic_state(cfg, 0), Wt.make_synthetic_tokenizer(cfg, 0), make_synthetic_smpl(cfg, 0),
                                max_batch=B, device=dev)
    frames = {f"f{i:02d}.jpg": f for i, f in enumerate(make_frames(16, seed=5))}
    rng = np.random.default_rng(9)
    cx, cy, size = make_boxes(N, seed=2)
    path = os.path.join(tempfile.mkdtemp(), "synthetic.npz")
    np.savez(path, imgname=np.array([f"f{i % 16:02d}.jpg" for i in range(N)]), center=np.stack([cx, cy], 1), scale=size,
             body_pose=0.3 * rng.normal(size=(N, 72)), has_body_pose=np.ones(N), betas=0.5 * rng.normal(size=(N, 10)), has_betas=np.ones(N),
             body_keypoints_3d=rng.normal(size=(N, 25, 4)), extra_keypoints_3d=rng.normal(size=(N, 19, 4)),
             gender=np.array(["m", "f"] * (N // 2)))
    mcfg = ConfigNode({"MODEL": {"IMAGE_SIZE": P, "IMAGE_MEAN": list(PP.DEFAULT_MEAN), "IMAGE_STD": list(PP.DEFAULT_STD), "BBOX_SHAPE": [192, 256]},
                       "SMPL": {"NUM_BODY_JOINTS": 23}})
    ds = ImageDataset(mcfg, path, "", device=dev, imread=lambda p: frames[os.path.basename(p)],
                      smpl_male=make_synthetic_smpl(HMRConfig(), 1), smpl_female=make_synthetic_smpl(HMRConfig(), 2))
    kp = [25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 43]
    batch = ds.batch(range(B))

    def e2e():
        ev = Evaluator(N, kp, 39, metrics=["mode_re", "mode_mpjpe", "mode_pve"], dataset="3DPW-TEST")
        run_eval(model, ds, ev, batch_size=B, device=dev, num_workers=4)

    def fwd():
        with torch.no_grad():
            for _ in range(N // B):
                model(batch)
        torch.cuda.synchronize()

    raw = {"end_to_end": [], "forward_only": []}
    for f in (e2e, fwd):
        f()
    for _ in range(rounds):
        for n, f in (("end_to_end", e2e), ("forward_only", fwd)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            raw[n].append(N / (time.perf_counter() - t0))
    return {"what": "eval_datasets_end_to_end", "items": N, "batch_size": B, "num_workers": 4, "frame": [W, H], "model": "vit_depth=1, dec_depth=1",
            "rounds": rounds, "columns": "[median, min, max] items per second (wall clock, synchronised at both ends)",
            "frames": "in memory: no JPEG decode is measured", **{n: med(v) for n, v in raw.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_dataset.jsonl"))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_dataset_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    recs = []
    for B in (8, 32, 64):
        recs.append(crop_arms(B, args.rounds, dev))
        print(json.dumps(recs[-1]), flush=True)
    recs.append(end_to_end(args.rounds, dev))
    print(json.dumps(recs[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for rec in recs:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
