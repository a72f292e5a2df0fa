"""Times JPEG decoding for the evaluation datasets, host against hybrid (host entropy decode + device reconstruction), in one process
on one GPU box with the arms interleaved, and writes profiles/jpeg_decode.jsonl.

    python scripts/jpeg_bench.py [--out profiles/jpeg_decode.jsonl] [--rounds 5]

Inputs: 64 different 1920x1080 JPEG files, 4:2:0 at quality 90, written at start by Pillow from procedural images (gradients, discs and
noise; nothing is committed).  Each item has one box of 300 to 700 px, so its crop reads a window of the frame (preprocess.source_window).
Records, each [median, min, max] over `rounds` alternating rounds:
  host_decode        per frame, one thread and 16 threads: `imread(path)` (the datasets' default decoder, the whole frame) against
                     read + thmr_jpeg_probe + thmr_jpeg_entropy_decode for the item's window (what decode="device" leaves on the host)
  device_batch       thmr_jpeg_decode_batch at 64 planned items (packing, the one upload and the two kernels), device events
  end_to_end         ds.batches(32, num_workers=16) from FILES through a depth-1 model and the evaluator, decode="host" against
                     decode="device", items per second of wall clock
The comparison is always against the host path in the same run."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tokenhmr_amd import jpeg as J  # noqa: E402
from tokenhmr_amd import preprocess as PP  # noqa: E402
from tokenhmr_amd.datasets import ImageDataset, default_imread  # noqa: E402

H, W, P, NFILES = 1080, 1920, 256, 64


def picture(seed):
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([255 * x / W, 255 * y / H, 255 * (x + y) / (W + H)], axis=-1)
    for _ in range(12):
        cx, cy, r = g.uniform(0, W), g.uniform(0, H), g.uniform(40, 300)
        img[(x - cx) ** 2 + (y - cy) ** 2 < r * r] = g.uniform(0, 255, size=3)
    img += g.uniform(-24, 24, size=img.shape).astype(np.float32)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def write_files(folder):
    from PIL import Image
    paths = []
    for i in range(NFILES):
        p = os.path.join(folder, f"f{i:02d}.jpg")
        Image.fromarray(picture(1000 + i)).save(p, quality=90, subsampling=2)
        paths.append(p)
    return paths


def med(v, nd=3):
    return [round(statistics.median(v), nd), round(min(v), nd), round(max(v), nd)]


def boxes(n, seed):
    rng = np.random.default_rng(seed)
    size = rng.uniform(300, 700, size=n)
    return rng.uniform(350, W - 350, size=n), rng.uniform(350, H - 350, size=n), size


def host_decode(paths, wins, rounds):
    imread = default_imread()

    def full(k):
        return imread(paths[k])

    def hybrid(k):
        with open(paths[k], "rb") as f:
            data = f.read()
        J.probe(data)
        return J.entropy_decode(data, wins[k])

    ks = list(range(len(paths)))
    raw = {"imread_1thread_ms": [], "entropy_1thread_ms": [], "imread_16threads_fps": [], "entropy_16threads_fps": []}
    pool = ThreadPoolExecutor(16)
    for fn in (full, hybrid):
        list(pool.map(fn, ks))
    for _ in range(rounds):
        for name, fn in (("imread", full), ("entropy", hybrid)):
            t0 = time.perf_counter()
            for k in ks:
                fn(k)
            raw[f"{name}_1thread_ms"].append(1e3 * (time.perf_counter() - t0) / len(ks))
            t0 = time.perf_counter()
            for _rep in range(4):
                list(pool.map(fn, ks))
            raw[f"{name}_16threads_fps"].append(4 * len(ks) / (time.perf_counter() - t0))
    pool.shutdown()
    planned = [hybrid(k) for k in ks]
    return {"what": "jpeg_host_decode", "files": len(paths), "frame": [W, H], "format": "4:2:0 q90", "rounds": rounds,
            "file_bytes_mean": int(np.mean([os.path.getsize(p) for p in paths])),
            "columns": "[median, min, max]; *_ms per frame on one thread, *_fps frames per second with 16 threads",
            "mcu_rows_decoded_mean": float(np.mean([p.plan.mcu_rows_decoded for p in planned])), "mcu_rows_of_frame": -(-H // 16),
            **{n: med(v) for n, v in raw.items()}}, planned


def device_batch(planned, rounds, dev):
    dec = J.JpegDecoder(dev)
    outs = [torch.empty(p.window[3], p.window[2], 3, dtype=torch.uint8, device=dev) for p in planned]
    for _ in range(3):
        dec.decode_planned(planned, out=outs)
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _c in range(10):
            dec.decode_planned(planned, out=outs)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / 10)
    rec = {"what": "jpeg_device_batch", "items": len(planned), "rounds": rounds, "calls_per_window": 10,
           "columns": "[median, min, max] milliseconds per thmr_jpeg_decode_batch call (packing + upload + 2 kernels)",
           "coef_bytes_uploaded": int(sum(p.nbytes for p in planned)), "window_bytes_written": int(sum(p.window[2] * p.window[3] * 3 for p in planned)),
           "frame_bytes_if_whole": len(planned) * H * W * 3, "decode_batch_ms": med(ms, 4)}
    dec.close()
    return rec


def end_to_end(folder, rounds, dev, N=256, B=32):
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as Wt
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.model import TokenHMR, ConfigNode
    from tokenhmr_amd.evaluator import Evaluator
    from tokenhmr_amd.eval_dp import run_eval
    cfg = HMRConfig(vit_depth=1, dec_depth=1)
    model = TokenHMR.from_state(cfg, Wt.make_synthetic_state(cfg, 0), Wt.make_synthetic_tokenizer(cfg, 0), make_synthetic_smpl(cfg, 0),
                                max_batch=B, device=dev)
    rng = np.random.default_rng(9)
    cx, cy, size = boxes(N, 2)
    path = os.path.join(folder, "synthetic.npz")
    np.savez(path, imgname=np.array([f"f{i % NFILES:02d}.jpg" for i in range(N)]), center=np.stack([cx, cy], 1), scale=size,
             body_pose=0.3 * rng.normal(size=(N, 72)), has_body_pose=np.ones(N), betas=0.5 * rng.normal(size=(N, 10)), has_betas=np.ones(N),
             body_keypoints_3d=rng.normal(size=(N, 25, 4)), extra_keypoints_3d=rng.normal(size=(N, 19, 4)),
             gender=np.array(["m", "f"] * (N // 2)))
    mcfg = ConfigNode({"MODEL": {"IMAGE_SIZE": P, "IMAGE_MEAN": list(PP.DEFAULT_MEAN), "IMAGE_STD": list(PP.DEFAULT_STD), "BBOX_SHAPE": [192, 256]},
                       "SMPL": {"NUM_BODY_JOINTS": 23}})
    sm, sf = make_synthetic_smpl(HMRConfig(), 1), make_synthetic_smpl(HMRConfig(), 2)
    ds = {mode: ImageDataset(mcfg, path, folder, device=dev, smpl_male=sm, smpl_female=sf, decode=mode) for mode in ("host", "device")}
    a, b = ds["host"].batch(range(B)), ds["device"].batch(range(B))
    torch.cuda.synchronize()
    assert torch.equal(a["img"], b["img"]), "decode='device' must give the crops of decode='host' bit for bit"
    kp = [25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 43]

    def e2e(mode):
        ev = Evaluator(N, kp, 39, metrics=["mode_re", "mode_mpjpe", "mode_pve"], dataset="3DPW-TEST")
        run_eval(model, ds[mode], ev, batch_size=B, device=dev, num_workers=16)

    raw = {"host": [], "device": []}
    for mode in raw:
        e2e(mode)
    for _ in range(rounds):
        for mode in raw:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e2e(mode)
            torch.cuda.synchronize()
            raw[mode].append(N / (time.perf_counter() - t0))
    st = ds["device"].decode_stats
    return {"what": "jpeg_end_to_end", "items": N, "files": NFILES, "batch_size": B, "num_workers": 16, "frame": [W, H],
            "model": "vit_depth=1, dec_depth=1", "rounds": rounds,
            "columns": "[median, min, max] items per second from files (wall clock, synchronised at both ends)",
            "crops_bit_equal": True, "device_fallbacks": st["fallback"], "coef_bytes_per_item": st["coef_bytes"] // max(st["device"], 1),
            "decode_host": med(raw["host"], 1), "decode_device": med(raw["device"], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_bench.py needs a GPU: the arms are only comparable on one box in one session")
    dev = torch.device("cuda:0")
    folder = tempfile.mkdtemp()
    paths = write_files(folder)
    cx, cy, size = boxes(NFILES, 1)
    wins = []
    for i in range(NFILES):
        w = PP.source_window(PP.gen_trans_from_patch_cv(cx[i], cy[i], size[i], size[i], P, P, 1.0, 0), P, H, W)
        wins.append((0, 0, 0, 0) if w is None else w)
    recs = []
    rec, planned = host_decode(paths, wins, args.rounds)
    recs.append(rec)
    print(json.dumps(rec), flush=True)
    recs.append(device_batch(planned, args.rounds, dev))
    print(json.dumps(recs[-1]), flush=True)
    recs.append(end_to_end(folder, args.rounds, dev))
    print(json.dumps(recs[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
