"""Times PNG decoding for the evaluation datasets, host against hybrid (host inflate + device un-filter and conversion), in one process
on one GPU box with the arms interleaved, and writes profiles/png_decode.jsonl.

    python scripts/png_dec_bench.py [--out profiles/png_decode.jsonl] [--rounds 5]

Inputs: 64 different 1920x1080 RGB PNG files written at start by Pillow at its default level from the procedural images of
scripts/jpeg_bench.py (gradients, discs and noise; nothing is committed).  Each item has one box of 300 to 700 px, so its crop reads a
window of the frame (preprocess.source_window).  Records, each [median, min, max] over `rounds` alternating rounds:
  png_files          the files' mean size, the share of each filter type, the mean strips per frame and kept-rows share
  host_decode        per frame, one thread and 16 threads: `imread(path)` (the datasets' default decoder, the whole frame) against
                     read + thmr_png_probe + thmr_png_inflate_window for the item's window (what decode="device+png" leaves on the host)
  inflate            the library's own inflate against zlib.decompress on the same streams, whole, one thread
  device_batch       thmr_png_decode_batch at 64 planned items and at 1 (packing, the one upload and the two kernels), device events
  end_to_end         ds.batches(32, num_workers=16) from FILES through a depth-1 model and the evaluator, decode="host" against
                     decode="device+png", items per second of wall clock
The comparison is always against the host path in the same run."""
import argparse
import json
import os
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import jpeg_bench as JB  # noqa: E402
from tokenhmr_amd import png as PNG  # noqa: E402
from tokenhmr_amd import preprocess as PP  # noqa: E402
from tokenhmr_amd.datasets import ImageDataset, default_imread  # noqa: E402

H, W, P, NFILES = JB.H, JB.W, JB.P, JB.NFILES
med = JB.med


def write_files(folder):
    from PIL import Image
    paths = []
    for i in range(NFILES):
        p = os.path.join(folder, f"f{i:02d}.png")
        Image.fromarray(JB.picture(1000 + i)).save(p)
        paths.append(p)
    return paths


def zlib_stream(data):
    """The IDAT chunks' data joined."""
    at, out = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        if kind == b"IDAT":
            out.append(data[at + 8:at + 8 + n])
        at += 12 + n
    return b"".join(out)


def describe(paths, wins):
    filters = np.zeros(5, np.int64)
    strips, kept, uploaded = [], [], []
    for p, win in zip(paths, wins):
        with open(p, "rb") as f:
            data = f.read()
        whole = PNG.inflate_window(data)
        f = whole.rows[:, 0]
        filters += np.bincount(f, minlength=5)
        item = PNG.inflate_window(data, win)
        fk = item.rows[:, 0]
        strips.append(int(1 + np.count_nonzero(fk[1:] <= 1)) if len(fk) else 0)
        kept.append(item.plan.rows_kept / H)
        uploaded.append(item.nbytes)
    return {"what": "png_files", "files": len(paths), "frame": [W, H], "format": "RGB 8-bit, Pillow default level",
            "file_bytes_mean": int(np.mean([os.path.getsize(p) for p in paths])),
            "filter_share_none_sub_up_avg_paeth": [round(float(v), 4) for v in filters / filters.sum()],
            "strips_per_window_mean": float(np.mean(strips)), "kept_rows_share_mean": round(float(np.mean(kept)), 4),
            "window_rows_share_mean": round(float(np.mean([w[3] / H for w in wins])), 4), "kept_bytes_per_item_mean": int(np.mean(uploaded))}


def host_decode(paths, wins, rounds):
    imread = default_imread()

    def full(k):
        return imread(paths[k])

    def hybrid(k):
        with open(paths[k], "rb") as f:
            data = f.read()
        PNG.probe(data)
        return PNG.inflate_window(data, wins[k])

    ks = list(range(len(paths)))
    raw = {"imread_1thread_ms": [], "inflate_window_1thread_ms": [], "imread_16threads_fps": [], "inflate_window_16threads_fps": []}
    pool = ThreadPoolExecutor(16)
    for fn in (full, hybrid):
        list(pool.map(fn, ks))
    for _ in range(rounds):
        for name, fn in (("imread", full), ("inflate_window", hybrid)):
            t0 = time.perf_counter()
            for k in ks:
                fn(k)
            raw[f"{name}_1thread_ms"].append(1e3 * (time.perf_counter() - t0) / len(ks))
            t0 = time.perf_counter()
            for _rep in range(2):
                list(pool.map(fn, ks))
            raw[f"{name}_16threads_fps"].append(2 * len(ks) / (time.perf_counter() - t0))
    pool.shutdown()
    planned = [hybrid(k) for k in ks]
    return {"what": "png_host_decode", "files": len(paths), "frame": [W, H], "rounds": rounds,
            "columns": "[median, min, max]; *_ms per frame on one thread, *_fps frames per second with 16 threads",
            "rows_inflated_mean": float(np.mean([p.plan.rows_inflated for p in planned])), "rows_of_frame": H,
            **{n: med(v) for n, v in raw.items()}}, planned


def inflate_arm(paths, rounds):
    streams = []
    for p in paths:
        with open(p, "rb") as f:
            streams.append(zlib_stream(f.read()))
    plain = H * (1 + 3 * W)
    assert all(PNG.inflate(z, plain) == zlib.decompress(z) for z in streams[:4])
    raw = {"own_inflate_ms": [], "zlib_decompress_ms": []}
    for _ in range(rounds):
        for name, fn in (("own_inflate_ms", lambda z: PNG.inflate(z, plain)), ("zlib_decompress_ms", zlib.decompress)):
            t0 = time.perf_counter()
            for z in streams:
                fn(z)
            raw[name].append(1e3 * (time.perf_counter() - t0) / len(streams))
    return {"what": "png_inflate", "streams": len(streams), "plain_bytes": plain, "stream_bytes_mean": int(np.mean([len(z) for z in streams])),
            "rounds": rounds, "columns": "[median, min, max] milliseconds per whole stream on one thread (the own call copies its result once more)",
            **{n: med(v) for n, v in raw.items()}}


def device_batch(planned, rounds, dev):
    dec = PNG.PNGDecoder(dev)
    rec = {"what": "png_device_batch", "rounds": rounds, "calls_per_window": 10,
           "columns": "[median, min, max] milliseconds per thmr_png_decode_batch call (packing + upload + 2 kernels)"}
    for items in (planned, planned[:1]):
        outs = [torch.empty(p.window[3], p.window[2], 3, dtype=torch.uint8, device=dev) for p in items]
        for _ in range(3):
            dec.decode_planned(items, out=outs)
        torch.cuda.synchronize()
        ms = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _c in range(10):
                dec.decode_planned(items, out=outs)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / 10)
        n = len(items)
        rec[f"items_{n}"] = {"decode_batch_ms": med(ms, 4), "row_bytes_uploaded": int(sum(p.nbytes for p in items)),
                             "window_bytes_written": int(sum(p.window[2] * p.window[3] * 3 for p in items)), "frame_bytes_if_whole": n * H * W * 3}
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
    cx, cy, size = JB.boxes(N, 2)
    path = os.path.join(folder, "synthetic.npz")
    np.savez(path, imgname=np.array([f"f{i % NFILES:02d}.png" for i in range(N)]), center=np.stack([cx, cy], 1), scale=size,
             body_pose=0.3 * rng.normal(size=(N, 72)), has_body_pose=np.ones(N), betas=0.5 * rng.normal(size=(N, 10)), has_betas=np.ones(N),
             body_keypoints_3d=rng.normal(size=(N, 25, 4)), extra_keypoints_3d=rng.normal(size=(N, 19, 4)),
             gender=np.array(["m", "f"] * (N // 2)))
    mcfg = ConfigNode({"MODEL": {"IMAGE_SIZE": P, "IMAGE_MEAN": list(PP.DEFAULT_MEAN), "IMAGE_STD": list(PP.DEFAULT_STD), "BBOX_SHAPE": [192, 256]},
                       "SMPL": {"NUM_BODY_JOINTS": 23}})
    sm, sf = make_synthetic_smpl(HMRConfig(), 1), make_synthetic_smpl(HMRConfig(), 2)
    ds = {mode: ImageDataset(mcfg, path, folder, device=dev, smpl_male=sm, smpl_female=sf, decode=mode) for mode in ("host", "device+png")}
    a, b = ds["host"].batch(range(B)), ds["device+png"].batch(range(B))
    torch.cuda.synchronize()
    assert torch.equal(a["img"], b["img"]), "decode='device+png' must give the crops of decode='host' bit for bit"
    kp = [25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 43]

    def e2e(mode):
        ev = Evaluator(N, kp, 39, metrics=["mode_re", "mode_mpjpe", "mode_pve"], dataset="3DPW-TEST")
        run_eval(model, ds[mode], ev, batch_size=B, device=dev, num_workers=16)

    raw = {"host": [], "device+png": []}
    for mode in raw:
        e2e(mode)
    for _ in range(rounds):
        for mode in raw:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e2e(mode)
            torch.cuda.synchronize()
            raw[mode].append(N / (time.perf_counter() - t0))
    st = ds["device+png"].png_stats
    return {"what": "png_end_to_end", "items": N, "files": NFILES, "batch_size": B, "num_workers": 16, "frame": [W, H],
            "model": "vit_depth=1, dec_depth=1", "rounds": rounds,
            "columns": "[median, min, max] items per second from files (wall clock, synchronised at both ends)",
            "crops_bit_equal": True, "png_fallbacks": st["fallback"], "stream_bytes_per_item": st["stream_bytes"] // max(st["device"], 1),
            "decode_host": med(raw["host"], 1), "decode_device_png": med(raw["device+png"], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_decode.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("png_dec_bench.py needs a GPU: the arms are only comparable on one box in one session")
    dev = torch.device("cuda:0")
    folder = tempfile.mkdtemp()
    paths = write_files(folder)
    cx, cy, size = JB.boxes(NFILES, 1)
    wins = []
    for i in range(NFILES):
        w = PP.source_window(PP.gen_trans_from_patch_cv(cx[i], cy[i], size[i], size[i], P, P, 1.0, 0), P, H, W)
        wins.append((0, 0, 0, 0) if w is None else w)
    recs = [describe(paths, wins)]
    print(json.dumps(recs[-1]), flush=True)
    rec, planned = host_decode(paths, wins, args.rounds)
    recs.append(rec)
    print(json.dumps(rec), flush=True)
    recs.append(inflate_arm(paths, args.rounds))
    print(json.dumps(recs[-1]), flush=True)
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
