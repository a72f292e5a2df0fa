"""Times PNG encoding of device images, device against host, in one process on one GPU box with the arms interleaved, and writes
profiles/png_encode.jsonl.

    python scripts/png_bench.py [--out profiles/png_encode.jsonl] [--rounds 5] [--compression fixed,dynamic]

Workloads (procedural images: a white ground, a shaded disc, a noisy photographic half; nothing is committed):
  panels_u8 / panels_f32   64 panels of 256x512x3, uint8 and float32 in [0, 1] (scale=255)
  frame                    one 1920x1080x3 uint8 frame
  sheet                    the `eval.py --render` sheet: (3, 2066, 1292) float32 CHW as visualize_tensorboard returns it, encoded through its
                           HWC view with scale=255, rounding="trunc", bgr=False
Arms, each [median, min, max] ms of wall clock over `rounds` alternating rounds, synchronised at both ends:
  device          PNGEncoder.encode: the three launches, the copy of the files to the host and the container, files as bytes; one arm
                  per mode of --compression (device_ms / device_file_bytes are the fixed mode's, device_dynamic_* the dynamic mode's)
  host_1thread    device-to-host copy of the raw pixels (+ the float conversion in numpy), then Pillow at compress_level=1 per image
                  (without Pillow: zlib.compress(level 1) of the rows behind a filter-0 byte, and the record says so)
  host_16threads  the same from a pool of 16 threads (one image cannot be split: at most one thread per image)
Sizes: bytes of the device files and of the host files, and for one render-like 256x512x3 panel the file of each mode over
zlib.compress(level 1) of the same filtered bytes."""
import argparse
import io
import json
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tokenhmr_amd import _cabi  # noqa: E402
from tokenhmr_amd import png as P  # noqa: E402

try:
    from PIL import Image
except ImportError:
    Image = None


def picture(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.full((h, w, 3), 255.0, np.float32)
    cx, cy, rad = rng.uniform(0.2, 0.4) * w, rng.uniform(0.4, 0.6) * h, rng.uniform(0.15, 0.3) * min(h, w)
    r = np.hypot(x - cx, y - cy) / rad
    shade = np.sqrt(np.clip(1.0 - r * r, 0.0, 1.0))
    for k in range(3):
        img[..., k] = np.where(r < 1.0, (60 + 50 * k) * shade + 30, img[..., k])
    photo = 128 + 60 * (np.sin(x / 9.0) * np.cos(y / 7.0))[..., None] + rng.normal(0, 12, (h, w, 3)).astype(np.float32)
    half = x >= w // 2
    img[half] = photo[half]
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def med(v, nd=3):
    return [round(statistics.median(v), nd), round(min(v), nd), round(max(v), nd)]


def host_encode_one(arr):
    """uint8 (H, W, C) RGB -> bytes."""
    if Image is not None:
        b = io.BytesIO()
        Image.fromarray(arr).save(b, format="PNG", compress_level=1)
        return b.getvalue()
    h, w, c = arr.shape
    rows = np.concatenate([np.zeros((h, 1), np.uint8), arr.reshape(h, w * c)], axis=1)
    return zlib.compress(rows.tobytes(), 1)


def to_host_u8(t, kw):
    a = t.cpu().numpy()
    if a.dtype != np.uint8:
        a = a * np.float32(kw.get("scale", 1.0))
        a = np.clip(a, 0, 255).astype(np.uint8) if kw.get("rounding") == "trunc" else np.clip(np.rint(a), 0, 255).astype(np.uint8)
    if kw.get("bgr", True):
        a = a[..., ::-1]
    return np.ascontiguousarray(a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_encode.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--compression", default="fixed,dynamic", help="the device arms, comma separated: fixed, dynamic")
    args = ap.parse_args()
    modes = args.compression.split(",")
    assert modes and set(modes) <= {"fixed", "dynamic"}, modes
    key = {"fixed": "device", "dynamic": "device_dynamic"}
    dev = torch.device("cuda:0")
    enc = P.PNGEncoder(dev)
    build = _cabi.load().thmr_build_info().decode()

    panels = [picture(256, 512, 100 + i) for i in range(64)]
    sheet = np.ascontiguousarray(np.pad(picture(2064, 1290, 7), ((1, 1), (1, 1), (0, 0))).transpose(2, 0, 1)).astype(np.float32) / np.float32(255)
    workloads = [
        ("panels_u8", [torch.from_numpy(p).to(dev) for p in panels], dict(bgr=True)),
        ("panels_f32", [(torch.from_numpy(p).to(dev).float() / 255) for p in panels], dict(scale=255.0, bgr=True)),
        ("frame", [torch.from_numpy(picture(1080, 1920, 3)).to(dev)], dict(bgr=True)),
        ("sheet", [torch.from_numpy(sheet).to(dev).permute(1, 2, 0)], dict(scale=255.0, rounding="trunc", bgr=False)),
    ]
    pool = ThreadPoolExecutor(16)
    records = []
    for name, images, kw in workloads:
        def device_arm(mode):
            return enc.encode(images, compression=mode, **kw)

        def host_arm(threads):
            arrs = [to_host_u8(t, kw) for t in images]
            return list(pool.map(host_encode_one, arrs)) if threads > 1 else [host_encode_one(a) for a in arrs]

        files = {m: device_arm(m) for m in modes}
        hfiles = host_arm(1)                      # warm-up of all arms, and the sizes
        t = {**{key[m]: [] for m in modes}, "host_1thread": [], "host_16threads": []}
        for _ in range(args.rounds):
            for arm, fn in [(key[m], lambda m=m: device_arm(m)) for m in modes] + [("host_1thread", lambda: host_arm(1)), ("host_16threads", lambda: host_arm(16))]:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t[arm].append((time.perf_counter() - t0) * 1e3)
        raw = sum(int(np.prod(i.shape)) for i in images)
        rec = {"what": "png_" + name, "images": len(images), "shape": list(images[0].shape), "dtype": str(images[0].dtype), "rounds": args.rounds,
               "columns": "[median, min, max] ms per call over all images, wall clock", "raw_bytes": raw,
               **{key[m] + "_file_bytes": sum(map(len, files[m])) for m in modes}, "host_file_bytes": sum(map(len, hfiles)),
               "host_encoder": "Pillow compress_level=1" if Image is not None else "zlib.compress(level 1) of filter-0 rows (no Pillow)",
               "host_threads_used": min(16, len(images)),
               **{key[m] + "_ms": med(t[key[m]]) for m in modes}, "host_1thread_ms": med(t["host_1thread"]),
               "host_16threads_ms": med(t["host_16threads"]), "build": build}
        for m in modes:
            rec[key[m] + "_over_host_16threads"] = round(rec[key[m] + "_ms"][0] / rec["host_16threads_ms"][0], 4)
            rec[key[m] + "_files_over_host_files"] = round(rec[key[m] + "_file_bytes"] / rec["host_file_bytes"], 4)
        records.append(rec)
        print(json.dumps(rec), flush=True)

    import _png_reader as R
    one = panels[0]
    for m in modes:
        data = enc.encode([torch.from_numpy(one).to(dev)], bgr=False, compression=m)[0]
        pixels, _, stream = R.read(data)
        assert np.array_equal(pixels, one) and data == P.encode_host(one, bgr=False, compression=m)
        z = len(zlib.compress(stream, 1))
        rec = {"what": "png_size", "compression": m, "image": "render-like 256x512x3 (panel 0)", "file_bytes": len(data),
               "zlib_level1_of_same_filtered_bytes": z, "ratio": round(len(data) / z, 4), "segment_bytes": P.segment_bytes(),
               "device_equals_host": True, "build": build}
        records.append(rec)
        print(json.dumps(rec), flush=True)
    with open(args.out, "w") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")
    enc.close()


if __name__ == "__main__":
    main()
