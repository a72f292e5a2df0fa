"""Times JPEG encoding of device images, device against host, in one process on one GPU box with the arms interleaved, and writes
profiles/jpeg_encode.jsonl.

    python scripts/jpeg_enc_bench.py [--out profiles/jpeg_encode.jsonl] [--rounds 5]

Workloads (the procedural images of scripts/png_bench.py; nothing is committed), all at quality 95 and 4:2:0:
  panels_u8   64 panels of 256x512x3 uint8
  frame       one 1920x1080x3 uint8 frame
  sheet       the `eval.py --render` sheet: (3, 2066, 1292) float32 CHW, encoded through its HWC view with scale=255, rounding="trunc", bgr=False
Arms, each [median, min, max] ms of wall clock over `rounds` alternating rounds, synchronised at both ends, the files in host memory at
the end of either:
  device          JpegEncoder.encode: one descriptor upload, the launches, the scans written into pinned staging, header + copy on the host;
                  device_span_ms is the part of it between two events on the stream, around the call
  host_1thread    device-to-host copy of the raw pixels (+ the float conversion in numpy), then Pillow save(quality=95, subsampling=2)
  host_16threads  the same from a pool of 16 threads (one image cannot be split: at most one thread per image)
Sizes: bytes of the device files over Pillow's (1.0: the files are equal, and the record says whether they are).  Per launch: the
device arm once more under the profiler's kernel timer (torch.profiler), the time of each kernel summed over one call."""
import argparse
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from png_bench import med, picture, to_host_u8  # noqa: E402
from tokenhmr_amd import _cabi  # noqa: E402
from tokenhmr_amd import jpeg as J  # noqa: E402

QUALITY, SUBSAMPLING = 95, "4:2:0"


def host_encode_one(arr):
    """uint8 (H, W, 3) RGB -> bytes."""
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="JPEG", quality=QUALITY, subsampling=2)
    return b.getvalue()


def kernel_times(fn):
    """{kernel name: microseconds summed over one call of fn} from the profiler's device timeline."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.events():
        name = ev.name
        dev_time = getattr(ev, "device_time", None)
        if dev_time is None:
            dev_time = getattr(ev, "cuda_time", 0)
        if "jpegenc_" in name and dev_time:
            short = name[name.index("jpegenc_"):].split("(")[0].split("E")[0]
            out[short] = round(out.get(short, 0.0) + float(dev_time), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encode.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-kernel-times", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    enc = J.JpegEncoder(dev)
    build = _cabi.load().thmr_build_info().decode()

    panels = [picture(256, 512, 100 + i) for i in range(64)]
    sheet = np.ascontiguousarray(np.pad(picture(2064, 1290, 7), ((1, 1), (1, 1), (0, 0))).transpose(2, 0, 1)).astype(np.float32) / np.float32(255)
    workloads = [
        ("panels_u8", [torch.from_numpy(p).to(dev) for p in panels], dict(bgr=True)),
        ("frame", [torch.from_numpy(picture(1080, 1920, 3)).to(dev)], dict(bgr=True)),
        ("sheet", [torch.from_numpy(sheet).to(dev).permute(1, 2, 0)], dict(scale=255.0, rounding="trunc", bgr=False)),
    ]
    pool = ThreadPoolExecutor(16)
    records = []
    for name, images, kw in workloads:
        def device_arm():
            return enc.encode(images, quality=QUALITY, subsampling=SUBSAMPLING, **kw)

        def host_arm(threads):
            arrs = [to_host_u8(t, kw) for t in images]
            return list(pool.map(host_encode_one, arrs)) if threads > 1 else [host_encode_one(a) for a in arrs]

        files, hfiles = device_arm(), host_arm(1)          # warm-up of all arms, and the sizes
        t = {"device": [], "device_span": [], "host_1thread": [], "host_16threads": []}
        for _ in range(args.rounds):
            for arm, fn in (("device", device_arm), ("host_1thread", lambda: host_arm(1)), ("host_16threads", lambda: host_arm(16))):
                torch.cuda.synchronize()
                first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                if arm == "device":
                    first.record()
                fn()
                if arm == "device":
                    last.record()
                torch.cuda.synchronize()
                t[arm].append((time.perf_counter() - t0) * 1e3)
                if arm == "device":
                    t["device_span"].append(first.elapsed_time(last))
        rec = {"what": "jpeg_enc_" + name, "images": len(images), "shape": list(images[0].shape), "dtype": str(images[0].dtype), "rounds": args.rounds,
               "quality": QUALITY, "subsampling": SUBSAMPLING, "columns": "[median, min, max] ms per call over all images, wall clock",
               "raw_bytes": sum(int(np.prod(i.shape)) for i in images), "device_file_bytes": sum(map(len, files)), "host_file_bytes": sum(map(len, hfiles)),
               "device_files_over_host_files": round(sum(map(len, files)) / sum(map(len, hfiles)), 4), "device_files_equal_host_files": files == hfiles,
               "host_encoder": "Pillow save(quality=95, subsampling=2)", "host_threads_used": min(16, len(images)),
               "device_ms": med(t["device"]), "device_span_ms": med(t["device_span"]), "host_1thread_ms": med(t["host_1thread"]), "host_16threads_ms": med(t["host_16threads"]), "build": build}
        rec["device_over_host_16threads"] = round(rec["device_ms"][0] / rec["host_16threads_ms"][0], 4)
        if not args.no_kernel_times:
            try:
                rec["kernel_us_one_call"] = kernel_times(device_arm)
            except Exception as ex:          # the timings above stand without it
                rec["kernel_us_one_call"] = f"unavailable: {type(ex).__name__}: {ex}"
        records.append(rec)
        print(json.dumps(rec), flush=True)
    with open(args.out, "w") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")
    enc.close()


if __name__ == "__main__":
    main()
