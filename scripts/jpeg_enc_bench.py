"""Times JPEG encoding of device images, device against host, in one process on one GPU box with the arms interleaved, and writes
profiles/jpeg_encode.jsonl.

    python scripts/jpeg_enc_bench.py [--out profiles/jpeg_encode.jsonl] [--append] [--rounds 5] [--calls 10] [--other-lib PATH]

Workloads (the procedural images of scripts/png_bench.py; nothing is committed), all at quality 95 and 4:2:0:
  panels_u8   64 panels of 256x512x3 uint8
  frame       one 1920x1080x3 uint8 frame
  sheet       the `eval.py --render` sheet: (3, 2066, 1292) float32 CHW, encoded through its HWC view with scale=255, rounding="trunc", bgr=False
Arms, each [median, min, max] ms of wall clock per call over `rounds` alternating rounds, synchronised at both ends, the files in host
memory at the end of either.  A device arm runs one untimed call and then `--calls` timed ones per round (a device arm straight after
the host arms' tens of ms would pay for waking an idle GPU), and the order of the device arms rotates from round to round:
  device          JpegEncoder.encode: one descriptor upload, the launches, the scans written into pinned staging, header + copy on the host;
                  device_span_ms is the part of it between two events on the stream, around the call
  device_optimize the same call with optimize=True: the symbol histogram and the table build between transform and count, the image's
                  own code words in count and pack (device_optimize_span_ms as above)
  other_build     --other-lib PATH: the default call through ANOTHER build of this library (the parent commit's, say) loaded beside
                  this one, interleaved with the rest: whether the default arm moved is read against it, not against an older session
  host_1thread    device-to-host copy of the raw pixels (+ the float conversion in numpy), then Pillow save(quality=95, subsampling=2)
  host_16threads  the same from a pool of 16 threads (one image cannot be split: at most one thread per image)
  host_optimize_1thread / _16threads    the two host arms with Pillow's optimize=True
Sizes: bytes of the device files over Pillow's (1.0: the files are equal, and the record says whether they are).  Per launch: the
device arm, and the optimize arm, once more under the profiler's kernel timer (torch.profiler), the time of each kernel summed over one
call: jpegenc_tables_kernel is the cost of the table-build launch alone, jpegenc_histogram_kernel that of the statistics.  The optimised
files' bytes over the default files' are in optimize_over_default_bytes (and whether they equal Pillow's optimize=True files)."""
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


def host_encode_one(arr, optimize=False):
    """uint8 (H, W, 3) RGB -> bytes."""
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="JPEG", quality=QUALITY, subsampling=2, optimize=optimize)
    return b.getvalue()


def host_encode_one_optimize(arr):
    return host_encode_one(arr, True)


def encoder_of(path, dev):
    """A JpegEncoder over another build of the library (its default call needs nothing that build lacks)."""
    other, load = _cabi.load(exp=path), _cabi.load
    _cabi.load = lambda exp=None: other
    try:
        return J.JpegEncoder(dev), other.thmr_build_info().decode()
    finally:
        _cabi.load = load


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
    ap.add_argument("--calls", type=int, default=10, help="timed calls of a device arm per round, after one untimed call")
    ap.add_argument("--no-kernel-times", action="store_true")
    ap.add_argument("--append", action="store_true", help="add the rows to --out instead of replacing it")
    ap.add_argument("--other-lib", default=None, help="another build of libtokenhmr_hip.so: its default arm is timed beside this one's")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    enc = J.JpegEncoder(dev)
    other, other_build = encoder_of(args.other_lib, dev) if args.other_lib else (None, None)
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

        def optimize_arm():
            return enc.encode(images, quality=QUALITY, subsampling=SUBSAMPLING, optimize=True, **kw)

        def other_arm():
            return other.encode(images, quality=QUALITY, subsampling=SUBSAMPLING, **kw)

        def host_arm(threads, one=host_encode_one):
            arrs = [to_host_u8(t, kw) for t in images]
            return list(pool.map(one, arrs)) if threads > 1 else [one(a) for a in arrs]

        files, hfiles = device_arm(), host_arm(1)          # warm-up of all arms, and the sizes
        ofiles, ohfiles = optimize_arm(), host_arm(1, host_encode_one_optimize)
        arms = [("device", device_arm), ("device_optimize", optimize_arm)] + ([("other_build", other_arm)] if other else []) + \
               [("host_1thread", lambda: host_arm(1)), ("host_16threads", lambda: host_arm(16)),
                ("host_optimize_1thread", lambda: host_arm(1, host_encode_one_optimize)), ("host_optimize_16threads", lambda: host_arm(16, host_encode_one_optimize))]
        if other:
            assert other_arm() == files, "the other build writes other default files"
        t = {a: [] for a, _ in arms}
        t.update({"device_span": [], "device_optimize_span": [], "other_build_span": []})
        ndev = sum(not a.startswith("host") for a, _ in arms)
        for rnd in range(args.rounds):
            # a device arm that follows tens of ms of host work finds the GPU idle and pays for waking it, whichever arm it is: each
            # device arm runs one untimed call first, then `calls` timed ones (the figure is their mean), and their order rotates
            order = [arms[(k + rnd) % ndev] for k in range(ndev)] + arms[ndev:]
            for arm, fn in order:
                on_device = not arm.startswith("host")
                calls = args.calls if on_device else 1
                if on_device:
                    fn()
                torch.cuda.synchronize()
                first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                if on_device:
                    first.record()
                for _ in range(calls):
                    fn()
                if on_device:
                    last.record()
                torch.cuda.synchronize()
                t[arm].append((time.perf_counter() - t0) * 1e3 / calls)
                if on_device:
                    t[arm + "_span"].append(first.elapsed_time(last) / calls)
        rec = {"what": "jpeg_enc_" + name, "images": len(images), "shape": list(images[0].shape), "dtype": str(images[0].dtype), "rounds": args.rounds, "device_calls_per_round": args.calls,
               "quality": QUALITY, "subsampling": SUBSAMPLING, "columns": "[median, min, max] ms per call over all images, wall clock",
               "raw_bytes": sum(int(np.prod(i.shape)) for i in images), "device_file_bytes": sum(map(len, files)), "host_file_bytes": sum(map(len, hfiles)),
               "device_files_over_host_files": round(sum(map(len, files)) / sum(map(len, hfiles)), 4), "device_files_equal_host_files": files == hfiles,
               "host_encoder": "Pillow save(quality=95, subsampling=2)", "host_threads_used": min(16, len(images)),
               "device_ms": med(t["device"]), "device_span_ms": med(t["device_span"]), "host_1thread_ms": med(t["host_1thread"]), "host_16threads_ms": med(t["host_16threads"]), "build": build}
        rec["device_over_host_16threads"] = round(rec["device_ms"][0] / rec["host_16threads_ms"][0], 4)
        rec.update({"device_optimize_ms": med(t["device_optimize"]), "device_optimize_span_ms": med(t["device_optimize_span"]),
                    "host_optimize_1thread_ms": med(t["host_optimize_1thread"]), "host_optimize_16threads_ms": med(t["host_optimize_16threads"]),
                    "host_optimize_encoder": "Pillow save(quality=95, subsampling=2, optimize=True)",
                    "optimize_file_bytes": sum(map(len, ofiles)), "optimize_over_default_bytes": round(sum(map(len, ofiles)) / sum(map(len, files)), 4),
                    "optimize_files_equal_host_optimize_files": ofiles == ohfiles,
                    "device_optimize_over_device": round(med(t["device_optimize"])[0] / rec["device_ms"][0], 4)})
        if other:
            rec.update({"other_build": other_build, "other_build_device_ms": med(t["other_build"]), "other_build_device_span_ms": med(t["other_build_span"]),
                        "device_over_other_build": round(rec["device_ms"][0] / med(t["other_build"])[0], 4)})
        if not args.no_kernel_times:
            for key, fn in (("kernel_us_one_call", device_arm), ("kernel_us_one_call_optimize", optimize_arm)):
                try:
                    rec[key] = kernel_times(fn)
                except Exception as ex:          # the timings above stand without it
                    rec[key] = f"unavailable: {type(ex).__name__}: {ex}"
        records.append(rec)
        print(json.dumps(rec), flush=True)
    with open(args.out, "a" if args.append else "w") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")
    enc.close()
    if other:
        other.close()


if __name__ == "__main__":
    main()
