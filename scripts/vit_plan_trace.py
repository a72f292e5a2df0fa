"""Same launches: every batch regime of the full path, once per size, for a kernel trace that is compared between two builds of the library.

A refactor of the host-side dispatch (csrc/vit_plan.h, engine.hip) must launch exactly what its parent launched.  The workload creates a
depth-32 engine with max_batch 64 and calls forward once per size for B = 1 ... 40, 48, 64 — the default mode first, then the exact-fp32
mode — and prints the plan the library reports for each size where it can (thmr_debug_vit_plan):

    python scripts/build_ab_lib.py <parent-ref> parent                    # no GPU: build_ab/parent/libtokenhmr_hip.so
    rocprofv3 --kernel-trace --output-format csv -d <dir>/parent -o t -- python scripts/vit_plan_trace.py --lib build_ab/parent/libtokenhmr_hip.so
    rocprofv3 --kernel-trace --output-format csv -d <dir>/new -o t -- python scripts/vit_plan_trace.py
    python scripts/vit_plan_trace.py --compare <dir>/parent <dir>/new --out profiles/vit_plan_trace_equal.json

--compare reads the *kernel_trace.csv of both directories and requires the ORDERED list of (kernel name, grid size, workgroup size) to be
identical; the first argument is the reference.  Exit status 1 if the lists differ (the first differing dispatches are printed)."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = list(range(1, 41)) + [48, 64]


def workload(lib):
    import ctypes as C
    import torch
    from tokenhmr_amd import _cabi
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.engine import Engine
    dev = torch.device("cuda:0")
    cfg = HMRConfig()
    eng = Engine(cfg, max_batch=max(SIZES), device=dev, experiments=lib)
    eng.load_state(W.make_synthetic_state(cfg, 0), W.make_synthetic_tokenizer(cfg, 0))
    eng.load_smpl(make_synthetic_smpl(cfg, 0))
    eng.finalize()
    img = torch.randn(max(SIZES), 3, 256, 256, generator=torch.Generator().manual_seed(4000)).to(dev)
    outs = {B: eng._alloc_outputs(B, taps=False, want_probs=True) for B in SIZES}
    crops = {B: img[:B].contiguous() for B in SIZES}
    torch.cuda.synchronize()
    cc = _cabi.Config(abi_version=_cabi.ABI_VERSION, vit_depth=cfg.vit_depth, dec_depth=cfg.dec_depth, max_batch=max(SIZES), device=0)
    for mode in ("split3", "f32"):
        eng.set_vit_gemm(mode)
        for B in SIZES:
            eng.forward(crops[B], outputs=outs[B])
            if hasattr(eng.lib, "thmr_debug_vit_plan"):
                d = _cabi.VitPlanDesc()
                _cabi.check(eng.lib.thmr_debug_vit_plan(C.byref(cc), 1 if mode == "split3" else 0, B, 1, C.byref(d)), lib=eng.lib)
                print(mode, B, _cabi.VIT_PATHS[d.path], *(f"{n}={_cabi.GEMM_KINDS[getattr(d, n).kind]}/{getattr(d, n).ksplit}"
                                                          for n in ("qkv", "proj", "fc1", "fc2", "to_kv")), f"blk={d.bs_blk}", flush=True)
        torch.cuda.synchronize()
        eng.status()
    print(f"vit_plan_trace: {len(SIZES)} sizes x 2 modes done on {eng.lib.thmr_build_info().decode()}", flush=True)


def dispatches(directory):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if len(files) != 1:
        sys.exit(f"vit_plan_trace: expected one *kernel_trace.csv under {directory}, found {files}")
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r["Dispatch_Id"])))
    return [(r["Kernel_Name"], tuple(int(r["Grid_Size_" + a]) for a in "XYZ"), tuple(int(r["Workgroup_Size_" + a]) for a in "XYZ")) for r in rows]


def compare(ref_dir, new_dir, out):
    ref, new = dispatches(ref_dir), dispatches(new_dir)
    first = next((i for i, (a, b) in enumerate(zip(ref, new)) if a != b), None if len(ref) == len(new) else min(len(ref), len(new)))
    res = {"what": "ordered (kernel name, grid size, workgroup size) of every dispatch of scripts/vit_plan_trace.py under rocprofv3 --kernel-trace: "
                   "reference build vs this build", "sizes": SIZES, "modes": ["split3", "f32"], "vit_depth": 32, "max_batch": max(SIZES),
           "dispatches_reference": len(ref), "dispatches_new": len(new), "distinct_kernels": len({d[0] for d in ref}),
           "identical": first is None}
    if first is not None:
        res["first_difference_at"] = first
        for i in range(max(0, first - 2), min(first + 3, max(len(ref), len(new)))):
            print(i, "ref:", ref[i] if i < len(ref) else None, "\n ", "new:", new[i] if i < len(new) else None)
    line = json.dumps(res)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0 if first is None else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libtokenhmr_hip.so (default: the in-tree shipped library)")
    ap.add_argument("--compare", nargs=2, metavar=("REF_DIR", "NEW_DIR"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.compare[0], a.compare[1], a.out))
    workload(a.lib)
