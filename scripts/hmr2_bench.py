"""The HMR2 head next to the token head on one box, in one process, interleaved (profiles/hmr2_head.jsonl).

Two engines of each kind live in one process (the library's per-device turnstile orders their calls):

  head    THMR_PROF_HEAD class time (HIP events around everything behind the to_kv GEMM) of thmr_head_forward at 1, 8 and 64 crops,
          engines of reduced ViT depth (the head does not depend on it).  The arms alternate, `reps` windows of `iters` profiled calls
          each; a window's figure is the class's ms per launch.  The HMR2 head does a strict subset of the token head's work, so the
          condition is median(hmr2) <= median(token) + spread(token), the spread being the token arm's own (max - min) / 2 over its
          windows.
  forward thmr_forward at 64 crops, release depth, default mode: ms per call between device events around `iters` back-to-back calls,
          the arms alternating; crops/s of both and the same condition.

    python scripts/hmr2_bench.py [--reps 7] [--iters 20] [--skip-forward] [--out profiles/hmr2_head.jsonl]

Every line written is one JSON record with the library's build id.  Exit status 1 if a condition fails.
"""
import argparse
import json
import os
import statistics
import sys
from dataclasses import replace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    return (max(xs) - min(xs)) / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--fwd-iters", type=int, default=8)
    ap.add_argument("--skip-forward", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hmr2_head.jsonl"))
    a = ap.parse_args()

    import torch
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.engine import Engine

    if not torch.cuda.is_available():
        sys.exit("hmr2_bench: needs a GPU (no CPU fallback, no CPU timing)")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    records, failed = [], False

    def emit(rec):
        records.append(rec)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)

    def make(cfg, max_batch, seed=0):
        e = Engine(cfg, max_batch=max_batch, device=dev)
        e.load_state(W.make_synthetic_state(cfg, seed), W.make_synthetic_tokenizer(cfg, seed) if cfg.head == "token" else None)
        e.load_smpl(make_synthetic_smpl(cfg, seed))
        e.finalize()
        return e

    # ---- 1. head class time -------------------------------------------------------------------------------------------------
    tcfg = HMRConfig(vit_depth=1, dec_depth=6)
    arms = {"token": make(tcfg, 64), "hmr2": make(replace(tcfg, head="hmr2"), 64)}
    build = arms["token"].lib.thmr_build_info().decode()
    ctx = torch.randn(64, 192, 1280, generator=torch.Generator().manual_seed(12)).to(dev)

    def head_call(name, x):
        arms[name].head_forward(x, want_probs=False)

    for B in (1, 8, 64):
        x = ctx[:B].contiguous()
        ms = {k: [] for k in arms}
        for name in arms:
            for _ in range(5):
                head_call(name, x)
        torch.cuda.synchronize()
        for rep in range(a.reps):
            for name in (("token", "hmr2") if rep % 2 == 0 else ("hmr2", "token")):
                e = arms[name]
                head_call(name, x)                                      # one untimed call after the switch
                e.prof_enable(True)
                for _ in range(a.iters):
                    head_call(name, x)
                torch.cuda.synchronize()
                p = e.prof_collect()["head"]
                e.prof_enable(False)
                ms[name].append(p["ms"] / max(1, p["launches"]))
        mt, mh, sp = statistics.median(ms["token"]), statistics.median(ms["hmr2"]), spread(ms["token"])
        ok = mh <= mt + sp
        failed |= not ok
        emit({"what": "head class (THMR_PROF_HEAD) ms per call, thmr_head_forward, arms interleaved", "build": build, "crops": B,
              "reps": a.reps, "iters_per_window": a.iters, "gpu": torch.cuda.get_device_name(0),
              "token_ms_windows": [round(v, 4) for v in ms["token"]], "hmr2_ms_windows": [round(v, 4) for v in ms["hmr2"]],
              "token_ms_median": round(mt, 4), "hmr2_ms_median": round(mh, 4), "token_spread_ms": round(sp, 4),
              "hmr2_spread_ms": round(spread(ms["hmr2"]), 4), "hmr2_over_token": round(mh / mt, 4), "hmr2_le_token_within_spread": ok})
    for e in arms.values():
        e.status()
        e.close()
    arms.clear()
    torch.cuda.empty_cache()

    # ---- 2. full forward, 64 crops, release depth, default mode ----------------------------------------------------------------
    if not a.skip_forward:
        fcfg = HMRConfig()
        arms = {"token": make(fcfg, 64), "hmr2": make(replace(fcfg, head="hmr2"), 64)}
        img = torch.randn(64, 3, 256, 256, generator=torch.Generator().manual_seed(4000)).to(dev)
        outs = {k: e._alloc_outputs(64, taps=False, want_probs=True) for k, e in arms.items()}
        ms = {k: [] for k in arms}
        for name, e in arms.items():
            assert e.vit_gemm() == "split3"
            for _ in range(3):
                e.forward(img, outputs=outs[name])
        torch.cuda.synchronize()
        for rep in range(a.reps):
            for name in (("token", "hmr2") if rep % 2 == 0 else ("hmr2", "token")):
                e = arms[name]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e.forward(img, outputs=outs[name])
                e0.record()
                for _ in range(a.fwd_iters):
                    e.forward(img, outputs=outs[name])
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1) / a.fwd_iters)
        mt, mh, sp = statistics.median(ms["token"]), statistics.median(ms["hmr2"]), spread(ms["token"])
        ok = mh <= mt + sp
        failed |= not ok
        emit({"what": "thmr_forward ms per 64-crop call, release depth, split3 mode, arms interleaved", "build": build, "crops": 64,
              "reps": a.reps, "iters_per_window": a.fwd_iters, "gpu": torch.cuda.get_device_name(0),
              "token_ms_windows": [round(v, 3) for v in ms["token"]], "hmr2_ms_windows": [round(v, 3) for v in ms["hmr2"]],
              "token_ms_median": round(mt, 3), "hmr2_ms_median": round(mh, 3), "token_spread_ms": round(sp, 3),
              "token_crops_per_s": round(64e3 / mt, 1), "hmr2_crops_per_s": round(64e3 / mh, 1), "hmr2_le_token_within_spread": ok})
        for e in arms.values():
            e.status()
            e.close()
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
