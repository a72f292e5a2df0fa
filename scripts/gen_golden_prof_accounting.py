"""Record the fixture that pins the engine profiler's HOST-SIDE accounting:

  tests/golden/prof_accounting.json   per case, for every profiler class: launches, flops and bytes as thmr_prof_collect reports them
                                      after ONE thmr_forward, from a library built from another commit (the parent of the change that
                                      must not move them), whose id is recorded.

Each ProfScope of csrc/engine.hip records a class, a flop count and a byte count computed on the host from the call's shapes and from the
plan (vit_plan.h), so the three numbers are deterministic and a case's record is at once a census of the launch sequence per class and of
the accounting formulas.  `ms` is measured and is never recorded.  The cases walk every regime of vit_plan.h (the smallest batch that
reaches each), both modes, both heads, the every-fourth-fc1 sampling of profiler mode "fc1" and the experiments library's
THMR_SPLIT3_SMALL path.  tests/test_gpu_pipeline.py::test_profiler_accounting_is_pinned imports CASES and run_case from here.

    python scripts/build_ab_lib.py <commit> parent                                  (no GPU; --lib)
    --exp-lib: libtokenhmr_hip_exp.so as that commit's own __graft_entry__.build() makes it in an exported copy of the commit
    (build_ab_lib.py <commit> <name> -DTHMR_EXPERIMENTS stops at build()'s own check that the shipped library is not an experiments build)
    python scripts/gen_golden_prof_accounting.py --lib build_ab/parent/libtokenhmr_hip.so --exp-lib build_ab/parent_exp/libtokenhmr_hip.so   (GPU)
"""
import argparse
import functools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "prof_accounting.json")

DEC_DEPTH, MAX_BATCH = 2, 32
# batch sizes: the smallest that reach each regime of vit_plan.h — 1 ring16 + key-split attention, 3 four-way split-K with fc2's planes in
# scratch, 5 two-way split-K, 7 the fp32 mid split, 16 proj unsplit with fc2 split, 17 fp32 unsplit, 32 all unsplit
REGIME_BATCHES = (1, 3, 5, 7, 16, 17, 32)


def _case(name, mode, batch, vit_depth=2, prof=True, head="token", lib="shipped", env=None):
    return {"name": name, "mode": mode, "batch": batch, "vit_depth": vit_depth, "prof": prof, "head": head, "lib": lib, "env": env or {}}


CASES = tuple(
    [_case(f"all.{m}.b{b}", m, b) for m in ("split3", "f32") for b in REGIME_BATCHES]
    # depth 8 makes the every-fourth sampling of profiler mode "fc1" visible
    + [_case(f"fc1.{m}.b4", m, 4, vit_depth=8, prof="fc1") for m in ("split3", "f32")]
    + [_case("all.hmr2.split3.b4", "split3", 4, head="hmr2")]
    + [_case(f"all.small.split3.b{b}", "split3", b, lib="exp", env={"THMR_SPLIT3_SMALL": "1"}) for b in (1, 6)]
    # with the knob alone the default mode takes a call back from three crops on (the case above at 6 crops runs THMR_VIT_PATH_SPLIT3);
    # THMR_SPLIT3_MIN_B=7 leaves six crops, the largest batch of the regime, to THMR_VIT_PATH_SPLIT3_SMALL as well
    + [_case("all.small.minb7.split3.b6", "split3", 6, lib="exp", env={"THMR_SPLIT3_SMALL": "1", "THMR_SPLIT3_MIN_B": "7"})])


@functools.lru_cache(maxsize=None)
def _assets(vit_depth, head):
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    cfg = HMRConfig(vit_depth=vit_depth, dec_depth=DEC_DEPTH, head=head)
    tok = W.make_synthetic_tokenizer(cfg, 0) if head == "token" else None
    return cfg, W.make_synthetic_state(cfg, 0), tok, make_synthetic_smpl(cfg, 0)


def case_inputs(case):
    """(cfg, state, tokenizer or None, smpl, img on the CPU) of a case: seeded, the same for the generator and the test."""
    import torch
    img = torch.randn(case["batch"], 3, 256, 256, generator=torch.Generator().manual_seed(4000))
    return _assets(case["vit_depth"], case["head"]) + (img,)


def run_case(case, device, libs, inputs=None):
    """One profiled thmr_forward of `case`.  libs: {"shipped": ..., "exp": ...}, each an `experiments=` argument of Engine (None / True = the
    in-tree libraries, a path = another build).  Returns ({class: {launches, flops, bytes}}, the forward's outputs)."""
    import torch
    from tokenhmr_amd.engine import Engine
    cfg, sd, tok, smpl, img = inputs or case_inputs(case)
    old = {k: os.environ.get(k) for k in case["env"]}
    os.environ.update(case["env"])          # the experiments library reads its knobs when the engine is created
    try:
        eng = Engine(cfg, max_batch=MAX_BATCH, device=device, experiments=libs[case["lib"]])
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        eng.load_state(sd, tok)
        eng.load_smpl(smpl)
        eng.finalize()
        eng.set_vit_gemm(case["mode"])
        eng.prof_enable(case["prof"])
        out = eng.forward(img.to(device), taps=True)
        torch.cuda.synchronize()
        eng.status()
        prof = eng.prof_collect()
        out = {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}
    finally:
        eng.close()
    return {n: {"launches": int(v["launches"]), "flops": float(v["flops"]), "bytes": float(v["bytes"])} for n, v in prof.items()}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="the recorded commit's shipped library (scripts/build_ab_lib.py)")
    ap.add_argument("--exp-lib", required=True, help="the same commit built with -DTHMR_EXPERIMENTS")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    import torch
    libs = {"shipped": os.path.abspath(a.lib), "exp": os.path.abspath(a.exp_lib)}
    with open(os.path.join(os.path.dirname(libs["shipped"]), "SOURCE")) as f:      # written by build_ab_lib.py: "<sha> (<ref>) <defines>"
        commit = f.read().split()[0]
    dev = torch.device("cuda:0")
    cases = []
    for case in CASES:
        prof, _ = run_case(case, dev, libs)
        cases.append(dict(case, expect=prof))
        print(case["name"], {k: v["launches"] for k, v in prof.items() if v["launches"]}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"what": "launches / flops / bytes per profiler class after one thmr_forward (scripts/gen_golden_prof_accounting.py)",
                   "commit": commit, "dec_depth": DEC_DEPTH, "max_batch": MAX_BATCH, "cases": cases}, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes) from {commit}")


if __name__ == "__main__":
    main()
