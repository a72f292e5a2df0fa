"""The token path of this tree next to a checkout of another commit (its parent), on one box in one session (profiles/hmr2_head.jsonl).

`--other DIR` is a BUILT checkout of the commit to compare with (python __graft_entry__.py in it first).  Two records:

  dump    `bench.py --dump-outputs` in each tree (seeded inputs and weights): every dumped array of this tree must equal the other
          tree's element for element, and both must dump the same set of names.
  bench   default `bench.py` lines of the two trees, alternating (`--reps` per arm, the order flipping each round); the medians must lie
          inside one arm's spread: |median(this) - median(other)| <= max over the arms of (max - min) / 2.

    python scripts/token_path_check.py --other ../parent [--reps 3] [--out profiles/hmr2_head.jsonl]

Every bench.py run is a child process of its own under a time limit; the first one that fails ends the script (nothing else is started
on the GPU after it).  Exit status 1 if a condition fails.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(tree, extra, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1"] + extra
    r = subprocess.run(cmd, cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit(f"token_path_check: {' '.join(cmd)} in {tree} ended with status {r.returncode}; nothing more is run\n{r.stderr[-2000:]}")
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print(f"# {os.path.relpath(tree, ROOT)}: bench.py {' '.join(extra)} -> {line.get('value')} {line.get('unit')}", flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True, help="a built checkout of the commit to compare with")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds one bench.py run may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hmr2_head.jsonl"))
    a = ap.parse_args()
    trees = {"this": ROOT, "other": os.path.abspath(a.other)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    failed = False

    def emit(rec):
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)

    # ---- dumped outputs, element for element ------------------------------------------------------------------------------------
    builds, arrays = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, tree in trees.items():
            d = os.path.join(tmp, name)
            line = run_bench(tree, ["--steps", "2", "--warmup", "1", "--dump-outputs", d], a.limit)
            builds[name] = line.get("build")
            arrays[name] = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}
    names = sorted(arrays["this"])
    same_names = names == sorted(arrays["other"])
    unequal = [k for k in names if k in arrays["other"] and not np.array_equal(arrays["this"][k], arrays["other"][k])]
    ok = same_names and bool(names) and not unequal
    failed |= not ok
    emit({"what": "bench.py --dump-outputs of this tree vs the other tree, element for element", "build": builds["this"],
          "other_build": builds["other"], "arrays": names, "elements": int(sum(arrays["this"][k].size for k in names)),
          "same_names": same_names, "unequal": unequal, "all_equal": ok})

    # ---- default bench lines, alternating -----------------------------------------------------------------------------------------
    vals = {k: [] for k in trees}
    for rep in range(a.reps):
        for name in (("this", "other") if rep % 2 == 0 else ("other", "this")):
            line = run_bench(trees[name], ["--steps", str(a.steps), "--warmup", str(a.warmup)], a.limit)
            vals[name].append(float(line["value"]))
    med = {k: statistics.median(v) for k, v in vals.items()}
    spread = {k: (max(v) - min(v)) / 2 for k, v in vals.items()}
    ok = abs(med["this"] - med["other"]) <= max(spread.values())
    failed |= not ok
    emit({"what": "default bench.py crops/s of this tree and the other tree, runs alternating", "build": builds["this"],
          "other_build": builds["other"], "steps": a.steps, "warmup": a.warmup, "this_crops_per_s": vals["this"],
          "other_crops_per_s": vals["other"], "this_median": med["this"], "other_median": med["other"], "this_spread": round(spread["this"], 3),
          "other_spread": round(spread["other"], 3), "this_over_other": round(med["this"] / med["other"], 5), "medians_inside_one_spread": ok})
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
