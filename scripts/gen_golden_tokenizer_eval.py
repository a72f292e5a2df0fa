"""Writes tests/golden/tokenizer_eval.npz: the reference's three reconstruction errors on seeded inputs.

    calculate_pose_reconstruction_error    tokenization/utils/eval_poseVQ.py:47-48
    calculate_mesh_reconstruction_error    :50-51
    calculate_jnts_reconstruction_error    :53-55   (valid_joints = 1..21)

The reference's file is executed IN PLACE (nothing of it is copied), loaded by path through oracle.ref_import's loader with stand-ins
for the modules its import lines need and this image may lack (tqdm, utils.pose_visualize, torch.utils.tensorboard): none of them is
touched by the three functions.  The fixture holds seeds, shapes and the recorded float32 results only — the inputs are regenerated
from the seed by `eval_inputs` (tests import it from here), so the file stays a few KB.

    python scripts/gen_golden_tokenizer_eval.py [--check]
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "tokenizer_eval.npz")

# name -> (seed, shape of gt and pred, the reference function)
CASES = {"pose": (101, (5, 21, 3, 3), "calculate_pose_reconstruction_error"),
         "mesh": (102, (3, 6890, 3), "calculate_mesh_reconstruction_error"),
         "jnts": (103, (3, 73, 3), "calculate_jnts_reconstruction_error")}


def eval_inputs(seed, shape, noise=0.05):
    """(gt, pred), float32: gt ~ N(0,1), pred = gt + noise * N(0,1)."""
    g = torch.Generator().manual_seed(int(seed))
    gt = torch.randn(*shape, generator=g, dtype=torch.float32)
    return gt, gt + noise * torch.randn(*shape, generator=g, dtype=torch.float32)


def load_reference_eval():
    """tokenization/utils/eval_poseVQ.py as a module, its absent imports stood in for."""
    from oracle import ref_import
    if not ref_import.available():
        raise RuntimeError(f"reference tree not found at {ref_import.REF}")

    # oracle/ref_import.py's own stand-ins (_install_stubs: timm, smplx) do not cover what THIS file imports, and every other golden script
    # relies on that module as it is, so the three modules are stood in for here, in ref_import's style (an empty module per missing name, installed
    # only where the real import fails), and the file is executed through ref_import's by-path loader like every other reference module
    def standin(name, **attrs):
        try:
            importlib.import_module(name)
        except Exception:
            parts = name.split(".")
            for i in range(1, len(parts) + 1):
                sys.modules.setdefault(".".join(parts[:i]), types.ModuleType(".".join(parts[:i])))
            for k, v in attrs.items():
                setattr(sys.modules[name], k, v)

    standin("tqdm", tqdm=lambda it, *a, **k: it)
    standin("utils.pose_visualize", visualize_from_mesh=lambda *a, **k: None)
    standin("torch.utils.tensorboard", SummaryWriter=object)
    return ref_import._load("_ref_tok_eval_poseVQ", os.path.join(ref_import.REF, "tokenization", "utils", "eval_poseVQ.py"))


def compute():
    mod = load_reference_eval()
    out = {}
    for name, (seed, shape, fn) in CASES.items():
        gt, pred = eval_inputs(seed, shape)
        r = getattr(mod, fn)(gt, pred)
        assert r.dtype == torch.float32 and r.dim() == 0
        out[f"{name}.seed"] = np.array(seed, dtype=np.int64)
        out[f"{name}.shape"] = np.array(shape, dtype=np.int64)
        out[f"{name}.value"] = r.numpy().astype(np.float32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed fixture instead of writing it")
    args = ap.parse_args()
    new = compute()
    if args.check:
        old = np.load(OUT)
        for k, v in new.items():
            assert np.array_equal(old[k], v), (k, old[k], v)
        print("tokenizer_eval.npz: the reference reproduces the committed values bit for bit")
        return
    np.savez(OUT, **new)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): " + ", ".join(f"{k} = {new[k + '.value']:.8f}" for k in CASES))


if __name__ == "__main__":
    main()
