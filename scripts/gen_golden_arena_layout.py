"""Record the fixture that pins the engine's checkpoint contract and the byte layout of its weight arena:

  tests/golden/arena_layout.json   from a library built from another commit (the parent of the change that must not move them), whose
                                   id and `src:` hash (thmr_build_info) are recorded.  Data only: names, integers, hex digests.

The weight arena is broadcast between ranks byte for byte, so a tensor that moved is a wrong model on every receiver.  Two parts:

  host   (no device)  for every config of HOST_CONFIGS: the whole thmr_spec list (names in order with numel), thmr_arena_bytes (weights and
         scratch) and thmr_mode_bytes in both modes.  tests/test_arena_layout_host.py.
  device for every case of GPU_CASES, on the smallest config thmr_create accepts: the engine is handed a ZEROED arena, every tensor and
         SMPL array is filled by a closed formula of (tensor ordinal, element index) that is exact in fp32 (no torch generator: those are
         stable per torch version only), and the sha256 of the whole arena is taken twice: after the load (only copies have run: every
         checkpoint slot, the SMPL block, the index tables, the padding rows, the flag words) and after finalize in the fp32 mode (the
         repacked convs, the codebook transpose, the code norms, the derived SMPL regions, the encoder repacks).
         tests/test_gpu_arena_layout.py.

    python scripts/build_ab_lib.py <commit> parent                                       (no GPU)
    python scripts/gen_golden_arena_layout.py --lib build_ab/parent/libtokenhmr_hip.so   (GPU; run it twice: --check compares with the file
                                                                                          instead of writing it, which is the determinism test)
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "arena_layout.json")

HOST_CONFIGS = tuple({"vit_depth": v, "dec_depth": d, "head": h, "max_batch": b}
                     for v, d in ((1, 1), (2, 2), (32, 6)) for h in ("token", "hmr2") for b in (2, 64))
VIT_DEPTH, DEC_DEPTH, MAX_BATCH = 1, 1, 2          # the device cases
GPU_CASES = ({"name": "token.encoder", "head": "token", "encoder": True},
             {"name": "token", "head": "token", "encoder": False},
             {"name": "hmr2", "head": "hmr2", "encoder": False})
SMPL_FLOATS = ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights", "J19_regressor")


def _ccfg(lib, vit_depth, dec_depth, head, max_batch):
    from tokenhmr_amd import _cabi
    return _cabi.Config(abi_version=lib.thmr_abi_version(), vit_depth=vit_depth, dec_depth=dec_depth, max_batch=max_batch, device=0,
                        flags=_cabi.CFG_HEAD_HMR2 if head == "hmr2" else 0)


def host_record(lib, vit_depth, dec_depth, head, max_batch):
    """What the library says about one config without a device: spec, arena bytes, mode bytes."""
    cfg = _ccfg(lib, vit_depth, dec_depth, head, max_batch)
    name, numel = C.c_char_p(), C.c_int64()
    n = lib.thmr_spec(C.byref(cfg), -1, None, None)
    spec = []
    for i in range(n):
        assert lib.thmr_spec(C.byref(cfg), i, C.byref(name), C.byref(numel)) == n
        spec.append([name.value.decode(), numel.value])
    wb, sb = C.c_size_t(), C.c_size_t()
    assert lib.thmr_arena_bytes(C.byref(cfg), C.byref(wb), C.byref(sb)) == 0
    modes = []
    for mode in (0, 1):
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        assert lib.thmr_mode_bytes(C.byref(cfg), mode, C.byref(a), C.byref(b), C.byref(c)) == 0
        modes.append([a.value, b.value, c.value])
    return {"spec": spec, "weight_bytes": wb.value, "scratch_bytes": sb.value, "mode_bytes": modes}


def fill(ordinal, numel):
    """Element k of tensor `ordinal`: ((ordinal * 40503 + k * 9973) % 65521 - 32760) / 65536, a 16-bit integer over 2^16: exact in fp32."""
    import torch
    k = torch.arange(numel, dtype=torch.int64)
    return (((ordinal * 40503 + k * 9973) % 65521 - 32760).to(torch.float32) / 65536.0)


def case_inputs(case):
    """(cfg, state + tokenizer tensors, smpl) of a device case.  Ordinals: the tensors of weights.spec, tokenizer_spec and
    tokenizer_encoder_spec in that order from 0, the six float arrays of SMPL_FLOATS from 1000; the integer arrays are the real SMPL tables."""
    import math
    import torch
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.config import HMRConfig, SMPL_PARENTS, SMPL_EXTRA_VERTS, SMPL_TO_OPENPOSE
    cfg = HMRConfig(vit_depth=VIT_DEPTH, dec_depth=DEC_DEPTH, head=case["head"])
    entries = list(W.spec(cfg))
    if case["head"] == "token":
        entries += list(W.tokenizer_spec(cfg))
        enc = list(W.tokenizer_encoder_spec(cfg))
        entries += enc if case["encoder"] else [None] * len(enc)      # the ordinals behind them do not depend on the case
    tensors = {}
    for i, ent in enumerate(entries):
        if ent is not None:
            tensors[ent[0]] = fill(i, math.prod(ent[1])).reshape(ent[1])
    shapes = {"v_template": (6890, 3), "shapedirs": (6890, 3, 10), "posedirs": (207, 20670), "J_regressor": (24, 6890),
              "lbs_weights": (6890, 24), "J19_regressor": (19, 6890)}
    smpl = {k: fill(1000 + i, math.prod(shapes[k])).reshape(shapes[k]) for i, k in enumerate(SMPL_FLOATS)}
    smpl["parents"] = torch.tensor(SMPL_PARENTS, dtype=torch.int32)
    smpl["extra_verts"] = torch.tensor(SMPL_EXTRA_VERTS, dtype=torch.int32)
    smpl["joint_map"] = torch.tensor(SMPL_TO_OPENPOSE, dtype=torch.int32)
    return cfg, tensors, smpl


def run_case(case, device, lib=None):
    """The two digests of a device case.  lib: an `experiments=` argument of Engine (None = the in-tree library, a path = another build)."""
    import torch
    from tokenhmr_amd.engine import Engine
    from tokenhmr_amd import _cabi
    cfg, tensors, smpl = case_inputs(case)
    wb = host_record(_cabi.load(exp=lib), VIT_DEPTH, DEC_DEPTH, case["head"], MAX_BATCH)["weight_bytes"]
    arena = torch.zeros(wb, dtype=torch.uint8, device=device)

    def digest():
        torch.cuda.synchronize(device)
        return hashlib.sha256(arena.cpu().numpy().tobytes()).hexdigest()

    eng = Engine(cfg, max_batch=MAX_BATCH, device=device, weight_arena=arena, experiments=lib, vit_gemm="f32")      # fp32: no split3 memory
    try:
        eng.load_state(tensors)
        eng.load_smpl(smpl)
        loaded = digest()
        eng.finalize()
        finalized = digest()
        eng.status()
    finally:
        eng.close()
    return {"weight_bytes": wb, "sha256_loaded": loaded, "sha256_finalized": finalized}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="the recorded commit's shipped library (scripts/build_ab_lib.py)")
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--check", action="store_true", help="compare with --out instead of writing it (a second process: the digests must be reproducible)")
    ap.add_argument("--host-only", action="store_true", help="no device: with --check, compare the host part only")
    a = ap.parse_args()
    from tokenhmr_amd import _cabi
    path = os.path.abspath(a.lib)
    lib = _cabi.load(exp=path)
    with open(os.path.join(os.path.dirname(path), "SOURCE")) as f:      # written by build_ab_lib.py: "<sha> (<ref>) <defines>"
        commit = f.read().split()[0]
    info = lib.thmr_build_info().decode()
    src = next(w for w in info.split() if w.startswith("src:"))
    host = [dict(c, **host_record(lib, **c)) for c in HOST_CONFIGS]
    device = []
    if not a.host_only:
        import torch
        dev = torch.device("cuda:0")
        for case in GPU_CASES:
            device.append(dict(case, **run_case(case, dev, path)))
            print(device[-1], flush=True)
    doc = {"what": "thmr_spec / arena sizes per config, and sha256 of the whole weight arena after load and after finalize "
                   "(scripts/gen_golden_arena_layout.py)",
           "commit": commit, "src": src, "vit_depth": VIT_DEPTH, "dec_depth": DEC_DEPTH, "max_batch": MAX_BATCH, "host": host, "device": device}
    if a.check:
        with open(a.out) as f:
            old = json.load(f)
        keys = ("commit", "src", "host") if a.host_only else tuple(doc)
        bad = [k for k in keys if old[k] != doc[k]]
        if bad:
            sys.exit(f"{a.out}: differs in {bad}")
        print(f"{a.out}: reproduced from {commit} ({src})")
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        # one line per config / case: a spec of several hundred names stays one line of the diff
        rows = {k: "[\n" + ",\n".join("  " + json.dumps(r) for r in doc[k]) + "\n ]" for k in ("host", "device")}
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {rows.get(k) or json.dumps(v)}" for k, v in doc.items()) + "\n}\n")
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes) from {commit} ({src})")


if __name__ == "__main__":
    main()
