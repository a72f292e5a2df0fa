"""The tokenizer round trip next to the sequence it replaces, on one box, in one process, interleaved (profiles/tokenizer_rt.jsonl).

One engine (HMRConfig(vit_depth=1, dec_depth=1): the tokenizer does not depend on the rest), `--poses` poses (default 64), two pairs of
arms, each pair alternating over `reps` windows of `iters` back-to-back calls between device events:

  roundtrip   old: encode_tokens -> a (B,160,2048) one-hot built with torch on the device (zeros + scatter_) -> vq_decode
              new: tokenizer_roundtrip (pose6d only; and with every output: statistics, rotmat, axis-angle)
  decode      old: vq_decode(one_hot), the one-hot already built (its 84 MB are read by the GEMM, not written in the window)
              new: vq_decode_idx(idx)

The new path does strictly less work, so the condition is median(new) <= median(old) + spread(old), the spread being the old arm's own
(max - min) / 2 over its windows.  Before timing, the arms' poses are compared (the hard decode bit for bit with the one-hot decode;
the round trip's straight-through pose to 1e-4, the project's bound for the decoder).

    python scripts/tokenizer_rt_bench.py [--poses 64] [--reps 7] [--iters 20] [--out profiles/tokenizer_rt.jsonl]

Every line written is one JSON record with the library's build id.  Exit status 1 if a condition fails.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    return (max(xs) - min(xs)) / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tokenizer_rt.jsonl"))
    a = ap.parse_args()

    import torch
    from tokenhmr_amd.config import HMRConfig
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    from tokenhmr_amd.engine import Engine

    if not torch.cuda.is_available():
        sys.exit("tokenizer_rt_bench: needs a GPU (no CPU fallback, no CPU timing)")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    failed = False

    def emit(rec):
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)

    cfg = HMRConfig(vit_depth=1, dec_depth=1)
    B = a.poses
    eng = Engine(cfg, max_batch=B, device=dev)
    tok = dict(W.make_synthetic_tokenizer(cfg, 0))
    tok.update(W.make_synthetic_encoder(cfg, 0))
    eng.load_state(W.make_synthetic_state(cfg, 0), tok)
    eng.load_smpl(make_synthetic_smpl(cfg, 0))
    eng.finalize()
    build = eng.lib.thmr_build_info().decode()
    pose = torch.randn(B, 21, 6, generator=torch.Generator().manual_seed(6100)).to(dev)

    def old_roundtrip():
        idx = eng.encode_tokens(pose)
        onehot = torch.zeros(B, 160, 2048, device=dev)
        onehot.scatter_(2, idx.long().unsqueeze(-1), 1.0)
        return eng.vq_decode(onehot)

    all_out = ("idx", "latent", "pose6d", "rotmat", "aa", "commit_loss", "perplexity", "code_count")
    idx0 = eng.encode_tokens(pose)
    onehot0 = torch.zeros(B, 160, 2048, device=dev).scatter_(2, idx0.long().unsqueeze(-1), 1.0)
    arms = {
        "roundtrip": {"old": old_roundtrip, "new": lambda: eng.tokenizer_roundtrip(pose, want=("pose6d",))["pose6d"],
                      "new_all_outputs": lambda: eng.tokenizer_roundtrip(pose, want=all_out)["pose6d"]},
        "decode": {"old": lambda: eng.vq_decode(onehot0), "new": lambda: eng.vq_decode_idx(idx0)},
    }
    # same results first
    d_rt = (arms["roundtrip"]["old"]() - arms["roundtrip"]["new"]()).abs().max().item()
    same_dec = bool(torch.equal(arms["decode"]["old"](), arms["decode"]["new"]()))
    eng.status()
    if d_rt > 1e-4 or not same_dec:
        sys.exit(f"tokenizer_rt_bench: the arms disagree (round trip max|diff| {d_rt:.3e}, hard decode bit-identical: {same_dec})")

    for what, fns in arms.items():
        ms = {k: [] for k in fns}
        for f in fns.values():
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        names = list(fns)
        for rep in range(a.reps):
            for name in (names if rep % 2 == 0 else names[::-1]):
                f = fns[name]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                f()                                                       # one untimed call after the switch
                e0.record()
                for _ in range(a.iters):
                    f()
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1) / a.iters)
        mo, sp = statistics.median(ms["old"]), spread(ms["old"])
        rec = {"what": {"roundtrip": "ms per call: encode_tokens -> torch one-hot -> vq_decode (old) vs tokenizer_roundtrip (new), arms interleaved",
                        "decode": "ms per call: vq_decode(one_hot) (old) vs vq_decode_idx (new), arms interleaved"}[what],
               "build": build, "poses": B, "reps": a.reps, "iters_per_window": a.iters, "gpu": torch.cuda.get_device_name(0),
               "old_spread_ms": round(sp, 4)}
        for name in names:
            rec[f"{name}_ms_windows"] = [round(v, 4) for v in ms[name]]
            rec[f"{name}_ms_median"] = round(statistics.median(ms[name]), 4)
            if name != "old":
                m = statistics.median(ms[name])
                ok = m <= mo + sp
                failed |= not ok
                rec[f"{name}_over_old"] = round(m / mo, 4)
                rec[f"{name}_le_old_within_spread"] = ok
        if what == "roundtrip":
            rec["pose_max_abs_diff_old_vs_new"] = d_rt
        else:
            rec["bit_identical"] = same_dec
        emit(rec)
    eng.status()
    eng.close()
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
