"""The discriminator's forward, and forward + value + input gradient, next to the same chain in torch ops under torch autograd with the
same weights, on one box, in one process, interleaved (profiles/discriminator.jsonl).  Needs a GPU; reads nothing outside the repository.

At 1, 8, 64 and 256 items, ms per call between device events around `iters` back-to-back calls; the arms alternate, `reps` windows each,
the order reversed every other repetition, one untimed call after each switch:

  fwd           Discriminator.__call__ without grad: thmr_disc_forward (four launches)
  vg            Discriminator.value_and_grad: out, loss_adv and its gradient by poses and betas, one thmr_disc_backward call (nine launches)
  vg_graph      the same call captured in a torch.cuda.graph and replayed
  torch_fwd     the reference's arithmetic in torch ops on the device (tests/discriminator_oracle.forward), no grad
  torch_vg      the same under torch autograd: out, loss_adv, torch.autograd.grad by poses and betas

and, at 64 items, ValidationLoss.value_and_grad with a body model without and with the discriminator (`loss_vg`, `loss_vg_adv`): what the
opt-in adds.  Nothing is tuned per arm; no number is a target.

    python scripts/disc_bench.py [--reps 7] [--iters 20] [--out profiles/discriminator.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def interleaved(arms, reps, iters):
    """{name: [ms per call of each window]}: the arms alternate, the order reversed every other repetition."""
    import torch
    ms = {k: [] for k in arms}
    for f in arms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    names = list(arms)
    for rep in range(reps):
        for name in (names if rep % 2 == 0 else names[::-1]):
            f = arms[name]
            f()                                                     # one untimed call after the switch
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / iters)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 8, 64, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "discriminator.jsonl"))
    a = ap.parse_args()

    import numpy as np
    import torch
    import discriminator_oracle as DO
    from tokenhmr_amd import weights as W
    from tokenhmr_amd.discriminator import Discriminator

    if not torch.cuda.is_available():
        sys.exit("disc_bench: needs a GPU (no CPU fallback, no CPU timing)")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    sd = W.make_synthetic_discriminator(0)
    D = Discriminator(dev).load_state_dict(sd)
    build = D.lib.thmr_build_info().decode()
    sd_dev = {k: v.to(dev) for k, v in sd.items()}

    def record(rec, ms):
        med = {k: statistics.median(v) for k, v in ms.items()}
        rec.update({"build": build, "reps": a.reps, "iters_per_window": a.iters, "gpu": torch.cuda.get_device_name(0),
                    "ms_median": {k: round(v, 4) for k, v in med.items()},
                    "ms_spread": {k: round((max(v) - min(v)) / 2, 4) for k, v in ms.items()},
                    "ms_windows": {k: [round(x, 4) for x in v] for k, v in ms.items()}})
        return med

    for B in a.sizes:
        inp = DO.make_inputs(B, 6000)
        poses, betas = torch.from_numpy(inp["poses"]).to(dev), torch.from_numpy(inp["betas"]).to(dev)
        bufs = {"out": torch.empty(B, 25, device=dev), "loss": torch.empty((), device=dev), "chunk_loss": torch.empty((), device=dev),
                "grad_poses": torch.empty(B, 23, 3, 3, device=dev), "grad_betas": torch.empty(B, 10, device=dev)}
        leaves = [poses.clone().requires_grad_(True), betas.clone().requires_grad_(True)]

        def fwd():
            with torch.no_grad():
                return D(poses, betas)

        def vg():
            return D.value_and_grad(poses, betas, target=1.0, bufs=bufs)

        def torch_fwd():
            with torch.no_grad():
                return DO.forward(sd_dev, poses, betas)

        def torch_vg():
            out = DO.forward(sd_dev, *leaves)
            loss = DO.loss(out, 1.0)
            return out, loss, torch.autograd.grad(loss, leaves)

        arms = {"fwd": fwd, "vg": vg, "torch_fwd": torch_fwd, "torch_vg": torch_vg}
        vg()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            vg()
        arms["vg_graph"] = graph.replay
        # the two chains compute the same thing (a check, not a tolerance test: tests/test_gpu_discriminator.py holds the bound)
        (o, l, gp, gb), (to, tl, (tgp, tgb)) = vg(), torch_vg()
        agree = {"out": float((o - to.detach()).abs().max() / to.detach().abs().max()), "loss": float((l - tl.detach()).abs() / tl.detach().abs()),
                 "grad": max(float((gp - tgp).abs().max() / tgp.abs().max()), float((gb - tgb).abs().max() / tgb.abs().max()))}
        ms = interleaved(arms, a.reps, a.iters)
        rec = {"what": "discriminator forward / value and input gradient, ms per call between device events, arms interleaved", "items": B}
        med = record(rec, ms)
        rec.update({"torch_fwd_over_fwd": round(med["torch_fwd"] / med["fwd"], 2), "torch_vg_over_vg": round(med["torch_vg"] / med["vg"], 2),
                    "torch_vg_over_vg_graph": round(med["torch_vg"] / med["vg_graph"], 2), "chains_max_rel_diff": agree})
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps({k: v for k, v in rec.items() if k != "ms_windows"}), flush=True)
        del graph

    # what the opt-in adds to value_and_grad, at 64 items
    import gen_golden_val_loss as GV
    import gen_golden_val_loss_grad as GG
    from tokenhmr_amd.losses import ValidationLoss
    from tokenhmr_amd.model import ConfigNode
    from tokenhmr_amd.smpl import SMPL
    from tokenhmr_amd.smpl_assets import make_synthetic_smpl
    B = 64
    g = np.load(os.path.join(ROOT, "tests", "golden", "val_loss_grad.npz"))
    th = {k[7:]: g[k] for k in g.files if k.startswith("thresh.")}
    m = SMPL(make_synthetic_smpl(seed=0), max_batch=B, device=dev).enable_grad()
    inp = GG.make_inputs(B, 6000 + B, thresholds=th)
    batch, output = GV.to_batch(inp, torch.float32)
    flags = batch.pop("smpl_params_is_axis_angle")
    mv = lambda d: {k: (mv(v) if isinstance(v, dict) else v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}      # noqa: E731
    batch, output = mv(batch), mv(output)
    batch["smpl_params_is_axis_angle"] = flags
    output["pred_cam"] = torch.from_numpy(inp["pred_cam"]).to(dev)
    cfg = ConfigNode({"MODEL": {"LOOSE_SUP": False, "LOOSE_WEIGHT": GV.LOOSE_WEIGHT}, "LOSS_WEIGHTS": dict(GV.LOSS_WEIGHTS, ADVERSARIAL=0.0005)})
    vl = ValidationLoss(cfg)
    kw = dict(body_model=m, focal_length=GG.FOCAL_LENGTH, image_size=GG.IMAGE_SIZE)
    arms = {"loss_vg": lambda: vl.value_and_grad(batch, output, **kw), "loss_vg_adv": lambda: vl.value_and_grad(batch, output, discriminator=D, **kw)}
    ms = interleaved(arms, a.reps, a.iters)
    rec = {"what": "ValidationLoss.value_and_grad with a body model, without and with the discriminator (w = 0.0005), ms per call, arms interleaved",
           "items": B}
    med = record(rec, ms)
    rec["adversarial_term_adds_ms"] = round(med["loss_vg_adv"] - med["loss_vg"], 4)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps({k: v for k, v in rec.items() if k != "ms_windows"}), flush=True)
    m.close()


if __name__ == "__main__":
    main()
