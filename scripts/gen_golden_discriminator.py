"""Writes tests/golden/discriminator.npz: the reference's own Discriminator (tokenhmr/lib/models/discriminator.py:4-99) executed IN PLACE
on the CPU in float32 and in float64 under torch autograd, on seeded inputs (B = 8) and the seeded synthetic weights
(tokenhmr_amd.weights.make_synthetic_discriminator, loaded with load_state_dict(strict=True)).

Nothing of the reference is copied: discriminator.py and geometry.py (aa_to_rotmat of the real branch, tokenhmr.py:357) are loaded by path.
Recorded per precision: out (B,25); loss_adv (tokenhmr.py:392-393), loss_fake, loss_real, loss_disc (:357-362); the autograd gradients of
loss_adv by poses and betas; those of sum(out * grad_out) for a random grad_out.  Also: the inputs, and the leading values of every weight
tensor, so that a drift of the seeded weights is detected — the weights themselves (7.2 MB) are regenerated from the seed by both sides.
The seed is accepted only under tests/discriminator_oracle.accept(): no ReLU pre-activation close enough to 0 for a precision to flip it.

    python scripts/gen_golden_discriminator.py [--check]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import discriminator_oracle as DO          # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "discriminator.npz")
LEAD = 8                                   # leading values kept of each weight tensor


def load_reference():
    """(the reference's Discriminator class, its aa_to_rotmat), loaded by path."""
    from oracle import ref_import
    if not ref_import.available():
        raise RuntimeError(f"reference tree not found at {ref_import.REF}")
    lib = os.path.join(ref_import.REF, "tokenhmr", "lib")
    disc = sys.modules.get("_ref_discriminator") or ref_import._load("_ref_discriminator", os.path.join(lib, "models", "discriminator.py"))
    geo = sys.modules.get("_ref_geometry") or ref_import._load("_ref_geometry", os.path.join(lib, "utils", "geometry.py"))
    return disc.Discriminator, geo.aa_to_rotmat


def reference_module(dtype, seed=DO.WEIGHT_SEED):
    from tokenhmr_amd.weights import make_synthetic_discriminator
    D = load_reference()[0]().to(dtype)
    D.load_state_dict({k: v.to(dtype) for k, v in make_synthetic_discriminator(seed).items()}, strict=True)
    return D.eval()


def run_reference(inp, dtype):
    """What tests/discriminator_oracle.run returns, computed by the reference's class."""
    D, aa_to_rotmat = reference_module(dtype), load_reference()[1]
    T = lambda k: torch.from_numpy(inp[k]).to(dtype)      # noqa: E731
    B = inp["betas"].shape[0]
    poses, betas = T("poses").requires_grad_(True), T("betas").requires_grad_(True)
    out = D(poses, betas)
    loss_adv = ((out - 1.0) ** 2).sum() / B
    gp, gb = torch.autograd.grad(loss_adv, (poses, betas), retain_graph=True)
    vp, vb = torch.autograd.grad((out * T("grad_out")).sum(), (poses, betas))
    with torch.no_grad():
        gt_rotmat = aa_to_rotmat(T("gt_body_pose_aa").view(-1, 3)).view(B, -1, 3, 3)
        loss_fake = ((D(poses.detach(), betas.detach()) - 0.0) ** 2).sum() / B
        loss_real = ((D(gt_rotmat, T("gt_betas")) - 1.0) ** 2).sum() / B
    r = {"out": out, "loss_adv": loss_adv, "loss_fake": loss_fake, "loss_real": loss_real, "loss_disc": loss_fake + loss_real,
         "grad_poses": gp, "grad_betas": gb, "vjp_poses": vp, "vjp_betas": vb}
    return {k: v.detach().numpy() for k, v in r.items()}


def compute(verbose=True):
    from tokenhmr_amd.weights import make_synthetic_discriminator
    inp = DO.make_inputs(DO.BATCH, DO.SEED)
    ratio = DO.accept(inp)
    out = {"in." + k: v for k, v in inp.items()}
    for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        for k, v in run_reference(inp, dtype).items():
            out[f"{name}.{k}"] = v
    for k, v in make_synthetic_discriminator(DO.WEIGHT_SEED).items():
        out["w." + k] = v.reshape(-1)[:LEAD].numpy()
    if verbose:
        print(f"seed {DO.SEED}, B = {DO.BATCH}: smallest ReLU margin ratio {ratio:.1f}; loss_adv {out['f64.loss_adv']:.6f}, "
              f"loss_disc {out['f64.loss_disc']:.6f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed fixture instead of writing it")
    args = ap.parse_args()
    new = compute()
    if args.check:
        old = np.load(OUT)
        assert set(old.files) == set(new), set(old.files) ^ set(new)
        for k, v in new.items():
            assert old[k].dtype == v.dtype and np.array_equal(old[k], v), k
        print("discriminator.npz: the reference reproduces the committed fixture bit for bit")
        return
    np.savez_compressed(OUT, **new)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
