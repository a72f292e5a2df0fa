"""Record the fixture that pins the tokenizer round trip to the reference:

  tests/golden/tokenizer_rt.npz   what the reference's OWN VanillaTokenizer (tokenization/models/vanilla_pose_vqvae.py:195-255) computes on
                                  the synthetic encoder / decoder weights (weights.make_synthetic_encoder / _tokenizer, seed 0) and a
                                  codebook drawn at the scale of its latents, for make_pose(3, 0) and make_pose(2, 5): code indices, the
                                  latent, the fp64 top-2 distance gaps, commit loss, perplexity, the non-zero code counts, pred_pose_body_6d,
                                  pred_pose_body_rotmat and matrix_to_axis_angle of it — in float32 and from the same modules in float64;
                                  and matrix_to_axis_angle (rotation_utils.py:428-441) on a set of rotations that takes every branch, with
                                  the function's own float32-vs-float64 distance per group.

The synthetic tokenizer's randn codebook (std 1) against latents of std 0.03 makes every token pick ONE code.  This fixture's codebook is
mu + FACTOR * sd * randn(2048, 256; seed 11) with mu / sd the per-dimension statistics of the reference encoder's latents over
make_pose(16, 7): the argmin has dozens of winners.  The 2 MB codebook is not stored: mu, sd, FACTOR, the seed and a checksum are.

The reference's files are executed IN PLACE through oracle.ref_import (nothing of them is copied).  tests/test_tokenizer_rt_host.py imports
this module for its live comparison.

    python scripts/gen_golden_tokenizer_rt.py [--check]
"""
import argparse
import copy
import json
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
GOLDEN = os.path.join(ROOT, "tests", "golden", "tokenizer_rt.npz")

from tokenhmr_amd.config import RELEASE                 # noqa: E402
from tokenhmr_amd import weights as W                   # noqa: E402
from oracle.gen_golden_encode import make_pose          # noqa: E402
import tokenizer_rt_oracle as T                         # noqa: E402

# the arch_params VanillaTokenizer.__init__ reads (:199-231) and that load the synthetic state strictly
ARCH = dict(CODE_DIM=256, NB_CODE=2048, DOWN_T=1, DEPTH=2, WIDTH=512, QUANTIZER="ema_reset", ROT_TYPE="rot6d", DILATION_RATE=3,
            TOKEN_SIZE_MUL=4, TOKEN_SIZE_DIV=4, NB_JOINTS=21)
FACTOR = 2.0                    # codebook spread in units of the latents' sd (0.5 / 1 / 2 compared 70 % / 88 % / 94 % of the tokens)
CB_SEED = 11
STAT_POSES = (16, 7)            # make_pose(B, seed) behind mu / sd
BATCHES = (("b3", 3, 0), ("b2", 2, 5))
GAP = 1e-5                      # a token is compared where its fp64 top-2 distance gap exceeds this
RANDOM_ROTATIONS = (4096, 21)   # count, seed
ABOVE_PI = math.pi + 1e-3       # the threshold of the fixture's "angle above pi" count


def reference_tokenizer(codebook, dtype=torch.float32):
    """The reference's VanillaTokenizer with the synthetic weights and `codebook`, load_state_dict(strict=True)-ed, in eval mode."""
    from oracle import ref_import
    ns = ref_import.load()
    net = ns.vqvae.VanillaTokenizer(types.SimpleNamespace(**ARCH), mesh_inference=False)
    sd = dict(W.make_synthetic_encoder(RELEASE, 0))
    sd.update(W.make_synthetic_tokenizer(RELEASE, 0))
    sd["quantizer.codebook"] = codebook
    net.load_state_dict(sd, strict=True)
    return net.to(dtype).eval()


def latent_statistics():
    """Per-dimension mean and standard deviation of the reference encoder's latents (the codebook value does not enter)."""
    net = reference_tokenizer(torch.zeros(2048, 256))
    with torch.no_grad():
        lat = net.quantizer.preprocess(net.encoder(make_pose(*STAT_POSES)))
    return lat.mean(0), lat.std(0)


def run_reference(net, pose):
    """forward (:244-255) plus what it does not return: the latent and the indices, by the same sub-modules; the axis-angle by the
    reference's matrix_to_axis_angle as PoseSPDecoderV1 calls it with mesh_inference (:183)."""
    from oracle import ref_import
    ns = ref_import.load()
    B = pose.shape[0]
    with torch.no_grad():
        output, loss, perplexity = net(pose)
        lat = net.quantizer.preprocess(net.encoder(pose))
        idx = net.quantizer.quantize(lat)
        rot = output["pred_pose_body_rotmat"]
        aa = ns.rotation_utils.matrix_to_axis_angle(rot.reshape(-1, 3, 3)).view(B, 63)
    return dict(idx=idx.view(B, 160), latent=lat.view(B, 160, -1), commit_loss=loss, perplexity=perplexity,
                pose6d=output["pred_pose_body_6d"].contiguous(), rotmat=rot, aa=aa)


def fp64_gaps(lat64, cb64):
    d = (lat64 ** 2).sum(-1, keepdim=True) - 2 * lat64 @ cb64.t() + (cb64 ** 2).sum(-1)[None]
    two = d.topk(2, dim=-1, largest=False)
    return two.indices[:, 0], two.values[:, 1] - two.values[:, 0]


# ------------------------------------------------------------------------------------------------ the rotation branch set
def _axis_rotation(axis, angle):
    """Rodrigues in float64 -> float32 bits (stored in the fixture: libm enters here)."""
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    R = torch.eye(3, dtype=torch.float64) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)
    return R.float()


def special_rotations():
    """(R (n,3,3) float32, {group: [start, end)}) — every branch of matrix_to_axis_angle."""
    X, Y, Z = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
    groups = [
        ("identity", [torch.eye(3)]),
        ("angle_1e-7", [_axis_rotation(a, 1e-7) for a in (X, Y, Z)]),                     # |angle| < 1e-6: the 0.5 - angle^2 / 48 branch
        ("angle_1e-3", [_axis_rotation(a, 1e-3) for a in (X, Y, Z)]),
        ("angle_pi-1e-3", [_axis_rotation(a, math.pi - 1e-3) for a in (X, Y, Z)]),
        ("angle_pi", [_axis_rotation(a, math.pi) for a in (X, Y, Z)] + [torch.diag(torch.tensor(d)) for d in
                                                                      ((1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0))]),
        # one case per quaternion candidate as the argmax winner: r (small angle), then i / j / k (an angle near pi about that axis)
        ("winner", [_axis_rotation((1.0, 2.0, 3.0), 0.5), _axis_rotation((0.9, 0.3, 0.3), 3.0), _axis_rotation((0.3, 0.9, 0.3), 3.0),
                    _axis_rotation((0.3, 0.3, 0.9), 3.0), _axis_rotation((0.9, 0.3, 0.3), -3.0), _axis_rotation((0.3, 0.9, -0.3), 3.1)]),
        # exact ties of q_abs: pi about a face diagonal (two-way), 120 degrees about the cube diagonal (four-way), 90 degrees about an axis
        ("tie", [torch.tensor(m) for m in ([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]], [[0.0, 0.0, 1.0], [0.0, -1.0, 0.0], [1.0, 0.0, 0.0]],
                                           [[-1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]], [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]],
                                           [[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]], [[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])]),
    ]
    mats, spans, n = [], {}, 0
    for name, ms in groups:
        spans[name] = [n, n + len(ms)]
        n += len(ms)
        mats += [m.float() for m in ms]
    return torch.stack(mats), spans


def random_rotations(n=RANDOM_ROTATIONS[0], seed=RANDOM_ROTATIONS[1]):
    """Unit quaternions -> matrices in float64 with +, -, *, / and sqrt only (IEEE-exact: the same bits on every machine), as float32."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(n, 4, generator=g, dtype=torch.float64)
    r, i, j, k = q.unbind(-1)
    nrm = torch.sqrt(((r * r + i * i) + j * j) + k * k)
    r, i, j, k = r / nrm, i / nrm, j / nrm, k / nrm
    R = torch.stack([1 - 2 * (j * j + k * k), 2 * (i * j - k * r), 2 * (i * k + j * r),
                     2 * (i * j + k * r), 1 - 2 * (i * i + k * k), 2 * (j * k - i * r),
                     2 * (i * k - j * r), 2 * (j * k + i * r), 1 - 2 * (i * i + j * j)], dim=-1)
    return R.view(n, 3, 3).float()


def rotation_checksum(R):
    return float((R.double().reshape(-1) * (1.0 + (torch.arange(R.numel()) % 7).double())).sum())


def rotation_set(special=None):
    special_R, spans = special_rotations()
    if special is not None:
        special_R = special
    R = torch.cat([special_R, random_rotations()], 0)
    spans = dict(spans)
    spans["random"] = [special_R.shape[0], R.shape[0]]
    return R, spans


def generate():
    from oracle import ref_import
    ns = ref_import.load()
    g = {"arch": np.array(json.dumps(ARCH)), "factor": np.array([FACTOR]), "cb_seed": np.array([CB_SEED]), "gap": np.array([GAP]),
         "batches": np.array(json.dumps([list(b) for b in BATCHES])), "stat_poses": np.array(STAT_POSES)}
    mu, sd = latent_statistics()
    cb = T.make_codebook(mu, sd, FACTOR, CB_SEED)
    g["mu"], g["sd"] = mu.numpy(), sd.numpy()
    g["cb_checksum"] = np.array([W.checksum({"cb": cb})], dtype=np.float64)
    g["enc_checksum"] = np.array([W.checksum(W.make_synthetic_encoder(RELEASE, 0))], dtype=np.float64)
    g["dec_checksum"] = np.array([W.checksum(W.make_synthetic_tokenizer(RELEASE, 0))], dtype=np.float64)
    net32 = reference_tokenizer(cb)
    net64 = copy.deepcopy(net32).double()
    for tag, B, seed in BATCHES:
        pose = make_pose(B, seed)
        r32, r64 = run_reference(net32, pose), run_reference(net64, pose.double())
        idx64, gap = fp64_gaps(r64["latent"].view(-1, 256), cb.double())
        assert torch.equal(idx64.view(B, 160), r64["idx"])
        share = float((gap > GAP).double().mean())
        same = bool(torch.equal(r32["idx"], r64["idx"]))
        counts = torch.bincount(r32["idx"].reshape(-1), minlength=2048)
        nz = counts.nonzero().reshape(-1)
        print(f"[{tag}] {nz.numel()} distinct codes of {B * 160}, perplexity {float(r32['perplexity']):.4f}, commit {float(r32['commit_loss']):.4e}, "
              f"fp64 gap > {GAP:g} on {100 * share:.1f} % of the tokens, fp32 indices == fp64 indices: {same}")
        assert share >= 0.90, "raise FACTOR: fewer than 90 % of the tokens would be compared"
        g[f"{tag}.idx"] = r32["idx"].numpy().astype(np.int32)
        g[f"{tag}.idx64"] = r64["idx"].numpy().astype(np.int32)
        g[f"{tag}.gap64"] = gap.numpy()
        g[f"{tag}.latent_sample"] = r32["latent"].view(-1, 256)[::7].numpy()
        if tag == "b2":
            g[f"{tag}.latent"] = r32["latent"].numpy()          # the whole latent of the small batch: the statistics kernel's input
        g[f"{tag}.code_ids"] = nz.numpy().astype(np.int32)
        g[f"{tag}.code_counts"] = counts[nz].numpy().astype(np.int32)
        dist = []
        for k in ("commit_loss", "perplexity", "pose6d", "rotmat", "aa"):
            g[f"{tag}.{k}"] = r32[k].numpy().astype(np.float32)
            g[f"{tag}.{k}.f64"] = r64[k].numpy().astype(np.float64)
            dist.append(float((r32[k].double() - r64[k]).abs().max()))
        g[f"{tag}.ref32_vs_f64"] = np.array(dist, dtype=np.float64)
        print(f"[{tag}] reference fp32 vs the same modules in fp64: commit {dist[0]:.2e}, perplexity {dist[1]:.2e}, 6d {dist[2]:.2e}, "
              f"rotmat {dist[3]:.2e}, aa {dist[4]:.2e}")
    # matrix_to_axis_angle on the branch set
    R, spans = rotation_set()
    special_n = spans["random"][0]
    with torch.no_grad():
        aa32 = ns.rotation_utils.matrix_to_axis_angle(R)
        aa64 = ns.rotation_utils.matrix_to_axis_angle(R.double())
    winner, q0 = T.quaternion_of(R)
    for name, want in zip(("winner",) * 4, range(4)):
        assert int(winner[spans["winner"][0] + want]) == want, "the winner group no longer has one case per candidate"
    assert sorted(set(winner.tolist())) == [0, 1, 2, 3]
    dist = {name: float((aa32[a:b].double() - aa64[a:b]).abs().max()) for name, (a, b) in spans.items()}
    g["rot.special"] = R[:special_n].numpy()
    g["rot.spans"] = np.array(json.dumps(spans))
    g["rot.random"] = np.array(RANDOM_ROTATIONS)
    g["rot.random_checksum"] = np.array([rotation_checksum(R[special_n:])], dtype=np.float64)
    g["rot.aa"] = aa32.numpy()
    g["rot.aa.f64"] = aa64.numpy()
    g["rot.winner"] = winner.numpy().astype(np.int8)
    g["rot.q0_negative"] = np.array([int((q0 < 0).sum())])
    # angles the reference leaves above pi (no standardisation), counted clear of pi itself: the exactly-pi cases sit within an ulp of it
    ang = aa32.norm(dim=-1)
    assert ((ang - ABOVE_PI).abs() > 1e-5).all()
    g["rot.angle_above_pi"] = np.array([int((ang > ABOVE_PI).sum())])
    g["rot.ref32_vs_f64"] = np.array(json.dumps(dist))
    print(f"[rotations] {R.shape[0]} matrices, winners {torch.bincount(winner, minlength=4).tolist()}, q0 < 0 on {int((q0 < 0).sum())}, "
          f"angle > pi + 1e-3 on {int(g['rot.angle_above_pi'][0])}; matrix_to_axis_angle fp32 vs fp64 per group: "
          + ", ".join(f"{k} {v:.2e}" for k, v in dist.items()))
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed fixture instead of writing it")
    args = ap.parse_args()
    g = generate()
    if args.check:
        old = np.load(GOLDEN)
        bad = [k for k in g if k not in old or not np.array_equal(np.asarray(g[k]), old[k])]
        print("fixture matches" if not bad else f"DIFFERS: {bad}")
        sys.exit(1 if bad else 0)
    np.savez_compressed(GOLDEN, **g)
    print(f"wrote {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
