"""A torch restatement of the reference's Discriminator (tokenhmr/lib/models/discriminator.py:52-99) and of the three losses tokenhmr.py
builds on it (:357-362, :392-394), in any dtype, for the tests of thmr_disc_forward / thmr_disc_backward where the
reference tree is absent.  Pinned to the reference's own record (tests/golden/discriminator.npz, both precisions) and, where the tree
exists, to the live class in tests/test_discriminator_host.py.  Also: the seeded inputs of the fixture and of every GPU test shape, and the
rule a seed is accepted by.  A plain module: no fixtures, no pytest hooks."""
import numpy as np
import torch

SEED, BATCH = 1000, 8                                      # the fixture
# tests/test_gpu_discriminator.py: each side of a 16-row MFMA tile and of the skinny GEMM's 64-row block, a B that is no multiple of 4.
# The seed of each: the first from 1000 up that accept() takes with a ratio of at least 8 — twice the rule's 4, because the device may be
# twice as far from float64 as float32 torch is (with 64 x 1024 pre-activations per wide layer several seeds fail the rule itself).
GPU_SEED = {1: 1000, 3: 1000, 8: 1000, 17: 1007, 64: 1012, 65: 1004}
GPU_BATCHES = tuple(GPU_SEED)
WEIGHT_SEED = 0
RELU_LAYERS = ("conv1", "conv2", "betas_fc1", "betas_fc2", "fc1", "fc2")
MARGIN = 4.0                                               # scripts/gen_golden_val_loss.py's factor for its thresholds


def aa_to_rotmat(aa):
    """Rodrigues in the dtype of aa (n,3) -> (n,3,3); the tests' own (float64 for the inputs)."""
    th = aa.norm(dim=1, keepdim=True).clamp_min(1e-12)
    k = aa / th
    K = torch.zeros(aa.shape[0], 3, 3, dtype=aa.dtype)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return torch.eye(3, dtype=aa.dtype) + torch.sin(th)[..., None] * K + (1 - torch.cos(th))[..., None] * (K @ K)


def make_inputs(B, seed):
    """Seeded float32 inputs: 'poses' (B,23,3,3) rotations of about 0.5 rad, 'betas' (B,10), the mocap batch 'gt_body_pose_aa' (B,69) and
    'gt_betas' (B,10), and 'grad_out' (B,25), a random cotangent."""
    g = torch.Generator().manual_seed(seed * 100 + B)
    aa = 0.5 * torch.randn(B * 23, 3, generator=g, dtype=torch.float64)
    return {"poses": aa_to_rotmat(aa).reshape(B, 23, 3, 3).float().numpy(), "betas": torch.randn(B, 10, generator=g).numpy(),
            "gt_body_pose_aa": (0.5 * torch.randn(B, 69, generator=g)).numpy(), "gt_betas": torch.randn(B, 10, generator=g).numpy(),
            "grad_out": torch.randn(B, 25, generator=g).numpy()}


def weights(dtype=torch.float32, seed=WEIGHT_SEED):
    from tokenhmr_amd.weights import make_synthetic_discriminator
    return {k: v.to(dtype) for k, v in make_synthetic_discriminator(seed).items()}


def forward(sd, poses, betas, taps=None):
    """-> (B,25).  taps: a dict that receives the six ReLU layers' pre-activations."""
    lin = torch.nn.functional.linear
    B = betas.shape[0]
    t = taps if taps is not None else {}
    x = poses.reshape(B, 23, 9)
    t["conv1"] = lin(x, sd["D_conv1.weight"].reshape(32, 9), sd["D_conv1.bias"])                   # (B,23,32): joint, channel
    t["conv2"] = lin(t["conv1"].relu(), sd["D_conv2.weight"].reshape(32, 32), sd["D_conv2.bias"])
    h = t["conv2"].relu()
    heads = torch.stack([lin(h[:, j], sd[f"pose_out.{j}.weight"], sd[f"pose_out.{j}.bias"])[:, 0] for j in range(23)], 1)
    t["betas_fc1"] = lin(betas, sd["betas_fc1.weight"], sd["betas_fc1.bias"])
    t["betas_fc2"] = lin(t["betas_fc1"].relu(), sd["betas_fc2.weight"], sd["betas_fc2.bias"])
    shape = lin(t["betas_fc2"].relu(), sd["betas_out.weight"], sd["betas_out.bias"])
    flat = h.permute(0, 2, 1).reshape(B, 736)                                                      # channel-major: c * 23 + j
    t["fc1"] = lin(flat, sd["D_alljoints_fc1.weight"], sd["D_alljoints_fc1.bias"])
    t["fc2"] = lin(t["fc1"].relu(), sd["D_alljoints_fc2.weight"], sd["D_alljoints_fc2.bias"])
    alljoints = lin(t["fc2"].relu(), sd["D_alljoints_out.weight"], sd["D_alljoints_out.bias"])
    return torch.cat([heads, shape, alljoints], 1)


def loss(out, target):
    return ((out - target) ** 2).sum() / out.shape[0]


def run(inp, dtype, sd=None, rotmat_of=None):
    """Everything the fixture records, in `dtype`: out, the four losses, the autograd gradients of loss_adv by poses and betas, and of
    sum(out * grad_out).  rotmat_of: the real branch's aa_to_rotmat (default: the Rodrigues above)."""
    sd = sd if sd is not None else weights(dtype)
    T = lambda k: torch.from_numpy(inp[k]).to(dtype)      # noqa: E731
    poses, betas = T("poses").requires_grad_(True), T("betas").requires_grad_(True)
    out = forward(sd, poses, betas)
    loss_adv = loss(out, 1.0)
    gp, gb = torch.autograd.grad(loss_adv, (poses, betas), retain_graph=True)
    vp, vb = torch.autograd.grad((out * T("grad_out")).sum(), (poses, betas))
    with torch.no_grad():
        real = (rotmat_of or aa_to_rotmat)(T("gt_body_pose_aa").reshape(-1, 3)).reshape(-1, 23, 3, 3)
        loss_fake, loss_real = loss(out, 0.0), loss(forward(sd, real, T("gt_betas")), 1.0)
    r = {"out": out, "loss_adv": loss_adv, "loss_fake": loss_fake, "loss_real": loss_real, "loss_disc": loss_fake + loss_real,
         "grad_poses": gp, "grad_betas": gb, "vjp_poses": vp, "vjp_betas": vb}
    return {k: v.detach().numpy() for k, v in r.items()}


def relu_margins(inp, seed=WEIGHT_SEED, keys=("poses", "betas")):
    """{layer: (smallest float64 |z|, largest float32-to-float64 distance of z, masks equal)} of the six ReLU layers."""
    t32, t64 = {}, {}
    with torch.no_grad():
        forward(weights(torch.float32, seed), *[torch.from_numpy(inp[k]).float() for k in keys], taps=t32)
        forward(weights(torch.float64, seed), *[torch.from_numpy(inp[k]).double() for k in keys], taps=t64)
    return {k: (t64[k].abs().min().item(), (t32[k].double() - t64[k]).abs().max().item(), bool(((t32[k] > 0) == (t64[k] > 0)).all()))
            for k in RELU_LAYERS}


def accept(inp, seed=WEIGHT_SEED, keys=("poses", "betas")):
    """The rule a seed is accepted by: a ReLU whose pre-activation changes sign between precisions changes a gradient by a whole term, not
    by rounding.  At each of the six ReLU layers the smallest float64 |z| is at least MARGIN x the largest float32-to-float64 distance of
    that layer's pre-activations, and the two masks are equal.  -> the smallest ratio; raises AssertionError otherwise."""
    worst = np.inf
    for k, (lo, d, same) in relu_margins(inp, seed, keys).items():
        assert same, f"{k}: the float32 and the float64 ReLU masks differ"
        assert lo >= MARGIN * d, f"{k}: smallest |z| {lo:.3e} < {MARGIN:g} x the precisions' distance {d:.3e}"
        worst = min(worst, lo / d if d > 0 else np.inf)
    return worst
