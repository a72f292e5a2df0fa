"""TEST INFRASTRUCTURE ONLY — CPU restatement of the tokenizer round trip the reference evaluates.

    VanillaTokenizer.forward            tokenization/models/vanilla_pose_vqvae.py:244-255
    QuantizeEMAReset.forward (eval)     tokenization/models/quantize_cnn.py:95-130 (perplexity :38-47, commit :121, straight-through :124)
    PoseSPDecoderV1.forward             vanilla_pose_vqvae.py:161-193 (rotation_6d_to_matrix :173, matrix_to_axis_angle :183)
    matrix_to_axis_angle                tokenization/models/rotation_utils.py:428-441 (:104-163 matrix_to_quaternion, :478-506)

The encoder, the quantiser's argmin and the decoder stack are oracle/tokenhmr_oracle.py's, by import.  Pinned by
tests/test_tokenizer_rt_host.py to tests/golden/tokenizer_rt.npz (written by scripts/gen_golden_tokenizer_rt.py from the reference's own
VanillaTokenizer) and, where the reference tree exists, to those classes live.  Every function works in float32 or float64 (the dtype
of its inputs)."""
import torch
import torch.nn.functional as F

from oracle import tokenhmr_oracle as O
from tokenhmr_amd.config import HMRConfig, RELEASE


def make_codebook(mu, sd, factor, seed, nb_code=2048):
    """The fixture's codebook, regenerated from what the fixture stores: mu + factor * sd * randn(nb_code, 256; seed) — codes at the
    scale of the encoder's latents, so that the argmin has many winners (the synthetic randn codebook of std 1 has one)."""
    g = torch.Generator().manual_seed(int(seed))
    z = torch.randn(nb_code, mu.numel(), generator=g, dtype=torch.float32)
    return mu.float() + float(factor) * sd.float() * z


def straight_through(x, codebook, idx):
    """quantize_cnn.py:124: x + (x_d - x), in that order — NOT x_d: an ulp away on some elements."""
    c = codebook[idx.long()]
    return x + (c - x)


def quantizer_stats(x, codebook, idx, counts=None):
    """(commit_loss, perplexity, code_count): quantize_cnn.py:121 F.mse_loss(x, x_d) and :38-47.  `counts`: a histogram to add this
    batch's to first (the chunked facade); the perplexity is that of the sum."""
    idx = idx.long()
    commit = F.mse_loss(x, codebook[idx])
    c = torch.bincount(idx, minlength=codebook.shape[0])
    if counts is not None:
        c = c + counts
    prob = c.to(x.dtype) / c.sum().to(x.dtype)
    perplexity = torch.exp(-torch.sum(prob * torch.log(prob + 1e-7)))
    return commit, perplexity, c


def decode_features(feat, tok, cfg: HMRConfig = RELEASE):
    """PoseSPDecoderV1 on dequantised features (B,160,256) -> (B,21,6): oracle.vq_decode with an identity codebook, so that its
    `probs @ codebook` hands `feat` through unchanged (one non-zero term per element: exact)."""
    t = dict(tok)
    t["quantizer.codebook"] = torch.eye(feat.shape[-1], dtype=feat.dtype)
    return O.vq_decode(feat, t, cfg)


def decode_indices(idx, tok, cfg: HMRConfig = RELEASE):
    """VanillaTokenizer.decode / DecodeTokens on hard indices: the code rows themselves (quantize_cnn.py:88-90)."""
    B = idx.shape[0]
    return decode_features(tok["quantizer.codebook"][idx.long().reshape(-1)].view(B, 160, -1), tok, cfg)


def matrix_to_axis_angle(matrix):
    """rotation_utils.py:428-441, the route of the reference step by step, dtype-generic.  (n,3,3) or (...,3,3) -> (...,3)."""
    lead = matrix.shape[:-2]
    m = matrix.reshape(-1, 9)
    tiny = torch.finfo(m.dtype).tiny
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m.unbind(-1)
    sq = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], dim=-1)
    q_abs = torch.where(sq > 0, torch.sqrt(sq.clamp(min=0)), torch.zeros_like(sq))                # _sqrt_positive_part, :92-101
    rows = torch.stack([torch.stack([q_abs[:, 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=-1),
                        torch.stack([m21 - m12, q_abs[:, 1] ** 2, m10 + m01, m02 + m20], dim=-1),
                        torch.stack([m02 - m20, m10 + m01, q_abs[:, 2] ** 2, m12 + m21], dim=-1),
                        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[:, 3] ** 2], dim=-1)], dim=-2)
    floor = torch.tensor(0.1, dtype=m.dtype)
    cand = rows / (2.0 * q_abs[..., None].max(floor)).clamp(min=tiny)                              # :155-156
    q = cand[torch.arange(m.shape[0]), q_abs.argmax(dim=-1)]                                       # :161-163, no standardisation
    norms = torch.linalg.norm(q[:, 1:], ord=2, dim=-1, keepdim=True)                               # :492
    half = torch.atan2(norms, q[:, :1])
    angles = 2 * half
    small = angles.abs() < 1e-6
    safe = torch.where(small, torch.ones_like(angles), angles)
    s = torch.where(small, 0.5 - (angles * angles) / 48, torch.sin(half) / safe)                   # :497-505
    return (q[:, 1:] / s.clamp(min=tiny)).reshape(lead + (3,))                                     # :506 safe_zero_division


def quaternion_of(matrix):
    """The quaternion matrix_to_axis_angle goes through (for the fixture's q0 < 0 count)."""
    m = matrix.reshape(-1, 9)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m.unbind(-1)
    sq = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], dim=-1)
    q_abs = torch.where(sq > 0, torch.sqrt(sq.clamp(min=0)), torch.zeros_like(sq))
    w = q_abs.argmax(dim=-1)
    first = torch.stack([q_abs[:, 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=-1)
    q0 = first[torch.arange(m.shape[0]), w] / (2.0 * q_abs.max(dim=-1).values.clamp(min=0.1))
    return w, q0


def roundtrip(pose6d, enc, tok, cfg: HMRConfig = RELEASE, latent=None, idx=None, want_aa=True):
    """VanillaTokenizer.forward on (B,21,6).  `latent` / `idx` given: the quantiser and decoder on those instead of this function's
    own (the GPU test feeds the device's latent and indices, so that near-tie flips do not enter the pose comparison)."""
    B = pose6d.shape[0]
    cb = tok["quantizer.codebook"]
    oidx, olat, dist = O.vq_encode(pose6d, enc, cb)
    lat = olat if latent is None else latent.reshape(-1, cb.shape[1])
    ix = oidx if idx is None else idx.reshape(-1).long()
    commit, perplexity, counts = quantizer_stats(lat, cb, ix)
    pose = decode_features(straight_through(lat, cb, ix).view(B, 160, -1), tok, cfg)
    rot = O.rot6d_to_rotmat(pose.reshape(-1, 6)).view(B, 21, 3, 3)
    out = dict(idx=ix.view(B, 160), latent=lat.view(B, 160, -1), dist=dist, commit_loss=commit, perplexity=perplexity, code_count=counts,
               pose6d=pose, rotmat=rot)
    if want_aa:
        out["aa"] = matrix_to_axis_angle(rot.view(-1, 3, 3)).view(B, 63)
    return out
