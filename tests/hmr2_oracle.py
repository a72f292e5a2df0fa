"""TEST INFRASTRUCTURE ONLY — CPU restatement of the HMR2.0 regressor head (MODEL.SMPL_HEAD.TYPE: transformer_decoder).

    SMPLTransformerDecoderHead.forward      tokenhmr/lib/models/heads/smpl_head.py:50-104 (IEF_ITERS = 1, zero input token, JOINT_REP 6d)
    TokenHMR.forward_step for that head      tokenhmr/lib/models/tokenhmr.py:135-188 (no 'cls_logits_softmax', :157-158)

The decoder, rot6d_to_rotmat, SMPL and the projection are oracle/tokenhmr_oracle.py's, by import: the two heads share them.  Pinned by
tests/test_hmr2_host.py to tests/golden/hmr2_head.npz (written by scripts/gen_golden_hmr2.py from the reference's own module) and, where
the reference tree exists, to that module live.  Works in float32 or float64 (the dtype of `ctx` / `sd`)."""
import torch
import torch.nn.functional as F

from oracle import tokenhmr_oracle as O
from tokenhmr_amd.config import HMRConfig, RELEASE


def head_forward(ctx, sd, cfg: HMRConfig = RELEASE):
    """smpl_head.py:56-103: token_out -> decpose / decshape / deccam (+ the mean parameters, :82-84) -> rotation matrices (:99)."""
    B = ctx.shape[0]
    token_out = O.decoder_forward(ctx, sd, cfg)                                        # :75-79
    H = "smpl_head."
    pose6d = F.linear(token_out, sd[H + "decpose.weight"], sd[H + "decpose.bias"]) + sd[H + "init_body_pose"]
    betas = F.linear(token_out, sd[H + "decshape.weight"], sd[H + "decshape.bias"]) + sd[H + "init_betas"]
    cam = F.linear(token_out, sd[H + "deccam.weight"], sd[H + "deccam.bias"]) + sd[H + "init_cam"]
    rotmat = O.rot6d_to_rotmat(pose6d).view(B, cfg.n_joints, 3, 3)
    return dict(token_out=token_out, pose6d=pose6d, betas=betas, cam=cam, rotmat=rotmat)


def forward(img, sd, smpl, cfg: HMRConfig = RELEASE, ctx=None):
    """tokenhmr.py:135-188 with the transformer_decoder head.  `ctx`: ViT features computed elsewhere (else oracle ViT of `img`)."""
    if ctx is None:
        ctx = O.vit_forward(img, sd, cfg)
    B = ctx.shape[0]
    h = head_forward(ctx, sd, cfg)
    cam = h["cam"]
    focal = cfg.focal_length * torch.ones(B, 2, dtype=ctx.dtype)
    cam_t = torch.stack([cam[:, 1], cam[:, 2], 2 * focal[:, 0] / (cfg.img_size * cam[:, 0] + 1e-9)], dim=-1)      # :165-169
    R = h["rotmat"]
    verts, joints = O.smpl_forward(R[:, [0]], R[:, 1:], h["betas"], smpl)
    kp2d = O.perspective_projection(joints, cam_t, focal / cfg.img_size)
    return {
        "pred_cam": cam,
        "pred_smpl_params": {"global_orient": R[:, [0]], "body_pose": R[:, 1:], "betas": h["betas"]},
        "pred_cam_t": cam_t,
        "focal_length": focal,
        "pred_keypoints_3d": joints,
        "pred_vertices": verts,
        "pred_keypoints_2d": kp2d,
        # extras (not in the reference dict) used by parity tests
        "vit_features": ctx, "token_out": h["token_out"], "pose6d": h["pose6d"],
    }
