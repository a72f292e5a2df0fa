"""Drop-ins for the tokenizer's entry points:

    from tokenhmr_amd.tokenizer import DecodeTokens, EncodeTokens, VanillaTokenizer     # was: from tokenization.models.vanilla_pose_vqvae import ...
    pose6d = DecodeTokens(ckpt_path)(logits)        # (B,160,2048) token probabilities -> (B,21,6)   vanilla_pose_vqvae.py:258-301
    idx    = EncodeTokens(ckpt_path)(pose6d)        # (B,21,6) -> (B*160,) int64 code indices         vanilla_pose_vqvae.py:304-346
    net = VanillaTokenizer(ckpt['hparams'].ARCH); net.load_state_dict(ckpt['net'])                  # train_poseVQ.py:63-66 (EXP.EVAL_ONLY)
    output, commit_loss, perplexity = net(pose)     # the round trip eval_poseVQ.py:88 evaluates      vanilla_pose_vqvae.py:195-255

Same constructor arguments, same call, same result layout as the reference classes; the arithmetic runs in the HIP engine
(`thmr_vq_decode`: soft codebook lookup + PoseSPDecoderV1; `thmr_encode_tokens`: PoseSPEncoderV1 + argmin-L2 quantiser).  The file is
the reference's `tokenizer.pth` ({'net', 'hparams': yacs CfgNode}), read without yacs (`ckpt_io.load_checkpoint`), its `hparams.ARCH` checked
against the architecture the kernels are built for.  An engine serves the whole TokenHMR path, so a tokenizer-only one is an engine of
ViT / decoder depth 1 whose other weights are zeros (~80 MB); pass `engine=` to share the engine of a loaded model instead
(`load_tokenhmr(...)[0].engine`: its tokenizer is the one the model was trained with).
"""
import torch

from . import ckpt_io
from . import weights as W
from .config import HMRConfig


def _read_tokenizer_file(ckpt_path):
    """(ckpt['net'], hparams.ARCH as a dict or None) of a tokenizer.pth, its architecture checked against the kernels'."""
    ckpt = ckpt_io.load_checkpoint(ckpt_path)
    if not isinstance(ckpt, dict) or "net" not in ckpt:
        raise KeyError(f"{ckpt_path}: not a tokenizer checkpoint (no 'net' entry, vanilla_pose_vqvae.py:299-301)")
    arch = ckpt_io.tokenizer_arch(ckpt)
    ckpt_io.check_tokenizer_arch(arch, HMRConfig(vit_depth=1, dec_depth=1))
    return ckpt["net"], arch


def _select_tokenizer_tensors(net, what, need_encoder, strict_unexpected=False):
    """The engine's tokenizer tensors out of a 'net' state dict (decoder + codebook, and the encoder half when complete);
    KeyError naming what is missing.  strict_unexpected: also refuse keys the engine has no slot for ('body_model.*' excepted:
    the reference's module carries its SMPL-H layer in the same dict, eval_poseVQ.py:118-125)."""
    cfg = HMRConfig(vit_depth=1, dec_depth=1)
    net = {k: v for k, v in net.items() if torch.is_tensor(v)}
    names = [n for n, *_ in W.tokenizer_spec(cfg)]
    enc_names = [n for n, *_ in W.tokenizer_encoder_spec(cfg)]
    missing = [n for n in names + (enc_names if need_encoder else []) if n not in net]
    if missing:
        raise KeyError(f"{what}: tokenizer tensors missing from ckpt['net']: {missing[:4]}{' ...' if len(missing) > 4 else ''}")
    if strict_unexpected:
        known = set(names) | set(enc_names)
        extra = [k for k in net if k not in known and not k.startswith("body_model.")]
        if extra:
            raise KeyError(f"{what}: unexpected tensors in the tokenizer state dict: {extra[:4]}{' ...' if len(extra) > 4 else ''}")
    for n, shape, *_ in W.tokenizer_spec(cfg) + W.tokenizer_encoder_spec(cfg):
        if n in net and tuple(net[n].shape) != tuple(shape):
            raise ValueError(f"{what}: '{n}' has shape {tuple(net[n].shape)}, the engine is built for {tuple(shape)}")
    tok = {n: net[n].float() for n in names}
    tok.update({n: net[n].float() for n in enc_names if all(m in net for m in enc_names)})
    return tok


def _engine_from_tensors(tok, device, max_batch):
    from .engine import Engine
    from .smpl_assets import make_synthetic_smpl
    cfg = HMRConfig(vit_depth=1, dec_depth=1)
    # the rest of the contract (backbone / head of depth 1): zeros — never read by the two tokenizer entry points
    rest = {n: torch.zeros(shape) for n, shape, *_ in W.spec(cfg)}
    eng = Engine(cfg, max_batch=max_batch, device=device)
    eng.load_state(rest, tok)
    eng.load_smpl(make_synthetic_smpl(cfg, 0))
    eng.finalize()
    return eng


def _tokenizer_engine(ckpt_path, device, max_batch, need_encoder):
    net, _ = _read_tokenizer_file(ckpt_path)
    return _engine_from_tensors(_select_tokenizer_tensors(net, ckpt_path, need_encoder), device, max_batch)


class _TokenizerModule:
    def __init__(self, ckpt_path, device, max_batch, engine, need_encoder):
        self.device = torch.device(device) if engine is None else engine.device
        self.max_batch = max_batch if engine is None else engine.max_batch
        self.engine = engine if engine is not None else _tokenizer_engine(ckpt_path, self.device, max_batch, need_encoder)

    # nn.Module surface the callers touch
    def eval(self):
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("tokenhmr_amd implements the inference path only")
        return self

    def to(self, device):
        d = torch.device(device)
        if d.type != self.device.type or (d.index is not None and d.index != self.device.index):
            raise ValueError(f"this module's engine lives on {self.device}; build it with device={device!r} instead of moving it")
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    def __call__(self, x):
        with torch.no_grad():
            return self.forward(x)

    def _chunks(self, x):
        for i in range(0, x.shape[0], self.max_batch):
            yield x[i:i + self.max_batch]


class DecodeTokens(_TokenizerModule):
    """vanilla_pose_vqvae.py:258-301.  `mesh_inference` only adds an SMPL mesh to the reference decoder's side outputs, which
    DecodeTokens.forward does not return; accepted and ignored."""

    def __init__(self, ckpt_path="", mesh_inference=False, device="cuda:0", max_batch=64, engine=None):
        super().__init__(ckpt_path, device, max_batch, engine, need_encoder=False)

    def forward(self, logits):
        """logits: (B,160,2048) token PROBABILITIES (the reference names them logits; token_classifier.py:104-106 passes the softmax) ->
        pred_pose_body_6d (B,21,6)."""
        if logits.dim() != 3 or tuple(logits.shape[1:]) != (160, 2048):
            raise ValueError(f"DecodeTokens expects (B,160,2048), got {tuple(logits.shape)}")
        if logits.shape[0] == 0:
            return torch.empty(0, 21, 6, device=self.device)
        return torch.cat([self.engine.vq_decode(c) for c in self._chunks(logits)], 0)


class EncodeTokens(_TokenizerModule):
    """vanilla_pose_vqvae.py:304-346."""

    def __init__(self, ckpt_path="", device="cuda:0", max_batch=64, engine=None):
        super().__init__(ckpt_path, device, max_batch, engine, need_encoder=True)

    def forward(self, x):
        """x: (B,21,6) rot6d body pose -> code indices, int64, flattened to (B*160,) as QuantizeEMAReset.quantize returns them
        (quantize_cnn.py:80-86 on the (B*160,256) rows of `preprocess`, :74-78); `.view(B, -1)` gives VanillaTokenizer.encode's layout."""
        if x.dim() != 3 or tuple(x.shape[1:]) != (21, 6):
            raise ValueError(f"EncodeTokens expects (B,21,6), got {tuple(x.shape)}")
        if x.shape[0] == 0:
            return torch.empty(0, dtype=torch.int64, device=self.device)
        return torch.cat([self.engine.encode_tokens(c) for c in self._chunks(x)], 0).reshape(-1).to(torch.int64)


class VanillaTokenizer(_TokenizerModule):
    """vanilla_pose_vqvae.py:195-255, the model the reference itself evaluates (train_poseVQ.py:57-68 with EXP.EVAL_ONLY,
    utils/eval_poseVQ.py:70-143): encoder -> QuantizeEMAReset -> decoder in one engine call (`thmr_tokenizer_roundtrip`), the latent
    never leaving the device.

        net = VanillaTokenizer(ckpt['hparams'].ARCH, mesh_inference=False)      # get_model(pretrained_hparams)
        net.load_state_dict(ckpt['net'], strict=True); net.cuda(); net.eval()
        output, loss_commit, perplexity = net(pose)

    The reference's positional arguments, then keyword-only ones of this port: `ckpt_path` (a tokenizer.pth to read instead of a later
    load_state_dict), `device`, `max_batch`, `engine` (share the engine of a loaded model: `load_tokenhmr(...)[0].engine`, which must
    have been given the encoder half) and `body_model`.  `arch_params` (a node or dict with the keys of hparams.ARCH) and the file's own
    hparams.ARCH are checked against the architecture the kernels are built for (`ckpt_io.check_tokenizer_arch`); 6D input and
    output only.  `add_noise=True` and `train(True)` raise NotImplementedError: this is the inference path.

    forward(x, global_step=None) -> (output, commit_loss, perplexity).  x: (B,21,6), or (B,21,3,3) rotation matrices whose first two
    rows are taken (matrix_to_rotation_6d, rotation_utils.py).  output: 'pred_pose_body_6d' (B,21,6), 'pred_pose_body_rotmat'
    (B,21,3,3), and with mesh_inference=True 'pred_pose_body_aa' (B,63).  The two scalars are 0-dim device tensors; nothing synchronises.
    The reference runs ONE quantiser call over the whole batch; here more than `max_batch` poses are chunked, so the statistics are
    merged to what that one call gives: `code_count` accumulates over the chunks on the device, the perplexity is that of the summed
    histogram, and the commit loss is the rows-weighted mean of the chunks' means (equal to the single mean up to fp32 rounding).
    `code_count` ((2048) int32, the last forward's histogram) is kept for codebook-usage reports.

    The body mesh ('pred_body_mesh', 'pred_body_vertices', 'pred_body_joints', vanilla_pose_vqvae.py:182-191) needs an SMPL-H layer, and
    no SMPL-H asset ships with this package: mesh_inference=True produces the axis-angle output and — only when `body_model=` is given —
    the three mesh keys; without it they are absent.  `body_model` is a directory or file holding SMPLH_NEUTRAL.pkl, or a constants dict
    (smpl_assets.load_smplh_pkl / make_synthetic_smplh): the module then builds a `tokenhmr_amd.smplh.SMPLHLayer` on its device, which
    runs the folded 22-joint kernels; or any callable, called as body_model(body_pose=rotmat) like the reference's module-level layer.

    `__call__` is the inference path and stays under no_grad.  The value and gradient of the training objective for its output (with a
    body model) take two lines (tokenhmr_amd.tokenizer_loss):

        output, loss_commit, perplexity = net(gt_pose)
        losses, grad_6d = PoseReConsLoss(hparams.LOSS, 21, 'rotmat', 'smplh', body_model=net.body_model).value_and_grad(batch, output, loss_commit)

    encode(x) -> (B,160) int64 does what EncodeTokens does (encoder, `preprocess`, argmin).  The reference's own
    VanillaTokenizer.encode RAISES ("mat1 and mat2 shapes cannot be multiplied (768x160 and 256x2048)"): it skips `preprocess`
    (:238-240), so there is no reference behaviour to match beyond the layout its `.view(batch_size, -1)` intends.
    decode(idx) -> (B,21,6) is the plain hard lookup + decoder (no straight-through term)."""

    def __init__(self, arch_params=None, input_joint_dim=6, output_joint_dim=6, mesh_inference=False, add_noise=False, *, ckpt_path="",
                 device="cuda:0", max_batch=64, engine=None, body_model=None):
        if add_noise:
            raise NotImplementedError("tokenhmr_amd implements the inference path only (add_noise is a training augmentation)")
        if input_joint_dim != 6 or output_joint_dim != 6:
            raise ValueError(f"the engine's tokenizer is built for 6D rotations in and out, got {input_joint_dim} / {output_joint_dim}")
        cfg = HMRConfig(vit_depth=1, dec_depth=1)
        if arch_params is not None:
            ckpt_io.check_tokenizer_arch(ckpt_io.tokenizer_arch({"hparams": {"ARCH": arch_params}}), cfg)
            try:
                joints = ckpt_io._scalar(ckpt_io._field(arch_params, "NB_JOINTS"))
            except KeyError:
                joints = 21
            if joints != 21:
                raise ValueError(f"tokenizer architecture differs from the engine's: ARCH.NB_JOINTS = {joints!r}, the HIP kernels are built for 21")
        self.mesh_inference = bool(mesh_inference)
        self.body_model = body_model
        self._own_body_model = body_model is not None and not callable(body_model)       # a model path or a constants dict
        self.code_count = None
        self._own_engine = engine is None
        tok = None
        if engine is None and ckpt_path:
            net, _ = _read_tokenizer_file(ckpt_path)
            tok = _select_tokenizer_tensors(net, ckpt_path, need_encoder=True)
        self.device = torch.device(device) if engine is None else engine.device
        self.max_batch = max_batch if engine is None else engine.max_batch
        self.engine = engine if engine is not None else (_engine_from_tensors(tok, self.device, max_batch) if tok is not None else None)
        if self._own_body_model:
            from .smplh import SMPLHLayer
            self.body_model = SMPLHLayer(body_model, num_betas=10, ext="pkl", max_batch=self.max_batch, device=self.device)

    def _body_mesh(self, rot):
        """body_model(body_pose=rotmat), vanilla_pose_vqvae.py:184.  The layer this module built itself holds max_batch poses per call,
        like the engine: more are chunked and the pieces joined."""
        if not self._own_body_model or rot.shape[0] <= self.max_batch:
            return self.body_model(body_pose=rot)
        import types
        parts = [self.body_model(body_pose=c) for c in self._chunks(rot)]
        return types.SimpleNamespace(**{k: torch.cat([getattr(p, k) for p in parts], 0)
                                        for k in ("vertices", "joints", "full_pose", "betas", "body_pose", "global_orient")}, transl=None)

    def load_state_dict(self, net, strict=True):
        """ckpt['net'] as train_poseVQ.py:63-66 passes it; 'body_model.*' keys (the reference module's SMPL-H layer) are ignored.
        strict: any other key the engine has no slot for is a KeyError, as is a missing tensor (either half)."""
        if not isinstance(net, dict):
            raise KeyError("load_state_dict expects the checkpoint's 'net' dict")
        if not self._own_engine:
            raise ValueError("this module shares a loaded model's engine, which carries its own tokenizer; build it without engine= to load weights")
        tok = _select_tokenizer_tensors(net, "load_state_dict", need_encoder=True, strict_unexpected=strict)
        if self.engine is None:
            self.engine = _engine_from_tensors(tok, self.device, self.max_batch)
        else:
            self.engine.load_state({}, tok)
            self.engine.finalize()
        return torch.nn.modules.module._IncompatibleKeys([], [])

    def __call__(self, x, global_step=None):
        with torch.no_grad():
            return self.forward(x, global_step)

    def _engine(self):
        if self.engine is None:
            raise RuntimeError("VanillaTokenizer has no weights yet: call load_state_dict(ckpt['net']) or pass ckpt_path= / engine=")
        return self.engine

    def _pose6d(self, x):
        if x.dim() == 4 and tuple(x.shape[1:]) == (21, 3, 3):
            x = x[:, :, :2, :].reshape(x.shape[0], 21, 6)          # matrix_to_rotation_6d: the first two rows
        if x.dim() != 3 or tuple(x.shape[1:]) != (21, 6):
            raise ValueError(f"VanillaTokenizer expects (B,21,6) or (B,21,3,3), got {tuple(x.shape)}")
        return x.to(self.device, torch.float32).contiguous()

    def forward(self, x, global_step=None):
        eng = self._engine()
        x = self._pose6d(x)
        B = x.shape[0]
        if B == 0:
            raise ValueError("VanillaTokenizer.forward needs at least one pose")
        want = ("pose6d", "rotmat", "commit_loss", "perplexity") + (("aa",) if self.mesh_inference else ())
        counts = torch.zeros(2048, device=self.device, dtype=torch.int32)
        parts, commit, perp = [], None, None
        for c in self._chunks(x):
            o = eng.tokenizer_roundtrip(c, want=want, outputs={"code_count": counts}, accumulate=True)
            parts.append(o)
            w = o["commit_loss"] * (c.shape[0] / B)
            commit = w if commit is None else commit + w
            perp = o["perplexity"]                     # of the counts summed so far: the last chunk's is the batch's
        if len(parts) == 1:
            commit = parts[0]["commit_loss"]
        self.code_count = counts
        cat = (lambda k: parts[0][k]) if len(parts) == 1 else (lambda k: torch.cat([p[k] for p in parts], 0))
        rot = cat("rotmat")
        output = {"pred_pose_body_6d": cat("pose6d"), "pred_pose_body_rotmat": rot}
        if self.mesh_inference:
            output["pred_pose_body_aa"] = cat("aa").reshape(B, 63)
            if self.body_model is not None:
                mesh = self._body_mesh(rot)
                output.update({"pred_body_mesh": mesh, "pred_body_vertices": mesh.vertices, "pred_body_joints": mesh.joints})
        return output, commit, perp

    def encode(self, x):
        eng = self._engine()
        x = self._pose6d(x)
        if x.shape[0] == 0:
            return torch.empty(0, 160, dtype=torch.int64, device=self.device)
        with torch.no_grad():
            return torch.cat([eng.encode_tokens(c) for c in self._chunks(x)], 0).to(torch.int64)

    def decode(self, idx):
        eng = self._engine()
        if idx.dim() != 2 or idx.shape[1] != 160:
            raise ValueError(f"VanillaTokenizer.decode expects (B,160) code indices, got {tuple(idx.shape)}")
        if idx.shape[0] == 0:
            return torch.empty(0, 21, 6, device=self.device)
        with torch.no_grad():
            return torch.cat([eng.vq_decode_idx(c) for c in self._chunks(idx)], 0)
