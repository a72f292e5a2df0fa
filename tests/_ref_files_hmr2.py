"""Writer of look-alike HMR2.0 reference files (MODEL.SMPL_HEAD.TYPE: transformer_decoder) for the loader tests, CPU and GPU.

The checkpoint, the SMPL pickles and the mean parameters come from tests/_ref_files.write_reference_files (called with an EMPTY
tokenizer, whose file is then deleted: an HMR2 model has none); model_config.yaml is rewritten in the 4D-Humans form — no
MODEL.TOKENIZER_CHECKPOINT_PATH key, TRANSFORMER_DECODER spelled out as hmr2's model_config.yaml spells it."""
import os

from _ref_files import write_reference_files

DECODER_YAML = {"depth": 6, "heads": 8, "mlp_dim": 1024, "dim_head": 64, "dropout": 0.0, "emb_dropout": 0.0, "norm": "layer",
                "context_dim": 1280}


def write_hmr2_reference_files(tmp_path, cfg, sd, smpl, head_overrides=None, decoder_overrides=None, extra_state=None):
    """-> (checkpoint path, model_config.yaml path).  head_overrides: extra MODEL.SMPL_HEAD keys (IEF_ITERS, TRANSFORMER_INPUT,
    JOINT_REP); decoder_overrides: TRANSFORMER_DECODER keys."""
    ckpt, ycfg = write_reference_files(tmp_path, cfg, sd, {}, smpl, extra_state=extra_state)
    os.remove(tmp_path / "tokenizer.pth")
    dec = dict(DECODER_YAML, depth=cfg.dec_depth)
    dec.update(decoder_overrides or {})
    head = {"TYPE": "transformer_decoder", "IN_CHANNELS": 2048}
    head.update(head_overrides or {})
    lines = "".join(f"    {k}: {v}\n" for k, v in head.items())
    dlines = "".join(f"      {k}: {v}\n" for k, v in dec.items())
    (tmp_path / "model_config.yaml").write_text(f"""
MODEL:
  IMAGE_SIZE: 256
  IMAGE_MEAN: [0.485, 0.456, 0.406]
  IMAGE_STD: [0.229, 0.224, 0.225]
  BACKBONE:
    TYPE: vit
  SMPL_HEAD:
{lines}    TRANSFORMER_DECODER:
{dlines}SMPL:
  MODEL_PATH: {tmp_path}/smpl
  GENDER: neutral
  NUM_BODY_JOINTS: 23
  JOINT_REGRESSOR_EXTRA: {tmp_path}/SMPL_to_J19.pkl
  MEAN_PARAMS: {tmp_path}/smpl_mean_params.npz
EXTRA:
  FOCAL_LENGTH: 5000
DATASETS:
  DATASET_DIR: none
""")
    return ckpt, ycfg
