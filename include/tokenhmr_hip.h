/*
 * tokenhmr_hip.h — C ABI of the MI355X-native TokenHMR inference engine (libtokenhmr_hip.so).
 *
 * The reference (saidwivedi/TokenHMR) has no FFI: its seam is the Python method
 *     model, cfg = load_tokenhmr(ckpt, model_cfg)          tokenhmr/lib/models/__init__.py:3-26
 *     out = model(batch)                                    tokenhmr/lib/models/tokenhmr.py:330-338
 * called from tokenhmr/eval.py:147, tokenhmr/demo.py:78, tokenhmr/track.py:39.
 * This header is what a ctypes binding for that seam binds; the Python
 * facade tokenhmr_amd/model.py is exactly such a binding.
 *
 * Conventions
 *   - plain C types only; every pointer named *_dev is a device (HBM) pointer owned by the caller
 *     (e.g. torch.Tensor.data_ptr()); the engine owns its weight arena and scratch arena.
 *   - all tensors are fp32, contiguous, row-major in the reference's own layouts.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous
 *     on it.  thmr_forward performs no allocation and no host synchronisation.
 *   - return value: 0 on success, negative thmr_status on failure; thmr_last_error() gives text.
 *   - one engine per GPU / per caller thread; not re-entrant.
 */
#ifndef TOKENHMR_HIP_H
#define TOKENHMR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 3): thmr_smpl_desc.reserved became update_hips (a round-1 host that left it uninitialised would get the hip shift at
 * random); the resample tables / padding row / flag words of the weight arena are written by thmr_load_weights on the LOADING
 * engine (round 1: thmr_create on every engine; round 2: thmr_finalize_weights(0)) and validated — not written — by
 * thmr_finalize_weights(assume_all_loaded = 1).
 * 3 (round 3): thmr_set_vit_gemm / thmr_get_vit_gemm and the split3 operators added (no struct changed).
 * 4 (round 5): an engine is CREATED in mode 1 ("split3") — thmr_finalize_weights builds the split3 weight copies, thmr_forward runs the bf16
 *   matrix pipe from 3 crops on — and thmr_set_vit_gemm(0) is the opt-out to exact-fp32 MFMA (up to ABI 3 it was the other way round); no
 *   struct or signature changed.
 * 5 (round 6): thmr_config.reserved[0] became `flags` (THMR_CFG_*: create in the opt-out mode, create without co-residency-dependent kernels;
 *   a zeroed field = ABI 4's behaviour), thmr_mode_bytes added; the split3 weight copies are shared among the engines of one weight arena. */
#define THMR_ABI_VERSION 5

typedef enum {
    THMR_OK = 0,
    THMR_ERR_INVALID = -1,      /* bad argument / shape / missing tensor */
    THMR_ERR_HIP = -2,          /* a HIP runtime call failed */
    THMR_ERR_STATE = -3,        /* call order violated (e.g. forward before weights are finalised) */
    THMR_ERR_NOMEM = -4,
    THMR_ERR_UNSUPPORTED = -5   /* a well-formed input of a kind this library does not handle (thmr_jpeg_*: the message names what was found) */
} thmr_status;

typedef struct thmr_engine thmr_engine;

/* Architecture knobs.  Everything else (192 tokens, 1280 dim, 16x80 heads, 160x2048 tokens ...)
 * is fixed by the reference (vit.py:12-24, tokenhmr_release.yaml:65-81) and baked into kernels. */
typedef struct {
    int32_t abi_version;        /* must be THMR_ABI_VERSION */
    int32_t vit_depth;          /* 32 for ViT-H (vit.py:17); smaller only for tests */
    int32_t dec_depth;          /* 6 (tokenhmr_release.yaml:74) */
    int32_t max_batch;          /* crops per thmr_forward call the scratch arena is sized for */
    int32_t device;             /* HIP device ordinal */
    int32_t flags;              /* THMR_CFG_* below, 0 = defaults */
    int32_t reserved[2];        /* must be 0 */
} thmr_config;

/* thmr_config.flags */
enum {
    /* Create the engine in the exact-fp32 mode (as if thmr_set_vit_gemm(0) had been called before thmr_finalize_weights): finalize then
     * builds NO split3 weight copies and allocates no split3 activation buffers (3.8 GB + 0.5 GB at release depth and 64 crops, outside the
     * caller's arenas: thmr_mode_bytes).  thmr_set_vit_gemm(1) later builds them on demand. */
    THMR_CFG_VIT_GEMM_F32 = 1,
    /* No kernel that needs ALL its workgroups resident at once: the head runs as the launch chain instead of the persistent decoder kernel
     * (grid barrier) and the split3 GEMMs one workgroup per tile instead of the 256-workgroup stream with slab hand-over (the ViT bit-identical,
     * the head to fp32 summation order; a few per cent slower).  For a GPU SHARED WITH ANOTHER PROCESS: there the persistent kernels can starve each other until their bounded
     * waits (~0.5 s) run out — one batch of invalid outputs, an error from the next call, then this mode anyway (thmr_engine_status).  Engines
     * of ONE process are ordered by the library itself (one turn per forward-type call) and do not need the flag. */
    THMR_CFG_NO_PERSISTENT = 2,
    /* The engine runs the reference's OTHER SMPL head (MODEL.SMPL_HEAD.TYPE: transformer_decoder — SMPLTransformerDecoderHead,
     * tokenhmr/lib/models/heads/smpl_head.py:10-104: the HMR2.0 regressor, the format of the 4D-Humans checkpoints) instead of the token head:
     * the same ViT, to_kv GEMM, one-token decoder, SMPL and projection; behind token_out three Linears 1024 -> 144 / 10 / 3 (one stacked
     * read-out in fp32 with a fixed summation order), + the mean parameters, rot6d_to_rotmat over all 24 joints.  IEF_ITERS = 1, the zero
     * input token and JOINT_REP 6d only.  With the flag
     *   - thmr_spec enumerates 'backbone.*' and 'smpl_head.transformer.*' as without it, then smpl_head.decpose.{weight,bias} (144 x 1024,
     *     144), smpl_head.decshape.*, smpl_head.deccam.*, smpl_head.init_body_pose / init_betas / init_cam — no decpose_grot / decpose_hands /
     *     decpose.mixer_* and no tokenizer tensor; thmr_load_weights needs (and accepts) none of those; the arenas are smaller;
     *   - thmr_forward / thmr_head_forward fill every thmr_outputs field EXCEPT cls_logits_softmax, cls_logits and token_idx: a non-NULL
     *     pointer there is THMR_ERR_INVALID (thmr_last_error names the field); thmr_vq_argmin, thmr_vq_decode and thmr_encode_tokens
     *     likewise.  token_out is bit-identical to a token engine's for the same 'smpl_head.transformer.*' weights and context;
     *   - the record of thmr_pack_records keeps its layout; pass token_idx = NULL and its 160 words are zero.
     * Up to 128 crops the head behind the to_kv GEMM is two launches (the persistent decoder kernel with the read-out as its last step, and
     * the finish); beyond that, with THMR_CFG_NO_PERSISTENT and after a recovered barrier timeout, the launch chain (equal to fp32 summation
     * order of the read-out).  (Bit value 4 is not assigned: ABI 5 hosts were promised that it is refused, and it still is.) */
    THMR_CFG_HEAD_HMR2 = 8
};

/* One named tensor of the reference checkpoint contract:
 *   'backbone.*' / 'smpl_head.*'   tokenhmr/lib/utils/misc.py:242-256 (load_pretrained)
 *   'decoder.decoder.*', 'quantizer.codebook'   tokenization/models/vanilla_pose_vqvae.py:299-301 */
typedef struct {
    const char* name;
    const void* data;           /* fp32, contiguous, reference layout */
    int64_t     numel;
    int32_t     on_device;      /* 0: host pointer, 1: device pointer */
    int32_t     reserved;
} thmr_tensor_desc;

/* SMPL constants (replaces smplx.SMPLLayer buffers + joint_regressor_extra,
 * tokenhmr/lib/models/smpl_wrapper.py:11-25).  Host or device pointers (all same side). */
typedef struct {
    const float*   v_template;      /* (6890,3) */
    const float*   shapedirs;       /* (6890,3,10) */
    const float*   posedirs;        /* (207,20670)  smplx layout */
    const float*   J_regressor;     /* (24,6890) */
    const float*   lbs_weights;     /* (6890,24) */
    const float*   J19_regressor;   /* (19,6890)  SMPL_to_J19.pkl */
    const int32_t* parents;         /* (24) kinematic tree, parents[0] = -1 */
    const int32_t* extra_verts;     /* (21) smplx vertex_ids['smplh'] */
    const int32_t* joint_map;       /* (25) smpl_wrapper.py:19-20 */
    int32_t        on_device;
    int32_t        update_hips;     /* SMPL(update_hips=...) smpl_wrapper.py:11,33-36: 1 = shift the two hip joints (mapped joints 9, 12);
                                     * MUST be 0 or 1 (it was `reserved` in ABI 1: initialise it) */
} thmr_smpl_desc;

/* Output buffers of one forward (tokenhmr.py:156-188).  Any pointer may be NULL (= not wanted). */
typedef struct {
    float*   pred_cam;              /* (B,3) */
    float*   rotmat;                /* (B,24,3,3): [:,0] = global_orient, [:,1:] = body_pose */
    float*   betas;                 /* (B,10) */
    float*   cls_logits_softmax;    /* (B,160,2048) */
    float*   pred_cam_t;            /* (B,3) */
    float*   focal_length;          /* (B,2) */
    float*   pred_keypoints_3d;     /* (B,44,3) */
    float*   pred_vertices;         /* (B,6890,3) */
    float*   pred_keypoints_2d;     /* (B,44,2) */
    int32_t* token_idx;             /* (B,160) argmax_k logits, lowest index on ties */
    /* optional taps for parity tests */
    float*   vit_features;          /* (B,192,1280) token-major last_norm output */
    float*   token_out;             /* (B,1024) */
    float*   cls_logits;            /* (B,160,2048) raw logits */
    float*   pose6d;                /* (B,144) */
} thmr_outputs;

/* kernel-class ids for the built-in HIP-event profiler (bench.py roofline leg) */
enum {
    THMR_PROF_GEMM_QKV = 0, THMR_PROF_GEMM_PROJ = 1, THMR_PROF_GEMM_FC1 = 2, THMR_PROF_GEMM_FC2 = 3,
    THMR_PROF_ATTN = 4, THMR_PROF_LN = 5, THMR_PROF_PATCH = 6, THMR_PROF_DEC_KV = 7,
    THMR_PROF_HEAD = 8, THMR_PROF_LBS = 9, THMR_PROF_NUM = 10
};
typedef struct {
    double  ms;         /* sum of HIP-event durations on the launch stream */
    double  flops;      /* algorithmic flops (2*MAC) of those launches */
    double  bytes;      /* algorithmic HBM bytes of those launches */
    int64_t launches;
} thmr_prof_entry;

int         thmr_abi_version(void);
const char* thmr_build_info(void);

/* Bytes the engine needs; lets the caller allocate the arenas itself (e.g. as torch tensors so
 * that torch.distributed/RCCL can broadcast the weight arena). */
int thmr_arena_bytes(const thmr_config* cfg, size_t* weight_bytes, size_t* scratch_bytes);

/* Device memory the engine allocates ITSELF, outside the two arenas, for `vit_gemm_mode` (0 / 1, see thmr_set_vit_gemm): the split3 copies
 * of the ViT weights (shared by all engines of this process that were created on the same weight_arena_dev), the split3 activation operands
 * of max_batch crops, the hand-over workspace of the persistent GEMM.  All 0 for mode 0 and for max_batch < 3.  workspace_bytes is an
 * UPPER BOUND: the workspace is allocated on devices with 256 compute units only, elsewhere the engine allocates none (0 bytes) and
 * runs the per-tile kernels.  No GPU needed. */
int thmr_mode_bytes(const thmr_config* cfg, int32_t vit_gemm_mode, size_t* split_weight_bytes, size_t* split_act_bytes, size_t* workspace_bytes);

/* Enumerate the checkpoint contract the engine expects (name + element count), index = 0..count-1.
 * Returns the number of tensors; name/numel may be NULL.  No GPU needed. */
int thmr_spec(const thmr_config* cfg, int32_t index, const char** name, int64_t* numel);

/* weight_arena_dev / scratch_arena_dev may be NULL: the engine then hipMallocs and owns them. */
int thmr_create(const thmr_config* cfg, void* weight_arena_dev, void* scratch_arena_dev, thmr_engine** out);
void thmr_destroy(thmr_engine* e);
const char* thmr_last_error(const thmr_engine* e);   /* e may be NULL: last global error */

/* Weight ingest — replaces load_pretrained/prepare_statedict (misc.py:215-256) and
 * DecodeTokens.load_weights (vanilla_pose_vqvae.py:299-301).  May be called several times with
 * disjoint subsets; unknown names are an error (strict=True semantics). */
int thmr_load_weights(thmr_engine* e, const thmr_tensor_desc* tensors, size_t n, void* stream);
int thmr_load_smpl(thmr_engine* e, const thmr_smpl_desc* smpl, void* stream);
/* Checks every required tensor arrived and builds derived layouts (conv/codebook repacks,
 * J_template/J_shapedirs).  Also the hook to call after an external broadcast into the arena:
 * assume_all_loaded = 1 skips the per-tensor bookkeeping (this engine loaded nothing itself) and instead requires the loader's
 * magic word in the arena — THMR_ERR_STATE if the arena was never filled by a thmr_load_weights (e.g. broadcast too early).
 * The arena is complete for a broadcast as soon as the root's thmr_load_weights + thmr_load_smpl have returned; the root
 * may finalize before or after broadcasting. */
int thmr_finalize_weights(thmr_engine* e, int32_t assume_all_loaded, void* stream);
int thmr_weight_arena(thmr_engine* e, void** ptr_dev, size_t* bytes);

/* The hot path: TokenHMR.forward (tokenhmr.py:330-338 -> forward_step :135-188).
 * img_dev: (B,3,256,256) fp32 normalised RGB crops.  1 <= B <= max_batch. */
int thmr_forward(thmr_engine* e, const float* img_dev, int32_t B, const thmr_outputs* out, void* stream);

/* Device-side health of the engine: synchronises `stream` and returns THMR_ERR_HIP if a kernel of this engine reported an
 * error asynchronously — the bounded grid barrier of the persistent decoder kernel, or a bounded hand-over wait of the persistent split3 GEMM,
 * timed out instead of hanging the GPU.  thmr_forward itself never synchronises; it does look at host-mapped copies of the same error words
 * on entry, so a timeout is also reported by the NEXT forward-type call.  Either way the error is returned once: the engine drains the
 * device, resets the barrier words / hand-over workspace and switches to the launch chain / per-tile kernel (no co-residency needed), so
 * re-submitting the batch works.  It also returns THMR_ERR_INVALID, once, after a thmr_vq_decode_idx / thmr_tokenizer_roundtrip call met a code
 * index outside [0, 2048) (clamped on the device; see thmr_vq_decode_idx). */
int thmr_engine_status(thmr_engine* e, void* stream);

/* Diagnostics: with THMR_DEC_TIMELINE=1 in the environment at thmr_finalize_weights, workgroup 0 of the persistent decoder kernel
 * stamps the 100 MHz wall clock after every step and barrier of the last call; this copies up to max_stamps (<= 240) of them. */
int thmr_debug_decoder_timeline(thmr_engine* e, uint64_t* stamps_host, int32_t max_stamps, void* stream);

/* Diagnostics: which kernel and which K split every ViT GEMM (and the decoder's to_kv GEMM) of a B-crop call runs with — the very
 * function the engine evaluates at the top of each call (csrc/vit_plan.h), for an engine of this config in `vit_gemm_mode` (0 / 1) whose
 * weights are finalized.  streams_available: non-zero = the device has 256 CUs, the config has no THMR_CFG_NO_PERSISTENT and no hand-over
 * timeout was recovered (the tile streams exist); the flag in cfg turns it off by itself.  The SPLIT FACTORS (ksplit of proj / fc2) fix
 * the association of the K sums, i.e. the bits, and depend on mode and B only; the KINDS are decompositions of the same sums (time only).
 * B outside [1, max_batch], a bad mode or a null `out`: THMR_ERR_INVALID.  No GPU needed. */
typedef enum {
    THMR_GEMM_F32_TILE = 0,         /* exact-fp32 MFMA, one workgroup per tile (launch_gemm's cost model picks the tile) */
    THMR_GEMM_F32_TILE_SPLITK,      /* ... K split `ksplit` ways into partial planes, summed by the residual + LayerNorm kernel */
    THMR_GEMM_F32_RING,             /* 64x64 tiles on the LDS-DMA ring (few crops), `ksplit` ways */
    THMR_GEMM_F32_RING16,           /* 64x48 tiles of 16x16x4 MFMAs (qkv of one and two crops) */
    THMR_GEMM_S3_TILE,              /* split3 on the bf16 matrix pipe, one workgroup per tile (incl. the launcher's mixed grid with half tiles) */
    THMR_GEMM_S3_TILE_SPLITK,       /* ... `ksplit` copies of the grid writing partial planes */
    THMR_GEMM_S3_STREAM_WIDE,       /* 256 persistent workgroups over the 128 x 256 tile stream */
    THMR_GEMM_S3_STREAM_NARROW,     /* ... over the 128 x 128 tile stream (three-stage ring) */
    THMR_GEMM_S3_SPLITK_STREAM,     /* split K with (tile, K slice) units through the 128 x 128 stream */
    THMR_GEMM_S3_RING               /* experiments library only: the ring kernel on split3 operands */
} thmr_gemm_kind;
enum { THMR_VIT_PATH_F32 = 0, THMR_VIT_PATH_SPLIT3 = 1, THMR_VIT_PATH_SPLIT3_SMALL = 2 /* experiments library only */ };
enum { THMR_ATTN_F32 = 0, THMR_ATTN_F32_KEYSPLIT = 1, THMR_ATTN_F32_SPLIT3_OUT = 2, THMR_ATTN_B16 = 3 };
typedef struct thmr_gemm_choice {
    int32_t kind;               /* thmr_gemm_kind */
    int32_t ksplit;             /* 1 = unsplit */
} thmr_gemm_choice;
typedef struct thmr_vit_plan_desc {
    int32_t path;               /* THMR_VIT_PATH_*: which block loop runs (buffers and LayerNorm kernels differ) */
    thmr_gemm_choice patch, qkv, proj, fc1, fc2, to_kv;
    int32_t attn;               /* THMR_ATTN_* */
    int32_t bs_blk;             /* 1: fc1 writes fc2's operand in the row-blocked form (fc2 on the 128 x 256 stream) */
    int32_t part2_in_scratch;   /* 1: fc2's partial planes live in the scratch arena (3-4 crops), 0: behind the engine's operand buffers */
    int32_t tile_opts;          /* GemmArgs::tile_opts of the split3 GEMMs: bits 0-4 of csrc/gemm_split3_rule.h (0 in the shipped library) */
} thmr_vit_plan_desc;
int thmr_debug_vit_plan(const thmr_config* cfg, int32_t vit_gemm_mode, int32_t B, int32_t streams_available, thmr_vit_plan_desc* out);

/* Sub-paths (configs 2 of BASELINE.json and unit parity). */
int thmr_vit_forward(thmr_engine* e, const float* img_dev, int32_t B, float* feats_dev /*(B,192,1280)*/, void* stream);
int thmr_head_forward(thmr_engine* e, const float* ctx_dev /*(B,192,1280)*/, int32_t B, const thmr_outputs* out, void* stream);
/* SMPL forward (smpl_wrapper.py:27-41 over smplx lbs) + projection (geometry.py:86-124) */
int thmr_lbs_forward(thmr_engine* e, const float* rotmat_dev /*(B,24,3,3)*/, const float* betas_dev /*(B,10)*/,
                     const float* cam_dev /*(B,3) or NULL*/, int32_t B, float* verts_dev, float* joints_dev,
                     float* cam_t_dev, float* kp2d_dev, void* stream);
/* QuantizeEMAReset.quantize (tokenization/models/quantize_cnn.py:80-86): argmin_k ||x-c_k||^2 in the
 * reference's expanded form; x (rows,256) -> idx (rows) int32; optional dist (rows,2048). */
int thmr_vq_argmin(thmr_engine* e, const float* x_dev, int32_t rows, int32_t* idx_dev, float* dist_dev, void* stream);

/* Tokenizer encode path: EncodeTokens.forward (tokenization/models/vanilla_pose_vqvae.py:334-342)
 * = PoseSPEncoderV1 (:66-111) -> QuantizeEMAReset.preprocess/quantize (quantize_cnn.py:74-86).
 * Needs the optional 'encoder.encoder.*' tensors of tokenizer.pth (loaded through thmr_load_weights; all or none).
 * pose_dev (B,21,6) rot6d body pose -> idx_dev (B,160) int32 code indices; latent_dev (B,160,256) optional. */
int thmr_encode_tokens(thmr_engine* e, const float* pose_dev, int32_t B, int32_t* idx_dev, float* latent_dev, void* stream);
/* DecodeTokens.forward (vanilla_pose_vqvae.py:294-297): probs (B,160,2048) @ codebook -> PoseSPDecoderV1 -> pose6d (B,21,6).
 * One-hot probs give the hard decode of code indices (QuantizeEMAReset.dequantize, quantize_cnn.py:88-90). */
int thmr_vq_decode(thmr_engine* e, const float* probs_dev, int32_t B, float* pose6d_dev, void* stream);
/* The hard decode of code indices (QuantizeEMAReset.dequantize = F.embedding, quantize_cnn.py:88-90, then PoseSPDecoderV1): idx (B,160)
 * int32 -> pose6d (B,21,6).  A lookup kernel writes the decoder's first conv operand directly — no (B,160,2048) one-hot, no 2048-deep
 * GEMM — and the rest is thmr_vq_decode's: bit-identical to thmr_vq_decode of the one-hot probabilities (a one-hot row contributes one
 * non-zero fp32 term).  An index outside [0, 2048) is a caller error: the kernel clamps it (nothing is read out of bounds) and sets a
 * host-mapped flag word of the engine; thmr_engine_status, or the next thmr_vq_decode_idx / thmr_tokenizer_roundtrip on the engine,
 * then returns THMR_ERR_INVALID once and clears the flag.  The outputs of the call that carried the index are invalid. */
int thmr_vq_decode_idx(thmr_engine* e, const int32_t* idx_dev, int32_t B, float* pose6d_dev, void* stream);
/* The tokenizer round trip the reference evaluates (VanillaTokenizer.forward, vanilla_pose_vqvae.py:244-255, as driven by
 * train_poseVQ.py:57-68 with EXP.EVAL_ONLY and utils/eval_poseVQ.py:70-143): PoseSPEncoderV1 -> QuantizeEMAReset.forward
 * (quantize_cnn.py:95-130) -> PoseSPDecoderV1 -> rotation_6d_to_matrix -> matrix_to_axis_angle, the latent staying on the device.
 * Every field is a device buffer or NULL = "not wanted":
 *   idx          (B,160) int32      code indices (quantize_cnn.py:80-86, as thmr_encode_tokens)
 *   latent       (B,160,256)        the encoder's output in the quantiser's (N*T, C) layout
 *   pose6d       (B,21,6)           pred_pose_body_6d: the decoder on the STRAIGHT-THROUGH value x + (c - x) (quantize_cnn.py:124, fp32 in
 *                                   that order — an ulp away from the code row c on ~6 % of the elements, so it differs from
 *                                   thmr_vq_decode_idx(idx) in the last bits: the reference's own quirk)
 *   rotmat       (B,21,3,3)         pred_pose_body_rotmat (rotation_6d_to_matrix == geometry.rot6d_to_rotmat bit for bit on this input)
 *   aa           (B,21,3)           pred_pose_body_aa = matrix_to_axis_angle(rotmat) (see thmr_op_rotmat_to_aa)
 *   commit_loss  1 float            F.mse_loss(x, c[idx]) over the B*160*256 elements
 *   perplexity   1 float            exp(-sum p log(p + 1e-7)), p = code_count / sum(code_count) (with accumulate_counts: of the SUMMED counts)
 *   code_count   (2048) int32       the code-usage histogram of this call; accumulate_counts != 0: added to what the buffer holds
 * Needs the encoder tensors as thmr_encode_tokens does.  Allocates nothing and never synchronises the host, so a call can be captured in a
 * hipGraph like thmr_forward; two calls give identical bits (integer atomics for the histogram, fixed-order float sums).  Encoder and
 * statistics scratch is the engine's big time-shared buffer, the decoder's its own conv buffers: do not overlap a forward on one engine. */
typedef struct thmr_tokenizer_out {
    int32_t* idx;
    float* latent;
    float* pose6d;
    float* rotmat;
    float* aa;
    float* commit_loss;
    float* perplexity;
    int32_t* code_count;
    int32_t accumulate_counts;
    int32_t reserved;
} thmr_tokenizer_out;
int thmr_tokenizer_roundtrip(thmr_engine* e, const float* pose6d_dev /*(B,21,6)*/, int32_t B, const thmr_tokenizer_out* out, void* stream);

/* Stateless operator entry points (unit parity of individual kernels; no engine needed). */
/* C[M,N] = epilogue(A[M,K] . W[N,K]^T) in exact fp32 (v_mfma_f32_32x32x2_f32 / 16x16x4_f32; csrc/gemm_f32.hip).  epi: 0 none, 1 +bias,
 * 2 +bias gelu(erf), 3 +bias relu, 4 resid + (acc+bias), 5 (+bias)*qscale on cols < qcols, 6 +bias +pos_embed (patch embed).  K % 32 == 0.
 * Strides, in elements, < 2^22: lda (and, for the split3 operators below, ldw) is a multiple of 4 (split3: 8) and >= K; W of this operator
 * is dense (row stride K); ldc is ANY value >= N (ldc < N, like M, N or K < 1, is refused before any launch).  The residual is read with
 * C's row stride, and C == resid (the sum written in place, what the engine's proj / fc2 do) is allowed: every element is read and
 * written by the same lane.  The split3 kernels store C as 16-byte vectors only when ldc % 4 == 0 and C is 16-byte aligned, and read the
 * residual as vectors only when ldc % 4 == 0 (resid 16-byte aligned); otherwise element by element.  Nothing outside the M x N window
 * is written.  The split-K ids of both families reduce with 16-byte stores: N % 4 == 0, ldc % 4 == 0 and C 16-byte aligned, else refused.
 * variant (the ids the ENGINE uses; the A/B-only ids are listed in tokenhmr_amd/ops.py):
 *   -1 = tile picked by the cost model over the 128x128 / 128x160 / 128x96 / 64x64 LDS-DMA tiles (7 / 8 / 10 / 9 force one);
 *   2 = skinny (M <= 64); 100 + j = 64x64 ring kernel, 4-deep, split-K 2^j (few crops); 11 = tiny-M kernel (32x32 tiles, K split over the
 *   8 waves; K % 256 == 0; epilogues 0-5; the VQ decoder up to six crops); 120 = small-M kernel on 16x16x4 tiles (qkv at one and two crops);
 *   200 + t / 400 + t = split-K 2 / 4 on big tile t.  Every variant sums K in the same order except split-K, the tiny-M kernel and 120. */
int thmr_op_gemm(const float* A_dev, int64_t lda, const float* W_dev, const float* bias_dev, const float* resid_dev,
                 float* C_dev, int64_t ldc, int32_t M, int32_t N, int32_t K, int32_t epi, float qscale, int32_t qcols,
                 int32_t variant, void* stream);
/* fp32 GEMM on the bf16 matrix pipe (csrc/gemm_split16.hip) — what the engine's DEFAULT mode (thmr_set_vit_gemm 1) runs for the ViT GEMMs;
 * also an operator of its own, measured beside thmr_op_gemm.  Every fp32 operand is carried as three bf16 pieces h + m + l (x == h + m + l
 * up to 2^-24 |x|) in the "split3" layout [rows][K/8][3][8] bf16 (row stride 6 * ld bytes); the product keeps the six piece pairs down to
 * 2^-16 of |a b| (what is dropped is below one fp32 rounding of the product), accumulation is fp32 in the MFMA.
 * thmr_op_split3 converts (K % 8 == 0, ld_dst % 8 == 0, ld_dst >= K, ld_src % 4 == 0).  thmr_op_gemm_split3: A / W split3 with row strides
 * lda / ldw in fp32-equivalents (multiples of 8), K % 32 == 0; bias / resid / C fp32; epi 0, 1, 2, 4, 5, 6 as thmr_op_gemm (6: per-tile variants, N % 4 == 0).  variant:
 *   -1 = the engine's rule; 0 = 128x256 tile, 8 waves; 2 = 128x128, 4 waves; 5 = the 128x256 grid with its ragged last round as 128x128
 *         half tiles (only shapes whose tile count leaves at most half a round: fc1 of a 64-crop batch; else an error) — all bit-identical;
 *   202 / 204 = split-K 2 / 4 on the big tiles (the engine's 5 ... 31 crops use 2, 3 and 4 crops 4);
 *   300 = 256 PERSISTENT workgroups over a tile stream (M % 32 == 0, N % 256 == 0, at least 256 tiles, a 256-CU device; a ragged last round
 *         is split along K with the accumulators handed from one workgroup to the next through memory — bit-identical to 0 / 2; the
 *         engine's fc2 at 32 crops and more);
 *   + 1000 (1000, 1002, 1202, 1204, 1300; epi 0 / 4): A is a ROW-BLOCKED split3 operand [rows / 32][K / 8][3][32][8] (rows padded to 32;
 *         chunk (r, k-group, piece) at (r / 32) K 192 + (k-group 3 + piece) 512 + (r % 32) 16 bytes) — the form the engine's fc1 hands fc2.
 * (Ids of kernels that lost their A/B exist in the experiments build only: tokenhmr_amd/ops.py lists them.) */
int thmr_op_split3(const float* src_dev, int64_t ld_src, void* dst_dev, int64_t ld_dst, int64_t rows, int32_t K, void* stream);
int thmr_op_gemm_split3(const void* A_split_dev, int64_t lda, const void* W_split_dev, int64_t ldw, const float* bias_dev,
                        const float* resid_dev, float* C_dev, int64_t ldc, int32_t M, int32_t N, int32_t K, int32_t epi,
                        float qscale, int32_t qcols, int32_t variant, void* stream);
/* the same product with the epilogue's result written as a split3 operand (the next GEMM's A; row stride 6 * ldcs bytes, N % 8 == 0,
 * ldcs % 8 == 0) instead of fp32: bit-identical to thmr_op_split3 of thmr_op_gemm_split3's output.  epi 0, 1, 2, 5; variant -1, 0, 2, 5;
 * 302 = the persistent kernel (epi 0 / 2); + 1000 = the result in the row-blocked form (Cs holds ceil(M / 32) * 32 rows). */
int thmr_op_gemm_split3_out_split3(const void* A_split_dev, int64_t lda, const void* W_split_dev, int64_t ldw, const float* bias_dev,
                                   void* C_split_dev, int64_t ldcs, int32_t M, int32_t N, int32_t K, int32_t epi, float qscale,
                                   int32_t qcols, int32_t variant, void* stream);
int thmr_op_layernorm(const float* x_dev, const float* gamma_dev, const float* beta_dev, float* y_dev,
                      int32_t rows, int32_t D, float eps, int32_t relu, void* stream);
/* ViT global attention over 192 tokens, 16 heads x 80 (vit.py:113-122); qkv (B,192,3840) with q pre-scaled. */
int thmr_op_vit_attention(const float* qkv_dev, float* out_dev /*(B,192,1280)*/, int32_t B, void* stream);
/* the same with the kernel forced: 0 = the batch-size rule of thmr_op_vit_attention; 1 = three 64-query workgroups per (crop, head),
 * 3 = one 192-query workgroup, 5 = persistent workgroups (1 / 3 / 5 are bit-identical); 6 = key-split (16 queries per workgroup,
 * the 192 keys split over its 4 waves, partial softmaxes merged: what the engine uses up to six crops; equal to fp32 rounding;
 * 61 / 62 / 63 = the same with 16 / 32 / 48 queries per workgroup, bit-identical to each other) */
int thmr_op_vit_attention_variant(const float* qkv_dev, float* out_dev, int32_t B, int32_t variant, void* stream);
/* thmr_op_vit_attention with the output written as a split3 operand [B*192][1280/8][3][8] bf16 (see thmr_op_split3): for B >= 3
 * bit-identical to thmr_op_split3 of thmr_op_vit_attention's output; for B = 1 and 2 this operator runs the key-split kernel (another
 * order of the key sum), so there it is bit-identical to thmr_op_split3 of thmr_op_vit_attention_variant(..., 6, ...)'s output.
 * (The engine's split3 mode ran this up to round 4; it now runs thmr_op_vit_attention_b16 with out_split = 1.) */
int thmr_op_vit_attention_split3(const float* qkv_dev, void* out_split_dev, int32_t B, void* stream);
/* The same attention (vit.py:113-122) on the bf16 matrix pipe: q, k, v and the un-normalised probabilities enter v_mfma_f32_16x16x32_bf16 as
 * three bf16 pieces each, six products per pair, fp32 accumulate (csrc/attention_b16.hip) — the split3 mode's arithmetic applied to
 * q k^T and p v; the three 64-key blocks are combined with a running row maximum.  fp32-grade (error against fp64 at or below the fp32-MFMA
 * kernel's, tests/test_gpu_ops.py::test_vit_attention_b16), NOT bit-identical to thmr_op_vit_attention.  What the engine's split3 mode runs.
 * out_split = 0: out_dev is fp32 (B,192,1280); 1: the split3 operand [B*192][1280/8][3][8] bf16.  qt = 0: batch-size rule; 1: three
 * 64-query workgroups per (crop, head); 3: one workgroup of 192 queries (bit-identical to each other and for any B). */
int thmr_op_vit_attention_b16(const float* qkv_dev, void* out_dev, int32_t B, int32_t out_split, int32_t qt, void* stream);
/* rot6d_to_rotmat (geometry.py:64-84): (n,6) -> (n,3,3) */
int thmr_op_rot6d(const float* x_dev, float* R_dev, int32_t n, void* stream);
/* grad_x (n,6) = the vector-Jacobian product of thmr_op_rot6d with grad_R (n,3,3): the adjoint of the Gram-Schmidt step as
 * rotation_6d_to_matrix (tokenization/models/rotation_utils.py:510-531) and geometry.rot6d_to_rotmat write it — b1 = normalize(a1),
 * b2 = normalize(a2 - (b1 . a2) b1), b3 = b1 x b2, rows stacked, F.normalize's clamp of the norm at 1e-12 included (below the clamp the
 * normalisation is a division by a constant, as autograd has it).  Stateless, one launch, elementwise per rotation. */
int thmr_op_rot6d_backward(const float* x_dev, const float* grad_R_dev, float* grad_x_dev, int32_t n, void* stream);
/* aa_to_rotmat (geometry.py:5-44; axis-angle -> quaternion -> rotation matrix, the reference's in-tree "Rodrigues" used for
 * ground-truth poses at tokenhmr.py:235,260,357): (n,3) -> (n,3,3) */
int thmr_op_aa_to_rotmat(const float* aa_dev, float* R_dev, int32_t n, void* stream);
/* grad_aa (n,3) = the vector-Jacobian product of axis-angle -> rotation matrix with grad_R (n,3,3): the adjoint of smplx batch_rodrigues'
 * formula (angle = |aa + 1e-8|, R = I + sin K + (1 - cos) K^2, 1 - cos evaluated as 2 sin^2(angle / 2)), the kernel thmr_smpl_backward runs
 * for pose2rot = 1.  thmr_op_aa_to_rotmat goes through a quaternion instead: the same function of aa up to 1e-8 / |aa|, so this is its
 * gradient too. */
int thmr_op_aa_to_rotmat_backward(const float* aa_dev, const float* grad_R_dev, float* grad_aa_dev, int32_t n, void* stream);

/* The row, glue and head kernels around the GEMMs and the attention (csrc/rowops.hip, head.hip, hmr2_head.hip), each as the engine launches
 * it (tests/test_gpu_rowops.py).  Every entry point checks its arguments before any HIP call: a null buffer, a count <= 0 or a constraint
 * named below is THMR_ERR_INVALID with a message in thmr_last_error(NULL).  All buffers fp32 and contiguous unless said otherwise. */
/* The split-K reduce of the ViT residual stream fused with the next LayerNorm (vit.py:149-150 followed by :149 / :150 / :335):
 *   xout = resid + ((((part[0] + part[1]) + ...) + part[S-1]) + bias);  y = LayerNorm(xout; gamma, beta, eps)
 * part (S, rows, D) slabs of rows * D floats; bias, gamma, beta (D); resid, xout (rows, D) — resid == xout (in place) is what the engine
 * passes; y fp32 (rows, D), or with y_is_split3 the split3 operand [rows][D/8][3][8] bf16 (thmr_op_split3 of the fp32 y, bit for bit).
 * D == 1280, S >= 1; the split3 output exists for S == 2 and 4 only. */
int thmr_op_splitk_resid_ln(const float* part_dev, int32_t S, int32_t rows, int32_t D, const float* bias_dev, const float* resid_dev,
                            float* xout_dev, const float* gamma_dev, const float* beta_dev, void* y_dev, float eps, int32_t y_is_split3,
                            void* stream);
/* MixerLayer's layernorm2(x + y) (heads/modules.py:59): s_out = x + y, z_out = LayerNorm64(s_out); all (rows, 64), gamma / beta (64). */
int thmr_op_add_ln64(const float* x_dev, const float* y_dev, const float* gamma_dev, const float* beta_dev, float* s_out_dev,
                     float* z_out_dev, int32_t rows, float eps, void* stream);
/* batched transpose (Bn, R, C) -> (Bn, C, R) (MixerLayer's y.transpose(2, 1), heads/modules.py:56-58; the codebook at finalize).
 * Bn <= 65535, R <= 32 * 65535 (grid dimensions). */
int thmr_op_transpose(const float* in_dev, float* out_dev, int32_t Bn, int32_t R, int32_t C, void* stream);
/* cls_logits.softmax(-1) over 2048 classes (token_classifier.py:104) and the token index argmax_k logits, LOWEST index on ties:
 * logits (rows, 2048) -> probs (rows, 2048) and / or idx (rows) int32; either output may be null, not both. */
int thmr_op_softmax_argmax(const float* logits_dev, float* probs_or_null, int32_t* idx_or_null, int32_t rows, void* stream);
/* CrossAttention.forward for one query token per crop (pose_transformer.py:111-124): per (crop, head of 64) softmax((q . k_j) / 8) over
 * the 192 context rows, times v.  q, out (B, 512); kv rows (b * 192 + j) of a (B * 192, ldkv) matrix with K of head h at column
 * koff + 64 h and V at koff + 512 + 64 h (the engine: ldkv = 1024 * decoder depth, koff = 1024 * layer).
 * ldkv % 4 == 0, koff % 4 == 0, koff >= 0, koff + 1024 <= ldkv. */
int thmr_op_cross_attn(const float* q_dev, const float* kv_dev, int64_t ldkv, int32_t koff, float* out_dev, int32_t B, void* stream);
/* The patch-embed GEMM's A operand (vit.py:341 x[:, :, :, 32:-32], then :168 Conv2d(3, 1280, k 16, s 16, p 2)): img (B, 3, 256, 256) ->
 * A (B * 192, 768), row b * 192 + py * 12 + px, column c * 256 + ky * 16 + kx; the zero padding applies to the sliced 192-wide window.
 * out_split = 0: A fp32; 1: the split3 operand [B*192][768/8][3][8] bf16 (thmr_op_split3 of the fp32 form, bit for bit). */
int thmr_op_im2col_patch(const float* img_dev, void* A_dev, int32_t B, int32_t out_split, void* stream);
/* The A operand of Conv1d(C -> *, k 3, padding = dilation = dil) on a channels-last signal, nearest-resampled through src and optionally
 * ReLU'd first (vanilla_pose_vqvae.py:135-154, resnet.py:55-68):
 *   out[b][t][dk * C + c] = f(in[b][src[t + (dk - 1) dil]][c])  where 0 <= t + (dk - 1) dil < Tout, else 0
 * in (Bn, Tin, C), out (Bn, Tout, 3 C), src (Tout) int32 with values in [0, Tin) or null = identity (then Tin >= Tout).  C % 4 == 0, dil >= 1. */
int thmr_op_conv3_gather(const float* in_dev, float* out_dev, const int32_t* src_or_null, int32_t Bn, int32_t Tin, int32_t Tout,
                         int32_t C, int32_t dil, int32_t prerelu, void* stream);
/* The same for the tokenizer encoder's general Conv1d(ks, stride, pad) with the channels zero-padded from C to Cp
 * (vanilla_pose_vqvae.py:66-88):  out[b][t][kk * Cp + c] = in[b][src[tp]][c], tp = t * stride - pad + kk, where 0 <= tp < Tsrc and c < C,
 * else 0.  in (Bn, Tin, C), out (Bn, Tout, ks * Cp), src (Tsrc) int32 or null = identity (then Tin >= Tsrc).  Cp >= C, ks >= 1,
 * stride >= 1, pad >= 0. */
int thmr_op_conv_gather(const float* in_dev, float* out_dev, const int32_t* src_or_null, int32_t Bn, int32_t Tin, int32_t Tsrc,
                        int32_t Tout, int32_t C, int32_t Cp, int32_t ks, int32_t stride, int32_t pad, void* stream);
/* The W operand that goes with those gathers: a Conv1d weight (co, ci, kk) -> (co, kk * cp), element [o][k * cp + i] = w[o][i][k] for
 * i < ci and 0 for ci <= i < cp.  cp == ci: the plain repack; cp > ci: the zero-padded one; cp < ci is rejected. */
int thmr_op_conv_repack(const float* w_dev, float* wp_dev, int32_t co, int32_t ci, int32_t cp, int32_t kk, void* stream);
/* QuantizeEMAReset.quantize (quantize_cnn.py:80-86) behind the x . C^T GEMM:  dist[k] = (sum(x^2) - 2 dot[k]) + cnorm[k] and its argmin,
 * LOWEST index on ties.  x (rows, 256), dot (rows, 2048), cnorm (2048) -> idx (rows) int32, dist (rows, 2048) optional. */
int thmr_op_vq_argmin_rows(const float* x_dev, const float* dot_dev, const float* cnorm_dev, int32_t* idx_dev, float* dist_or_null,
                           int32_t rows, void* stream);
/* quantize_cnn.py:83 torch.sum(k_w ** 2, dim=0):  cb (ncode, 256) -> cn (ncode). */
int thmr_op_code_norm(const float* cb_dev, float* cn_dev, int32_t ncode, void* stream);
/* What QuantizeEMAReset.forward returns beside the codes (quantize_cnn.py:38-47,118-121; csrc/tokenizer.hip), over x (rows, 256), the
 * codebook (2048, 256) and idx (rows) int32:  code_count (2048) int32 histogram (integer atomics; accumulate = 0 overwrites, else adds to
 * the caller's counts), commit = mean((x - codebook[idx])^2), perplexity = exp(-sum p log(p + 1e-7)) with p = code_count / sum(code_count)
 * AFTER this call's update.  commit / perplexity: one device float each, either may be null.  partial_scratch: ceil(rows / 32) floats.
 * Fixed-order float sums, no float atomics: two runs are bit-equal.  No host synchronisation.  An index outside [0, 2048) is clamped. */
int thmr_op_vq_stats(const float* x_dev, const float* codebook_dev, const int32_t* idx_dev, int32_t rows, int32_t* code_count_dev,
                     int32_t accumulate, float* partial_scratch_dev, float* commit_or_null, float* perplexity_or_null, void* stream);
/* matrix_to_axis_angle (tokenization/models/rotation_utils.py:428-441): (n,3,3) -> (n,3), the reference's route exactly:
 * _sqrt_positive_part of the four squared quaternion magnitudes, the candidate of the largest one (lowest index on ties) over
 * 2 max(q_abs, 0.1), half = atan2(|q_1..3|, q_0), angle = 2 half, q_1..3 / (|angle| < 1e-6 ? 0.5 - angle^2 / 48 : sin(half) / angle) with the
 * divisor clamped at the smallest normal float.  The quaternion is NOT standardised: q_0 < 0 gives an angle above pi, as the reference. */
int thmr_op_rotmat_to_aa(const float* R_dev, float* aa_dev, int32_t n, void* stream);
/* What follows the read-out GEMM of the SMPL head: mean parameters added, rot6d_to_rotmat (geometry.py:64-84) over the 24 joints,
 * pred_cam_t = [cam1, cam2, 2 f / (img_size cam0 + 1e-9)] (tokenhmr.py:165-169).  ro (B, ldro).
 *   kind 0, the token head (token_head.py:99-105,123): ro columns grot 0..5 | shape 6..15 | cam 16..18 | hands 19..30, ldro >= 31;
 *           pose6d = [ro 0..5 | bpose (B, 126) | ro 19..30] + init_pose; bpose is required;
 *   kind 1, the HMR2 head (smpl_head.py:56-103): ro columns pose 0..143 | shape 144..153 | cam 154..156, ldro >= 157; bpose is unused.
 * init_pose (144), init_betas (10), init_cam (3) -> rotmat (B, 24, 3, 3), betas (B, 10), cam (B, 3); pose6d (B, 144), cam_t (B, 3) and
 * focal (B, 2) are optional (null). */
int thmr_op_head_finish(int32_t kind, const float* ro_dev, int32_t ldro, const float* bpose_or_null, const float* init_pose_dev,
                        const float* init_betas_dev, const float* init_cam_dev, float* pose6d_or_null, float* rotmat_dev,
                        float* betas_dev, float* cam_dev, float* cam_t_or_null, float* focal_or_null, float focal_length, float img_size,
                        int32_t B, void* stream);
/* The decoder's first token (pose_transformer.py:350-354 with the zero input token of token_head.py:91): x[b][:] = bias + pos for every
 * crop; bias, pos (E) -> x (B, E).  B * E <= 2^30. */
int thmr_op_decoder_init(const float* bias_dev, const float* pos_dev, float* x_dev, int32_t B, int32_t E, void* stream);

/* Stand-alone SMPL model: the GT-side meshes the reference computes per sample on the CPU with
 * smplx.SMPL(gender) inside dataset workers (tokenhmr/lib/datasets/image_dataset.py:151-164,254-270, emdb_dataset.py:184-199)
 * reuse the LBS kernels with their own (male / female) constants.
 *   pose2rot = 0: pose_dev is (B,24,3,3) rotation matrices; 1: (B,72) axis-angle, converted by smplx batch_rodrigues. */
typedef struct thmr_smpl thmr_smpl;
int  thmr_smpl_create(const thmr_smpl_desc* desc, int32_t max_batch, int32_t device, thmr_smpl** out);
void thmr_smpl_destroy(thmr_smpl* m);
int  thmr_smpl_forward(thmr_smpl* m, const float* pose_dev, int32_t pose2rot, const float* betas_dev, int32_t B,
                       float* verts_dev /*(B,6890,3)*/, float* joints_dev /*(B,44,3) or NULL*/, void* stream);
/* The body model's vector-Jacobian product: what smplx.SMPL / SMPLLayer give under torch autograd.  New symbols under
 * ABI 5: no struct or signature changed.
 * thmr_smpl_grad_reserve, once per handle: allocates the backward workspace (the gradient of v_posed, the per-workgroup bone-matrix
 * partial sums, the split-K planes of the blend GEMM's reverse) and builds the transposed copy of the blend-shape matrix.  It may allocate
 * and synchronise; a second call does nothing.  A handle that never calls it keeps the footprint it had.
 * thmr_smpl_backward takes the pose and betas of the forward it differentiates (it recomputes the forward's intermediates into the
 * handle's workspace, so forwards issued in between do not matter) and the gradients of the two outputs; a NULL gradient input means
 * zeros, a NULL output is not computed.  grad_pose_dev has the layout of pose_dev: (B,24,3,3) for pose2rot = 0 — the plain derivative by
 * each matrix entry, as autograd gives it — or (B,72).  It never allocates and never synchronises: capturable in a graph on one stream.
 * No floating-point atomics: every sum has a fixed order, so the result is bit-reproducible and a crop's gradient does not depend on the
 * rest of the batch.  THMR_ERR_INVALID (message in thmr_last_error(NULL)) before any launch for a null handle, pose or betas, both
 * gradient inputs null, both outputs null, B outside [1, max_batch], a pose2rot that is not 0 or 1, a handle that has not reserved. */
int  thmr_smpl_grad_reserve(thmr_smpl* m);
int  thmr_smpl_backward(thmr_smpl* m, const float* pose_dev, int32_t pose2rot, const float* betas_dev, int32_t B,
                        const float* grad_verts_dev /*(B,6890,3) or NULL*/, const float* grad_joints_dev /*(B,44,3) or NULL*/,
                        float* grad_pose_dev /*(B,24,3,3) or (B,72); may be NULL*/, float* grad_betas_dev /*(B,10); may be NULL*/,
                        void* stream);

/* Stand-alone SMPL-H model: the body mesh of the tokenizer workflow.  Replaces smplx.SMPLHLayer, the decoder's module-level
 * body model (tokenization/models/vanilla_pose_vqvae.py:10-17, called :182-191 as body_model(body_pose=rotmat)), and smplx.SMPLH, the
 * dataset's per-item CPU ground truth (tokenization/dataset/dataset_poseVQ.py:81,111-113), by one batched device call (csrc/smplh.hip).
 * 52 chain joints (22 body + 2 x 15 hand), 459 pose features, 73 output joints = the 52 posed chain joints + the 21 vertices
 * extra_verts picks (smplx vertex_ids['smplh'] in VertexJointSelector order).  New symbols under ABI 5: no struct or signature changed.
 *   v_template (6890,3), shapedirs (6890,3,10), posedirs (459,20670) smplx's layout, J_regressor (52,6890), lbs_weights (6890,52),
 *   parents[52] (parents[0] = -1, parents[i] in [0, i)), extra_verts[21] (ids in [0, 6890)); on_device: the pointers are device memory.
 * thmr_smplh_create refuses (THMR_ERR_INVALID, message in thmr_last_error(NULL)) a null field, parents[0] != -1, a parents[i] outside
 * [0, i) and an extra_verts id outside [0, 6890).  It also builds the FOLDED tables of the body-only path: every hand joint's weight
 * column added into the body joint it hangs from (its wrist), and the blend-shape operand of the 21 body joints' 189 pose features. */
typedef struct thmr_smplh_desc {
    const float* v_template;
    const float* shapedirs;
    const float* posedirs;
    const float* J_regressor;
    const float* lbs_weights;
    const int32_t* parents;
    const int32_t* extra_verts;
    int32_t on_device;
    int32_t reserved;
} thmr_smplh_desc;
typedef struct thmr_smplh thmr_smplh;
int  thmr_smplh_create(const thmr_smplh_desc* desc, int32_t max_batch, int32_t device, thmr_smplh** out);
void thmr_smplh_destroy(thmr_smplh* m);
/* pose2rot = 0: pose_dev holds rotation matrices; 1: axis-angle, converted by smplx batch_rodrigues (thmr_op_aa_to_rotmat's kernel).
 * body_only = 0: 52 joints, (B,52,3,3) / (B,156).  body_only = 1: the root and the 21 body joints, (B,22,3,3) / (B,66), the hands at
 * the identity — the tokenizer's call; runs the folded path (22-joint skinning, K = 224 blend product), same result up to rounding.
 * betas_dev (B,10) and transl_dev (B,3) may be NULL (zeros); transl is added to vertices and joints.  joints_dev (B,73,3) may be NULL.
 * Arguments are validated before any HIP call (a null handle / pose / verts, B outside [1, max_batch], a flag that is not 0 or 1);
 * the call never allocates and never synchronises: three launches (four with pose2rot) on `stream`, capturable in a graph. */
int  thmr_smplh_forward(thmr_smplh* m, const float* pose_dev, int32_t pose2rot, const float* betas_dev, const float* transl_dev,
                        int32_t body_only, int32_t B, float* verts_dev /*(B,6890,3)*/, float* joints_dev /*(B,73,3) or NULL*/,
                        void* stream);
/* SMPL-H's vector-Jacobian product, both paths: what smplx.SMPLH / SMPLHLayer give under torch autograd.  New symbols
 * under ABI 5: no struct or signature changed.
 * thmr_smplh_grad_reserve, the one-time call: `paths` is a mask of THMR_SMPLH_GRAD_FOLDED (body_only = 1) and THMR_SMPLH_GRAD_FULL.  Per
 * requested path it allocates the backward workspace and builds the transposed copy of that path's blend-shape matrix, (224, 20672) folded
 * and (480, 20672) full — the full copy is 40 MB, so a handle pays only for what it asks for.  It may allocate and synchronise; a path
 * already reserved is skipped.  A handle that never calls it keeps the footprint it had.
 * thmr_smplh_backward takes the inputs of the forward it differentiates (it recomputes the forward's intermediates into the handle's
 * workspace, so forwards issued in between do not matter) and the gradients of the two outputs; a NULL gradient input means zeros, a NULL
 * output is not computed.  grad_pose_dev has the layout of pose_dev, (B,52,3,3) / (B,156) or with body_only (B,22,3,3) / (B,66): the
 * plain derivative by each matrix entry, as autograd gives it.  betas_dev and transl_dev may be NULL, as in the forward.  It never
 * allocates and never synchronises: five launches (seven with pose2rot) on `stream`, capturable in a graph.  No floating-point atomics:
 * every sum has a fixed order, so the result is bit-reproducible and a pose's gradient does not depend on the rest of the batch.
 * THMR_ERR_INVALID (message in thmr_last_error(NULL)) before any launch for a null handle or pose, both gradient inputs null, every output
 * null, B outside [1, max_batch], a pose2rot or body_only that is not 0 or 1, a path that was not reserved. */
#define THMR_SMPLH_GRAD_FOLDED 1
#define THMR_SMPLH_GRAD_FULL 2
int  thmr_smplh_grad_reserve(thmr_smplh* m, int32_t paths);
int  thmr_smplh_backward(thmr_smplh* m, const float* pose_dev, int32_t pose2rot, const float* betas_dev, const float* transl_dev,
                         int32_t body_only, int32_t B, const float* grad_verts_dev /*(B,6890,3) or NULL*/,
                         const float* grad_joints_dev /*(B,73,3) or NULL*/, float* grad_pose_dev /*may be NULL*/,
                         float* grad_betas_dev /*(B,10); may be NULL*/, float* grad_transl_dev /*(B,3); may be NULL*/, void* stream);
/* The tokenizer's reconstruction objective, value and gradient in one call (csrc/loss.hip): PoseReConsLoss
 * (tokenization/utils/losses.py:65-131) with the weighted total of tokenization/train_poseVQ.py:152-156.  Stateless, fp32 contiguous device
 * buffers, two launches, no allocation, no synchronisation; fixed-order two-stage reduction (fp32 partials, fp64 finish) without float
 * atomics, so two runs are bit-equal; the results stay on the device.
 *   pred / gt rotation matrices (B,21,3,3), vertices (B,6890,3), joints (B,73,3); vert_weights (6890,3) or NULL (required by 'wt_l2' on the
 *   mesh); commit: one device float or NULL (zero).  A term whose prediction and ground truth are both NULL is absent: its mean is 0 and
 *   it has no gradient (at least one term is present).  A kind is THMR_RECON_L1 / _L2 / _L1_SMOOTH (torch's L1Loss / MSELoss / SmoothL1Loss,
 *   beta = 1, mean reduction) or _WT_L2 (mean(w (a - b)^2); on the pose and the joints the reference's weights are all ones, so it is _L2
 *   there).  THMR_RECON_GEODESIC and _ROTDIST are refused by name (THMR_ERR_UNSUPPORTED): acos at their clamp has no finite gradient.
 *   The joint term runs over joint rows [joint_lo, joint_hi): [1, 22) for ONLY_VALID_JNT, [0, 73) otherwise.
 *   losses_dev (4): the three unweighted means (pose, mesh, joints) and total = w_total (w_pose pose + w_mesh mesh + w_joint joints +
 *   w_commit commit).  grad_*_dev: the gradient of that TOTAL by the predicted tensor, same shape; any may be NULL.  At the kinks torch's
 *   conventions: l1 gives 0 at a zero difference, l1_smooth is continuous at |d| = 1.  Joints outside the row range get a written zero.
 *   workspace_dev: THMR_TOK_RECON_WS_BASE + B * THMR_TOK_RECON_WS_PER_ITEM floats, written before it is read in every call.
 * Refused before any launch: a null required buffer, B outside [1, 2^16], an unknown kind, a joint range outside
 * 0 <= joint_lo < joint_hi <= 73. */
#define THMR_RECON_L1 0
#define THMR_RECON_L2 1
#define THMR_RECON_L1_SMOOTH 2
#define THMR_RECON_WT_L2 3
#define THMR_RECON_GEODESIC 4
#define THMR_RECON_ROTDIST 5
#define THMR_TOK_RECON_WS_BASE 3
#define THMR_TOK_RECON_WS_PER_ITEM 21
int thmr_tok_recon_loss(const float* pred_rotmat_dev, const float* gt_rotmat_dev, const float* pred_verts_dev, const float* gt_verts_dev,
                        const float* pred_joints_dev, const float* gt_joints_dev, const float* vert_weights_or_null,
                        const float* commit_or_null, int32_t pose_kind, int32_t mesh_kind, int32_t joint_kind, int32_t joint_lo,
                        int32_t joint_hi, double w_pose, double w_mesh, double w_joint, double w_commit, double w_total, int32_t B,
                        float* losses_dev, float* grad_rotmat_or_null, float* grad_verts_or_null, float* grad_joints_or_null,
                        float* workspace_dev, void* stream);
/* out_dev[0] = mean over items b < B and rows row_lo <= i < row_hi of || a[b][i] - b[b][i] ||_2, a and b (B, n_rows_per_item, 3): the three
 * errors of the tokenizer's evaluation (tokenization/utils/eval_poseVQ.py) are this one operator —
 *   calculate_pose_reconstruction_error :47-48   rows of the rotation matrices:  n = 63 (21 matrices x 3 rows), rows [0, 63)
 *   calculate_mesh_reconstruction_error :50-51   vertices:                      n = 6890, rows [0, 6890)
 *   calculate_jnts_reconstruction_error :53-55   body joints 1..21 of 73:       n = 73, rows [1, 22)
 * Fixed-order two-stage fp32 / fp64 reduction without float atomics (two runs are bit-equal); the result stays on the device.
 * workspace_dev: THMR_MEAN_ROW_DIST_WS floats, written before it is read in every call (needs no initialisation).
 * Refused before any HIP call: a null buffer, B < 1, a row range outside 0 <= row_lo < row_hi <= n_rows_per_item, B * n > 2^29. */
#define THMR_MEAN_ROW_DIST_WS 256
int thmr_op_mean_row_dist(const float* a_dev, const float* b_dev, int32_t n_rows_per_item, int32_t row_lo, int32_t row_hi, int32_t B,
                          float* out_dev, float* workspace_dev, void* stream);

/* The forward value of the reference's loss (csrc/loss.hip): TokenHMR.compute_loss (tokenhmr/lib/models/tokenhmr.py:190-277)
 * with its loss modules (losses.py:36-228) for B items, as validation_step runs it straight after forward_step (:421-440).  Stateless, all
 * buffers fp32 device memory and contiguous.  New symbols under ABI 5: no existing struct or signature changed.
 *   mode THMR_VAL_LOSS_PLAIN  the `else` branch (:250-262), what validation runs:
 *        2D   sum conf |pred - gt|                                        (Keypoint2DLoss, L1)
 *        3D   sum conf |(pred - pred[pelvis]) - (gt - gt[pelvis])|          (Keypoint3DLoss)
 *        global_orient / body_pose / betas   sum has (pred - gt)^2 over 9 / 23 x 9 / 10 values per item   (ParameterLoss)
 *   mode THMR_VAL_LOSS_LOOSE  the LOOSE_SUP branch (:214-249), the threshold-adaptive loss with the *PCKT modules:
 *        kp2d_err = conf sum_xy (pred - gt)^2;  valid2d = kp2d_err > kp2d_thresh;  weak2d = conf (1 - valid2d);  the 2D loss uses
 *        conf valid2d, plus loose_weight x the same sum under weak2d;  the 3D confidence becomes conf3d [(valid_3d + conf valid2d) > 0.5];
 *        angle_err = |matrix_to_axis_angle(R_pred R_gt^T)| per joint (losses.py:22-33; thmr_op_rotmat_to_aa's device function);
 *        valid_rot = ((angle_err > angle_thresh) has + valid_3d) != 0;  weak_rot = (1 - valid_rot) has;  the pose terms are
 *        sum valid_rot sum_9 (.)^2 plus loose_weight x the same under weak_rot;  betas uses has_betas x valid_3d and the plain form.
 * The ground-truth pose is (B,72) axis-angle, converted by aa_to_rotmat (thmr_op_aa_to_rotmat's arithmetic, line for line; :235,260), or — with
 * gt_pose_is_rotmat — (B,24,3,3) matrices; joint 0 is global_orient on both sides, so pred_rotmat is exactly thmr_outputs.rotmat.
 * ONE DELIBERATE DEPARTURE: the reference writes into the batch (:223, :227, :240); this call writes into no input.  The values it would
 * have written are the optional outputs conf2d_used, conf3d_used and has_betas_used (loose mode only).
 * Two launches on `stream`, no host synchronisation, no allocation, no float atomics: one wave per item writes five partial sums, one
 * workgroup adds them in fp64 in a fixed order.  Two runs are bit-equal and a captured call replays like the eager one.
 * workspace_dev: THMR_VAL_LOSS_WS_PER_ITEM x B floats, written before they are read in every call (no initialisation needed).
 * Refused before any HIP call (THMR_ERR_INVALID, message in thmr_last_error(NULL)): a null descriptor / input / output struct, a null
 * required input, B outside [1, 2^24], a mode that is not 0 or 1, loose mode without valid_3d, kp2d_thresh or angle_thresh, pelvis_id
 * outside [0, 44), a gt_pose_is_rotmat that is not 0 or 1, a null workspace, gt_keypoints_3d not 16-byte or pred_keypoints_2d not 8-byte
 * aligned (their rows are read as float4 / float2), a `running` that is not 8-byte aligned. */
#define THMR_VAL_LOSS_PLAIN 0
#define THMR_VAL_LOSS_LOOSE 1
#define THMR_VAL_LOSS_WS_PER_ITEM 5
typedef struct thmr_val_loss_desc {
    double w_keypoints_2d, w_keypoints_3d, w_global_orient, w_body_pose, w_betas;   /* cfg.LOSS_WEIGHTS */
    double loose_weight;                                                            /* cfg.MODEL.LOOSE_WEIGHT */
    int32_t pelvis_id;                /* 39 in the reference (25 + 14, :228,253) */
    int32_t mode;                     /* THMR_VAL_LOSS_* */
    int32_t gt_pose_is_rotmat;        /* 0: gt_pose (B,72) axis-angle; 1: (B,24,3,3) rotation matrices */
    int32_t reserved;
} thmr_val_loss_desc;
typedef struct thmr_val_loss_in {
    const float* pred_keypoints_2d;   /* (B,44,2) */
    const float* pred_keypoints_3d;   /* (B,44,3) */
    const float* pred_rotmat;         /* (B,24,3,3) */
    const float* pred_betas;          /* (B,10) */
    const float* gt_keypoints_2d;     /* (B,44,3), confidence last */
    const float* gt_keypoints_3d;     /* (B,44,4), confidence last */
    const float* gt_pose;             /* see gt_pose_is_rotmat */
    const float* gt_betas;            /* (B,10) */
    const float* has_global_orient;   /* (B) */
    const float* has_body_pose;       /* (B) */
    const float* has_betas;           /* (B) */
    const float* valid_3d;            /* (B); loose mode only */
    const float* kp2d_thresh;         /* (44); loose mode only */
    const float* angle_thresh;        /* (24), [0] = global_orient; loose mode only */
} thmr_val_loss_in;
typedef struct thmr_val_loss_out {   /* every pointer may be NULL */
    float* losses;                    /* (6): loss, loss_keypoints_2d, loss_keypoints_3d, loss_global_orient, loss_body_pose, loss_betas */
    float* per_item;                  /* (B,5): the five unweighted terms of every item, in the order of losses[1..5] */
    float* kp2d_err;                  /* (B,44)  loose mode only, like the seven below */
    float* angle_err;                 /* (B,24) */
    float* valid2d;                   /* (B,44) 0 / 1 */
    float* weak2d;                    /* (B,44) */
    float* valid_rot;                 /* (B,24) 0 / 1 */
    float* weak_rot;                  /* (B,24) */
    float* conf2d_used;               /* (B,44) */
    float* conf3d_used;               /* (B,44) */
    float* has_betas_used;            /* (B) */
    double* running;                  /* (7): += the six losses of this call (their fp32 values), [6] += 1 */
} thmr_val_loss_out;
int thmr_val_loss(const thmr_val_loss_desc* desc, const thmr_val_loss_in* in, int32_t B, const thmr_val_loss_out* out,
                  float* workspace_dev, void* stream);
/* The gradient of that loss (csrc/loss.hip): d total / d of what compute_loss reads and, through the projection of
 * forward_step (tokenhmr.py:166-168, 183-185), d total / d (the body model's joints, pred_cam).  `desc` and `in` are thmr_val_loss's, with
 * the same meaning; the total is the weighted SUM over the B items that thmr_val_loss writes to losses[0] (nothing is divided by B).  The
 * masks of the loose mode are recomputed by the forward's own device functions and are constants for the gradient; the L1 terms carry
 * torch's sign(0) = 0.  New symbol under ABI 5: no struct or signature changed.
 * grads_host: a table in HOST memory of THMR_LOSS_GRAD_SLOTS device pointers, indexed by THMR_LOSS_GRAD_*.  A NULL slot is not computed;
 * every other slot is written in full, zeros included:
 *   KP2D   (B,44,2)    by pred_keypoints_2d:  w2d c2 sign(pred - gt), c2 = conf (plain) or conf valid2d + loose_weight weak2d (loose)
 *   KP3D   (B,44,3)    by pred_keypoints_3d:  c_k = w3d conf3d_used sign((p_k - p_pelvis) - (g_k - g_pelvis)), minus sum_k c_k on the pelvis row
 *   JOINTS (B,44,3)    by the body model's joints, KP3D + the projection's adjoint of KP2D: what thmr_smpl_backward takes as grad_joints_dev
 *   CAM    (B,3)       by pred_cam, through t = (cam1, cam2, 2 F / (S cam0 + 1e-9))
 *   ROTMAT (B,24,3,3)  by pred_rotmat, the direct term only:  2 w m (P - G), joint 0 with w_global_orient; m = has (plain) or
 *                      valid_rot + loose_weight weak_rot (loose)
 *   BETAS  (B,10)      by pred_betas, the direct term only:  2 w_betas has_betas (p - g); loose: has_betas valid_3d
 * pred_cam (B,3) device memory or NULL; JOINTS and CAM need it.  The projection is that of thmr_lbs_forward with focal_length
 * (EXTRA.FOCAL_LENGTH) and image_size (MODEL.IMAGE_SIZE): X = pred_keypoints_3d + t, (u, v) = (F / S) X_xy / X_z, with (u, v) read from
 * pred_keypoints_2d, the values the loss saw.
 * One launch on `stream` (one wave per item), no workspace, no allocation, no host synchronisation, no atomics: two runs are bit-equal and
 * a captured call replays like the eager one.
 * Refused before any HIP call (THMR_ERR_INVALID, message in thmr_last_error(NULL)): a null descriptor, input struct or table; what
 * thmr_val_loss refuses of `desc`, `in` and B (a null required input, B outside [1, 2^24], a mode that is not 0 or 1, loose mode without
 * valid_3d, kp2d_thresh or angle_thresh, pelvis_id outside [0, 44), a gt_pose_is_rotmat that is not 0 or 1, gt_keypoints_3d not 16-byte
 * or pred_keypoints_2d not 8-byte aligned); every slot NULL; JOINTS or CAM without pred_cam; with pred_cam, a focal_length or image_size
 * that is not finite and positive. */
#define THMR_LOSS_GRAD_KP2D 0
#define THMR_LOSS_GRAD_KP3D 1
#define THMR_LOSS_GRAD_JOINTS 2
#define THMR_LOSS_GRAD_CAM 3
#define THMR_LOSS_GRAD_ROTMAT 4
#define THMR_LOSS_GRAD_BETAS 5
#define THMR_LOSS_GRAD_SLOTS 6
int thmr_val_loss_grad(const thmr_val_loss_desc* desc, const thmr_val_loss_in* in, const float* pred_cam, double focal_length,
                       double image_size, int32_t B, float** grads_host, void* stream);
/* TokenLoss (losses.py:230-252): CrossEntropyLoss in mean reduction over the rows of an fp32 (rows, 2048) matrix,
 *   out_dev[0] = mean_r (log sum_k exp(x[r][k] - max_r) + max_r - x[r][target[r]]),
 * applied to whatever it is handed — the reference passes the softmax output cls_logits_softmax (rows = B x 160); raw logits work too.
 * target_dev: int32 (rows).  A target outside [0, 2048) is never read through: that row's loss is NaN and so is the mean.
 * One wave per row reads it once (8 float4 per lane); the row losses go to workspace_dev (THMR_TOKEN_CE_WS_PER_ROW x rows floats, written
 * before they are read), one workgroup adds them in fp64 in a fixed order.  Bit-equal between runs, capturable, no host synchronisation.
 * Refused before any HIP call: a null buffer, rows < 1, x_dev not 16-byte aligned. */
#define THMR_TOKEN_CE_WS_PER_ROW 1
int thmr_op_token_ce(const float* x_dev, const int32_t* target_dev, int32_t rows, float* out_dev, float* workspace_dev, void* stream);
/* The HMR pose and shape discriminator and the adversarial terms built on it (csrc/discriminator.hip): Discriminator
 * (tokenhmr/lib/models/discriminator.py:4-99) as tokenhmr.py uses it — loss_adv (:392-394), loss_fake and loss_real (:357-362).  fp32
 * throughout, but for the shape branch (165 multiply-adds per item, accumulated in fp64: column 23 is one short, badly conditioned chain
 * per item, which the loss's gradient multiplies by out - target).  New symbols under ABI 5: no struct or signature changed.  STATELESS: no handle; the weights are one device block of
 * THMR_DISC_WEIGHT_FLOATS floats that the caller holds, 16-byte aligned, in a layout of this library's own (the transposed copies the
 * backward streams are made once, when the block is written; nothing here updates a weight).  The block: these tensors in this order,
 * each starting at a multiple of 64 floats —
 *   D_conv1.weight^T (9,32) | D_conv1.bias (32) | D_conv2.weight^T (32,32) | D_conv2.weight (32,32) | D_conv2.bias (32) |
 *   D_conv1.weight (32,9) | pose_out.j.weight as row j (23,32) | pose_out.j.bias (23) | betas_fc1.weight (10,10) | .bias (10) |
 *   betas_fc2.weight (5,10) | .bias (5) | betas_out.weight (5) | .bias (1) |
 *   fc1 (1024, THMR_DISC_KPAD): D_alljoints_fc1.weight with column j * 32 + c holding the reference's column c * 23 + j (it flattens
 *       channel-major, :91) and columns 736 .. 767 zero | D_alljoints_fc1.bias (1024) | the first 736 columns of fc1 transposed (736,1024) |
 *   D_alljoints_fc2.weight (1024,1024) | .bias (1024) | its transpose (1024,1024) | D_alljoints_out.weight (1024) | .bias (1).
 * poses_dev: (B,23,3,3) with pose_stride floats between items (>= 207; 216 for the body_pose view of a (B,24,3,3) buffer, which needs no
 * copy); read as scalars, 4-byte alignment suffices.  betas_dev: (B,10).  out (B,25): columns 0..22 the per-joint heads (:77-81), 23 the
 * shape branch (:84-88), 24 the all-joints branch (:91-96).
 * The loss is L(target) = sum_{b,c} (out[b][c] - target)^2 / loss_div: loss_div = the batch size the loss is a mean over (:358,393), 0 = B
 * (a caller that splits a batch over several calls passes the whole batch's size and adds the calls' values).
 * bufs_host: a table in HOST memory of THMR_DISC_SLOTS device pointers, indexed by THMR_DISC_*:
 *   OUT         (B,25)        forward: required; backward: optional
 *   LOSS        one float     optional: L(target), summed in fp64 in a fixed order
 *   GRAD_POSES  (B,23,3,3)    backward only: d/d poses, contiguous, written in full
 *   GRAD_BETAS  (B,10)        backward only: d/d betas; either gradient may be NULL and is then not computed, not both
 *   WORKSPACE   THMR_DISC_WS_PER_ITEM x B floats, 16-byte aligned, required; every word that is read was written earlier in the same
 *               call, so it needs no initialisation (the zero columns of fc1's padded operand included)
 * thmr_disc_forward: four launches on `stream`, five with LOSS: the per-joint front, shape branch and heads (one workgroup per item);
 * two skinny GEMMs with bias + ReLU that stream the wide weights once (K = 736 is padded to THMR_DISC_KPAD); the read-out (one wave per
 * item); the loss sum.
 * thmr_disc_backward: the gradient of sum(out * grad_out) with grad_out_or_null (B,25) given, else of L(target), by the INPUTS (there
 * is no gradient by the weights).  It keeps no activations between calls: it runs the forward again into the workspace — so it needs no
 * preceding forward, and OUT / LOSS of the same call are that forward's, bit-equal to thmr_disc_forward's — then two skinny GEMMs on the
 * transposed weights (the first with the ReLU mask as its epilogue) and the front's backward: eight launches, nine with LOSS.  ReLU's
 * derivative is torch's, zero at z <= 0.  Without GRAD_POSES the wide layers are only run when OUT or LOSS is asked for.
 * Both: no float atomics, no allocation, no host synchronisation; two runs are bit-equal and a captured call replays like the eager one.
 * Refused before any HIP call (THMR_ERR_INVALID, message in thmr_last_error(NULL)): a null weights_dev, poses_dev, betas_dev or table; a
 * null WORKSPACE; forward without OUT; backward with GRAD_POSES and GRAD_BETAS both NULL; B outside [1, THMR_DISC_MAX_BATCH]; loss_div < 0;
 * pose_stride < 207; weights_dev or WORKSPACE not 16-byte aligned (their rows are read as float4); a target that is not finite where it
 * is read (LOSS given, or backward without grad_out_or_null). */
#define THMR_DISC_OUT 0
#define THMR_DISC_LOSS 1
#define THMR_DISC_GRAD_POSES 2
#define THMR_DISC_GRAD_BETAS 3
#define THMR_DISC_WORKSPACE 4
#define THMR_DISC_SLOTS 5
#define THMR_DISC_MAX_BATCH 256
#define THMR_DISC_KPAD 768
#define THMR_DISC_WEIGHT_FLOATS 3644480
#define THMR_DISC_WS_PER_ITEM 5665
int thmr_disc_forward(const float* weights_dev, const float* poses_dev, int64_t pose_stride, const float* betas_dev, int32_t B,
                      int32_t loss_div, double target, float** bufs_host, void* stream);
int thmr_disc_backward(const float* weights_dev, const float* poses_dev, int64_t pose_stride, const float* betas_dev,
                       const float* grad_out_or_null, int32_t B, int32_t loss_div, double target, float** bufs_host, void* stream);

/* Evaluation metrics right after the hot path — stateless, all buffers device-side.
 * Replaces compute_similarity_transform / eval_pose and the arithmetic of Evaluator.__call__
 * (tokenhmr/lib/utils/pose_utils.py:61-143, :201-275): pelvis alignment, MPJPE, PA-MPJPE (3x3 SVD Procrustes), PVE, in mm.
 *   pred_joints (B,n_joints,3); gt_joints (B,n_joints,gt_stride) (gt_stride = 4 for batch['keypoints_3d'] with its confidence column)
 *   pelvis_mode 0: joint pelvis_ind; 1: (joint1 + joint2)/2 (EMDB branch); any other value is refused.  verts may be NULL (no PVE).
 *   pelvis_scratch (B,6) receives [pred_pelvis | gt_pelvis].
 *   Refused before any HIP call: a null buffer, n_kp outside [1, 64], gt_stride < 3, B < 1, n_joints < 3, pelvis_ind outside
 *   [0, n_joints), pelvis_mode outside {0, 1}, and n_verts < 1 when pred_verts, gt_verts and pve_mm are all given (both vertex
 *   buffers are (B,n_verts,3)).  A kp_list entry outside [0, n_joints) is never read through: that crop's mpjpe and re are NaN. */
int thmr_eval_pose(const float* pred_joints_dev, const float* gt_joints_dev, int32_t n_joints, int32_t gt_stride,
                   const int32_t* kp_list_dev, int32_t n_kp, int32_t pelvis_ind, int32_t pelvis_mode,
                   const float* pred_verts_dev, const float* gt_verts_dev, int32_t n_verts, int32_t B,
                   float* mpjpe_mm_dev, float* re_mm_dev, float* pve_mm_dev, float* pelvis_scratch_dev, void* stream);
/* joints = J (n_joints,n_verts) @ verts (B,n_verts,3): J_regressor_24_SMPL of the EMDB branch (pose_utils.py:212,219) */
int thmr_regress_joints(const float* J_dev, const float* verts_dev, int32_t n_joints, int32_t n_verts, int32_t B,
                        float* out_dev, void* stream);

/* Crop preprocessing right before the hot path: decoded uint8 frame on the device + one affine per crop ->
 * normalised (n,3,patch,patch) fp32 = batch['img'].  Replaces, per crop, the reference's CPU-side
 *   skimage.filters.gaussian anti-alias of the whole frame   tokenhmr/lib/datasets/vitdet_dataset.py:62-68, utils.py:583-587
 *   cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT)            tokenhmr/lib/datasets/utils.py:351-356 (generate_image_patch_cv2)
 *   [:, :, ::-1], HWC->CHW float32, (x - mean)/std           vitdet_dataset.py:75-80, utils.py:599-617
 * with OpenCV's fixed-point bilinear and scipy's correlate1d arithmetic reproduced exactly (csrc/crop.hip).  The affine itself
 * (gen_trans_from_patch_cv + cv2.getAffineTransform, utils.py:81-128) is 3 points of host arithmetic and stays with the caller
 * (tokenhmr_amd/preprocess.py mirrors ViTDetDataset).
 *   M       forward 2x3 matrix exactly as passed to cv2.warpAffine (src -> dst), row-major
 *   sigma   gaussian sigma of the anti-alias blur applied before the warp, 0 = none; truncate: 4.0 (vitdet) / 3.0 (get_example)
 *   frame   (H, W, 3) uint8, row_stride bytes per row; swap_rb = 1 flips the channel order (BGR frame -> RGB planes)
 *   mean/std  in 0..255 units, indexed by OUTPUT channel.
 * The handle owns grow-only device scratch for the blurred regions; growing it synchronises the stream.
 * thmr_cropper_run refuses with THMR_ERR_INVALID, before any HIP call: a null buffer, H, W, n or patch <= 0, patch > 4096,
 * row_stride < W * 3, a frame side above 32767 (the warp's 16-bit texel coordinates), a singular or non-finite affine, a negative or
 * non-finite sigma, truncate <= 0, and a blur radius above 4096: anything but truncate * sigma + 0.5 < 4097, compared in double,
 * so an infinite or NaN product is refused too. */
typedef struct thmr_crop_desc {
    double M[6];
    double sigma;
    double truncate;
} thmr_crop_desc;
typedef struct thmr_cropper thmr_cropper;
int  thmr_cropper_create(int32_t device, thmr_cropper** out);
void thmr_cropper_destroy(thmr_cropper* c);
const char* thmr_cropper_last_error(const thmr_cropper* c);
int  thmr_cropper_run(thmr_cropper* c, const uint8_t* frame_dev, int32_t H, int32_t W, int64_t row_stride,
                      const thmr_crop_desc* crops_host, int32_t n, int32_t patch, int32_t swap_rb, const float* mean_host,
                      const float* std_host, float* out_dev, void* stream);

/* A batch of crops from a TABLE of frames (the eval.py shape: n items, n decoded frames of n sizes, one crop each), in one call:
 * one descriptor copy and at most three launches (rows pass, columns pass, warp); each workgroup takes frame pointer, geometry and
 * window origin from its item's descriptor.  The arithmetic is thmr_cropper_run's: item i is bit-equal to thmr_cropper_run on that
 * item's full frame alone.
 * An item need not bring its whole frame, only a WINDOW of it that covers what the crop can touch:
 *   un-blurred  the fixed-point source coordinates of the four patch corners (the value thmr_cropper_run's warp computes, >> 10),
 *               [lo - 1, hi + 2] on each axis, clipped to the frame;
 *   blurred     that box widened by the kernel radius lw = int(truncate * sigma + 0.5) on all four sides, clipped to the frame;
 *   an empty box means every output pixel is border: nothing of that item's window is read and win_dev may be null.
 * tokenhmr_amd.preprocess.source_window restates the rule.  Refused with THMR_ERR_INVALID and the item's index in
 * thmr_cropper_last_error, before any HIP call: a window that does not lie inside the frame or does not cover the box, a null
 * pointer where the box is not empty, row_stride < win_w * 3, a frame side above 32767 (the warp's 16-bit texel coordinates), and
 * what thmr_cropper_run refuses.  The arguments are checked before the handle, so the refusals need no device. */
typedef struct thmr_frame_crop {
    const uint8_t* win_dev;     /* device pointer to a WINDOW of this item's decoded frame, (win_h, win_w, 3) uint8 */
    int64_t  row_stride;        /* bytes per window row, >= win_w * 3 */
    int32_t  H, W;              /* size of the FULL frame: the zero-border and edge-replication rules use these */
    int32_t  win_x0, win_y0, win_w, win_h;   /* where the window sits in the frame; (0,0,W,H) = the whole frame */
    double   M[6], sigma, truncate;          /* as thmr_crop_desc */
} thmr_frame_crop;
int  thmr_cropper_run_frames(thmr_cropper* c, const thmr_frame_crop* items_host, int32_t n, int32_t patch, int32_t swap_rb,
                             const float* mean_host, const float* std_host, float* out_dev /* (n,3,patch,patch) */, void* stream);

/* Mesh renderer: the reference's pyrender scenes (tokenhmr/lib/utils/renderer.py) rasterised on the device
 * (csrc/render.hip).  The kernels know no presets: the host scene builder (tokenhmr_amd/render.py) fills the descriptor.
 *   camera frame   x right, y down, z forward (the frame of perspective_projection); per mesh m
 *                  translate_first = 0: p = R v + t_m   (Renderer.__call__: R = the side-view rotation)
 *                  translate_first = 1: p = R (v + t_m) (vertices_to_trimesh / render_rgba*: R = the rot_axis / rot_angle rotation)
 *   projection     u = fx X/Z + cx, v = fy Y/Z + cy; pixel (row i, col j) covers [j, j+1) x [i, i+1)
 *   coverage       1 sample (pixel centre) or 4 (rotated grid (0.375,0.125) (0.875,0.375) (0.125,0.625) (0.625,0.875)); vertices
 *                  snapped to 1/256 px, exact integer edge functions, top-left rule; back faces (clockwise in the image frame, i.e.
 *                  GL's clockwise-in-window after the y flip) and degenerate faces culled; a face with a vertex at Z < znear or
 *                  projecting beyond 2^21 px is rejected (no clipping)
 *   visibility     per sample the smallest (fp32 depth, mesh, face); deterministic
 *   shading        glTF metallic-roughness, smooth angle-weighted normals, once per (pixel, distinct winning face) at the centre
 *   output         rgb = (sum shaded + (S - k) bg) / S, alpha = k / S, each rounded to 8 bits; (n_img, H, W, out_channels) fp32
 *   mode           THMR_RENDER_PER_IMAGE: N images, image m holds mesh m; THMR_RENDER_ONE_IMAGE: one image holding all N meshes
 * Lights are in the camera frame: a directional light's vec is the direction it travels, a point light's vec its position
 * (radiance color * intensity / distance^2).  thmr_renderer_run arguments: verts_dev (N, V, 3) and cam_t_dev (N, 3) fp32 device;
 * bg_dev NULL, or (n_img, 3, H, W) normalised images composited as Renderer.__call__ does (out = rgb a + (1 - a) (x std + mean),
 * out_channels 3); out_dev (n_img, H, W, out_channels).  The handle grows device scratch at a new, larger size (and synchronises the
 * stream then); otherwise a call allocates nothing and does not synchronise. */
#define THMR_RENDER_MAX_LIGHTS 16
#define THMR_RENDER_PER_IMAGE 0
#define THMR_RENDER_ONE_IMAGE 1
#define THMR_LIGHT_DIRECTIONAL 0
#define THMR_LIGHT_POINT 1
typedef struct thmr_render_light {
    int32_t type;               /* THMR_LIGHT_DIRECTIONAL / THMR_LIGHT_POINT */
    float vec[3];               /* direction of travel / position, camera frame */
    float color[3];
    float intensity;
} thmr_render_light;
typedef struct thmr_render_desc {
    int32_t width, height;      /* 1 ... 8192 */
    float fx, fy, cx, cy;
    float znear;                /* > 0 */
    int32_t samples;            /* 1 or 4 */
    int32_t mode;               /* THMR_RENDER_PER_IMAGE / THMR_RENDER_ONE_IMAGE */
    int32_t translate_first;
    float rot[9];               /* R, row-major */
    float base_color[3];        /* every mesh's base colour ... */
    const float* mesh_colors;   /* ... or per mesh: host (N, 3), NULL = base_color */
    float bg_color[3];          /* background, alpha 0 */
    float metallic, roughness;
    float ambient[3];           /* ambient light; the shaded colour gains ambient * base */
    int32_t n_lights;           /* 0 ... THMR_RENDER_MAX_LIGHTS */
    thmr_render_light lights[THMR_RENDER_MAX_LIGHTS];
    int32_t out_channels;       /* 3 or 4 */
    float img_mean[3], img_std[3];   /* de-normalisation of bg_dev */
    uint32_t* ids_dev;          /* optional (n_img, H, W, samples) device: winning mesh * F + face per sample, 0xFFFFFFFF = none */
} thmr_render_desc;
typedef struct thmr_renderer thmr_renderer;
/* faces_host (F, 3) int32, every index in [0, V); builds the vertex -> face lists once (needs the device) */
int  thmr_renderer_create(int32_t device, const int32_t* faces_host, int32_t F, int32_t V, thmr_renderer** out);
void thmr_renderer_destroy(thmr_renderer* r);
const char* thmr_renderer_last_error(const thmr_renderer* r);
int  thmr_renderer_run(thmr_renderer* r, const thmr_render_desc* desc, const float* verts_dev, const float* cam_t_dev, int32_t N,
                       const float* bg_dev, float* out_dev, void* stream);

/* Contact sheet: the reference's MeshRenderer.visualize / visualize_tensorboard (tokenhmr/lib/utils/mesh_renderer.py,
 * render_openpose.py) as one canvas, in two launches on `stream`.  Per person the tiles are, in this order, those requested in
 * `panels` (the image; the front and the side render under the hard mask out = alpha > 0.8 ? rgb : bg, bg = the image / ones) and one
 * skeleton panel per keypoint set given (predicted, then ground truth).  Tiles are laid out as torchvision's make_grid(nrow, padding)
 * does, pad value 0: xmaps = min(nrow, tiles), ymaps = ceil(tiles / xmaps), canvas (3, ymaps (H + padding) + padding,
 * xmaps (W + padding) + padding) fp32 planes, tile k at row padding + (k / xmaps)(H + padding), column padding + (k % xmaps)(W + padding).
 *   images_dev   (n, 3, H, W) fp32, values in 0 ... 1           front_dev / side_dev   (n, H, W, 4) fp32 RGBA of thmr_renderer_run
 *   pred_kp_dev  (n, 44, 2) fp32 or NULL: normalised keypoints, confidence 1; pixel = img_res (k + 0.5) in fp32; body keypoints 1 ... 14
 *                take the matching ones of the 19 extra keypoints
 *   gt_kp_dev    (n, 44, 3) fp32 or NULL: x, y, confidence; scaled the same way and remapped where the extra keypoint has confidence > 0
 *                and the body one confidence 0 — IN PLACE, as the reference does on its caller's array
 *   records_dev  ((pred ? n : 0) + (gt ? n : 0), THMR_SHEET_RECORDS, THMR_SHEET_RECORD_WORDS) int32, 16-byte aligned; required with
 *                keypoints.  The draw list of render_openpose per skeleton, in draw order: 24 limbs, then 25 joints; a record is
 *                {kind (0 = not drawn, 1 = line, 2 = circle), x0, y0, x1, y1, radius, thickness, colour index, box x0, y0, x1, y1}.
 *                Written by the first launch, read by the second; the caller may read it back.
 * A draw-list entry is what render_openpose passes to cv2 (same integer points, radius, thickness, colour, order), except that an
 * entry with a coordinate beyond +-16384 (or non-finite) is not drawn.  Coverage: integer point (x, y) is the centre of pixel column x,
 * row y; a line of thickness t covers the pixels within t / 2 of the closed segment; a circle of radius r and thickness k > 0 the
 * pixels at distance d with (2r - k)^2 <= 4 d^2 <= (2r + k)^2 (no lower bound when 2r <= k), k < 0 the disc d <= r; later entries
 * overwrite earlier ones.  A covered pixel is colour / 255, any other fl(fl(255 x) / 255) of the image.
 * Nothing is allocated and nothing synchronises; two calls give identical bits. */
#define THMR_SHEET_IMAGE 1
#define THMR_SHEET_FRONT 2
#define THMR_SHEET_SIDE 4
#define THMR_SHEET_KEYPOINTS 44
#define THMR_SHEET_RECORDS 49
#define THMR_SHEET_RECORD_WORDS 12
typedef struct thmr_sheet_desc {
    int32_t n;                  /* people, >= 1 */
    int32_t width, height;      /* of every image and render, 1 ... 8192 */
    int32_t img_res;            /* keypoint scale (MODEL.IMAGE_SIZE), 1 ... 8192 */
    int32_t panels;             /* THMR_SHEET_IMAGE | THMR_SHEET_FRONT | THMR_SHEET_SIDE */
    int32_t nrow, padding;      /* make_grid's */
    int32_t canvas_width, canvas_height;   /* of canvas_dev; must equal the size stated above */
} thmr_sheet_desc;
int  thmr_renderer_sheet(thmr_renderer* r, const thmr_sheet_desc* desc, const float* images_dev, const float* front_dev,
                         const float* side_dev, const float* pred_kp_dev, float* gt_kp_dev, int32_t* records_dev, float* canvas_dev,
                         void* stream);

/* ---- data-parallel collectives for hosts without torch.distributed ----
 * The reference has no collective on this path (inference is single-device, tokenhmr/eval.py:52-54).  Crops shard with NO data-path
 * collective; two collectives surround the path: ONE broadcast of the packed weight arena at start-up (only rank `root` read the
 * checkpoint; follow it with thmr_finalize_weights(assume_all_loaded = 1) on the receivers) and ONE all-gather per batch of the packed
 * per-crop records.  `nccl_comm` is an ncclComm_t the caller created (ncclCommInitRank) with the RCCL already loaded in the process;
 * the library resolves ncclBroadcast / ncclAllGather from that copy at first use (it does not link its own).  Asynchronous on `stream`.
 *   record = [pred_vertices 20670 | pred_keypoints_3d 132 | pred_keypoints_2d 88 | rotmat 216 | betas 10 | pred_cam 3 | pred_cam_t 3 |
 *             token_idx 160 (int32 bits)] = THMR_RECORD_WORDS 32-bit words per crop (85,128 B).  token_idx may be NULL (an engine with
 *             THMR_CFG_HEAD_HMR2 has none): its 160 words are then zero; every other field is required. */
#define THMR_RECORD_WORDS 21282
int thmr_pack_records(const thmr_outputs* out, int32_t B, float* rec_dev /*(B, THMR_RECORD_WORDS)*/, void* stream);
int thmr_bcast_weights(thmr_engine* e, void* nccl_comm, int32_t root, void* stream);
/* every rank contributes `rows` records (pad to the largest shard); recv_dev is (world * rows, THMR_RECORD_WORDS) in rank order */
int thmr_allgather_records(void* nccl_comm, const float* rec_dev, int32_t rows, float* recv_dev, void* stream);
const char* thmr_collective_last_error(void);

/* Built-in profiler: HIP events recorded on the launch stream around each kernel class.
 * on = 0 off, 1 every class, 2 only the four ViT GEMM classes, 3 only fc1 (the dominant kernel), sampled.  An event pair costs ~2-3 us
 * of stream time: 128 pairs per call (on = 2) were 0.75 % of a B = 64 step and 20 % of a B = 1 call (round 3: the facade call
 * without events was FASTER than the timed loop), which is why bench.py times with on = 3, which samples every 4th fc1 launch (8 pairs per call; all 32 launches have one shape). */
/* How the four ViT GEMMs (qkv / proj / fc1 / fc2: 97 % of the path's arithmetic), the ViT attention and the decoder's to_kv GEMM multiply.
 * Both modes are fp32 in, fp32 accumulate, fp32 out.
 *   1 (DEFAULT, ABI 4): "split3" — each fp32 operand as three bf16 pieces, six bf16 MFMA products per element pair, fp32 accumulation
 *      (csrc/gemm_split16.hip, attention_b16.hip; v_mfma_f32_16x16x32_bf16).  fp32-GRADE, not bitwise fp32: the measured error against an
 *      fp64 product is no larger than the exact-fp32 kernel's (tests/test_gpu_ops.py::test_gemm_split3), at ~1.55x its rate end to end.
 *      It is what bench.py's `value`, the facade (tokenhmr_amd.model.load_tokenhmr) and every parity claim of the default path refer to:
 *      0 of 40,960 pose-token indices differ from the reference's on the four 64-crop fixtures, joints / vertices within
 *      max(0.1 mm, 2 x the reference's own fp32-vs-fp64 distance) (tests/test_gpu_model.py).  Applies to calls of at least 3 crops (one
 *      and two crops run the exact-fp32 kernels in either mode).  Four ranges, a crop's result is batch-independent within each: 3 and 4
 *      crops split the K sums of proj and fc2 four ways, 5 ... 15 two ways, 16 ... 31 only fc2's (two ways), 32 and more neither.
 *      LayerNorm, the epilogues and the rest of the head are fp32 arithmetic in both modes.
 *   0 (opt-out): exact-fp32 MFMA (v_mfma_f32_32x32x2_f32 / 16x16x4_f32) everywhere — bitwise an fmaf chain.
 * Mode 1 needs the engine-owned split3 copy of the ViT weights (1.5x their fp32 bytes) and the operand buffers (+ the partial-sum planes
 * of its split-K ranges): built by thmr_finalize_weights while the mode is on (i.e. by default) or by thmr_set_vit_gemm(1) on finalized
 * weights, kept until thmr_destroy (setting 0 does not free them).  An engine created with max_batch < 3 never runs the mode and builds
 * nothing.  Like thmr_forward the switch allocates nothing per call, so a call in either mode can be captured in a hipGraph.
 * Returns 0 / negative; thmr_get_vit_gemm returns the mode. */
int thmr_set_vit_gemm(thmr_engine* e, int32_t mode, void* stream);
int thmr_get_vit_gemm(thmr_engine* e);
int thmr_prof_enable(thmr_engine* e, int32_t on);
int thmr_prof_collect(thmr_engine* e, thmr_prof_entry* entries /*[THMR_PROF_NUM]*/, int32_t reset);

/* Baseline JPEG decoding for the evaluation datasets (csrc/jpeg.hip, jpeg_host.h, jpeg_math.h): new symbols under ABI 5.
 * A hybrid: the host parses the markers and decodes the Huffman stream — the sequential part — into quantised coefficient blocks, only
 * for the MCU rows and blocks a WINDOW of the frame needs; the device dequantises, runs the inverse DCT, upsamples the chroma and converts
 * the colour, for that window only, straight into the (win_h, win_w, 3) uint8 buffer thmr_cropper_run_frames takes.  The arithmetic is
 * libjpeg's default pipeline restated in integers, bit for bit: the JDCT_ISLOW inverse DCT (13-bit constants, PASS1_BITS 2), h2v1 / h2v2
 * "fancy" triangle upsampling with the edges replicated at the TRUE downsampled component size (plain replication where that width is
 * at most 2, as libjpeg chooses), and the 16-bit fixed-point YCbCr -> RGB tables.
 *   supported     SOF0 (baseline sequential DCT), Huffman, 8 bits, ONE interleaved scan; 1 component (grey, replicated to 3 channels) or
 *                 3 (YCbCr) with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1; DRI / RSTn; 0xFF00 stuffing; up to four Huffman and four
 *                 quantisation tables, redefined between markers; APPn / COM skipped
 *   unsupported   THMR_ERR_UNSUPPORTED, the message names what was found: every other SOF (progressive, extended, lossless, arithmetic),
 *                 DAC, another sample precision, 4 components, Adobe APP14 transform 0 or component ids 'R','G','B' with 3 components,
 *                 a scan that does not hold every component (multi-scan), other sampling factors, a side above 32767, height 0 (DNL)
 *   malformed     THMR_ERR_INVALID: never a read outside [data, data + len), never an unbounded loop (every Huffman symbol is at most
 *                 16 + 15 bits, and a block that consumed bits past the last entropy-coded byte ends the decode)
 * The host entry points need no device, are re-entrant and keep no state; their message is in thmr_last_error(NULL) (thread-local). */
typedef struct thmr_jpeg_info {
    int32_t height, width, components;  /* components: 1 or 3 where supported, else what the frame header says */
    int32_t h_samp, v_samp;             /* luma sampling factors (1,1) (2,1) (2,2); (1,1) for grey */
    int32_t restart_interval;           /* MCUs between RSTn markers, 0 = none */
    int32_t supported;                  /* 1, or 0 with the reason in thmr_last_error(NULL) */
    int32_t reserved;
} thmr_jpeg_info;
/* What thmr_jpeg_entropy_decode kept.  Component c's blocks are the rectangle [bx0, bx0 + bw) x [by0, by0 + bh) of its 8x8-block grid,
 * stored row-major from block index coef_block[c] of the coefficient buffer, 64 int16 each: QUANTISED values in natural (row-major,
 * zig-zag undone) order.  The rectangles cover the window's samples, for sub-sampled chroma widened by the one sample on each side that
 * fancy upsampling reads, clipped to the component's true size. */
typedef struct thmr_jpeg_plan {
    int32_t height, width, components, h_samp, v_samp;
    int32_t win_x0, win_y0, win_w, win_h;       /* the window the plan was made for */
    int32_t mcu_row0, mcu_rows_kept;            /* MCU rows that hold kept blocks */
    int32_t mcu_rows_decoded;                   /* MCU rows entropy-decoded, those above the window (decoded and discarded) included */
    int32_t bx0[3], by0[3], bw[3], bh[3], coef_block[3];
    int32_t n_blocks;                           /* blocks in the coefficient buffer */
    uint16_t quant[3][64];                      /* each component's quantisation table, natural order */
} thmr_jpeg_plan;
int thmr_jpeg_probe(const uint8_t* data, size_t len, thmr_jpeg_info* info);
/* window: {x0, y0, w, h} inside the frame (an empty one keeps nothing), NULL = the whole frame.  coef NULL: only the plan is filled
 * (the size: n_blocks * 64 int16) and nothing is entropy-decoded; otherwise coef_capacity_blocks >= plan->n_blocks blocks are written.
 * MCU rows above the window are decoded and discarded; decoding stops after the last MCU row the window needs. */
int thmr_jpeg_entropy_decode(const uint8_t* data, size_t len, const int32_t* window, int16_t* coef, int64_t coef_capacity_blocks,
                             thmr_jpeg_plan* plan);
/* The full decode of a window on the CPU, with the kernels' arithmetic (shared __host__ __device__ functions, csrc/jpeg_math.h):
 * out (win_h, win_w, 3) uint8 host, row_stride >= win_w * 3 bytes per row, bytes beyond win_w * 3 of a row untouched; bgr = 1 writes
 * B, G, R (cv2.imread), 0 R, G, B (PIL). */
int thmr_jpeg_decode_host(const uint8_t* data, size_t len, const int32_t* window, int32_t bgr, uint8_t* out, int64_t row_stride);
/* The device half.  The handle owns two grow-only sets of staging (pinned host + device), used alternately, and device scratch for the
 * component planes.  thmr_jpeg_decode_batch decodes n items of n sizes and formats with ONE packed upload and TWO launches (inverse
 * DCT of every block of the batch; upsampling + colour of every window).  A staging set is rewritten only after the event behind its
 * last use — two calls back — has completed; beyond that the call synchronises only when a buffer grows (never inside a
 * stream capture: THMR_ERR_STATE then — run the call once at those sizes first; a captured call keeps reading its staging set, so
 * give it a handle of its own).  Every argument is checked before the handle and the handle before any HIP call: n <= 0, a null table,
 * and per item (the message names its index) a null plan / coefficients, a window outside the frame or other than the plan's frame,
 * row_stride < win_w * 3, a null out_dev with a non-empty window, a plan whose block rectangles do not cover the window or lie outside
 * the component.  Bytes of out_dev beyond win_w * 3 of a row are not written. */
typedef struct thmr_jpeg_item {
    const int16_t* coef;                /* host: plan->n_blocks * 64 int16 */
    const thmr_jpeg_plan* plan;         /* host */
    int32_t win_x0, win_y0, win_w, win_h;
    uint8_t* out_dev;                   /* device: (win_h, win_w, 3) uint8 */
    int64_t row_stride;                 /* bytes per output row, >= win_w * 3 */
} thmr_jpeg_item;
typedef struct thmr_jpeg thmr_jpeg;
int  thmr_jpeg_create(int32_t device, thmr_jpeg** out);
void thmr_jpeg_destroy(thmr_jpeg* j);
const char* thmr_jpeg_last_error(const thmr_jpeg* j);
int  thmr_jpeg_decode_batch(thmr_jpeg* j, const thmr_jpeg_item* items_host, int32_t n, int32_t bgr, void* stream);

/* PNG encoding of device images: the counterpart of cv2.imwrite(".png") (csrc/png.hip, png_host.h, png_math.h): new symbols
 * under ABI 5.  Everything is integer arithmetic and deterministic: the bytes of a file are a function of the pixels and the arguments
 * only, and thmr_png_encode_host — the same algorithm on the CPU, sharing its arithmetic and selection rules with the kernels through
 * __host__ __device__ functions — writes the same file byte for byte.
 *   pixels        uint8 or float32, 1 / 3 / 4 channels, any ELEMENT strides (stride_y, stride_x, stride_c): HWC, CHW, a panel of a sheet.
 *                 swap_rb reverses the first three channels of a 3 / 4-channel image (cv2 hands over BGR(A), the file holds RGB(A)).
 *                 float32 is multiplied by `scale` in fp32 (one rounding) and converted by `rounding`: THMR_PNG_ROUND_NEAREST rounds to
 *                 nearest even and saturates to [0, 255] (cv2's saturate_cast<uchar>); THMR_PNG_ROUND_TRUNC clamps to [0, 255] and
 *                 truncates (np.clip(x, 0, 255).astype(np.uint8)).  NaN gives 0 in both, +-inf saturate.  uint8 ignores both.
 *   file          signature, IHDR (8 bits; grey, RGB or RGBA; no interlace), ONE IDAT, IEND.  Each row takes the filter 0 ... 4 with the
 *                 smallest sum of |residual as a signed byte| (libpng's default heuristic), ties to the lowest number; row 0 sees a zero
 *                 previous row.  The zlib stream is 78 01, then the filtered stream cut into segments of thmr_png_segment_bytes() bytes,
 *                 each compressed alone — LZ77 with matches that never reach behind the segment start, one fixed-Huffman block, and
 *                 (but for the last) an empty stored block 00 00 FF FF back to a byte boundary; a segment whose coded form would be
 *                 larger than a stored block is a stored block — then the Adler-32.  No file is larger than thmr_png_bound().
 *   compression   THMR_PNG_FIXED writes the file above.  THMR_PNG_DYNAMIC keeps the filters, the segments and the LZ77 tokens, and gives
 *                 a segment ONE dynamic-Huffman block where that takes strictly fewer bits than the fixed block, header included.  The
 *                 block rule (csrc/png_math.h): the tokens' literal / length and distance symbols are counted with one end-of-block, a
 *                 distance alphabet with fewer than two symbols in use is padded to two; optimal code lengths limited to 15 bits (7 for
 *                 the code-length alphabet) by thmr_png_code_lengths, ties to the lower symbol index; canonical codes (RFC 1951
 *                 3.2.2); HLIT, HDIST and HCLEN trimmed; the lengths run-length coded greedily with the symbols 16, 17 and 18.  The
 *                 stored-block rule then applies to the winner, so thmr_png_bound() holds in both modes.
 *   refused       before any HIP call, the message names the item: THMR_ERR_UNSUPPORTED for a 16-bit dtype and for 2 channels;
 *                 THMR_ERR_INVALID for any other dtype / channel count / rounding, width or height < 1, a filtered stream of 2^31 bytes
 *                 or more, a compression other than the two named, a null pointer, and a capacity below thmr_png_bound(). */
enum { THMR_PNG_U8 = 0, THMR_PNG_F32 = 1, THMR_PNG_U16 = 2 /* refused by name */ };
enum { THMR_PNG_ROUND_NEAREST = 0, THMR_PNG_ROUND_TRUNC = 1 };
enum { THMR_PNG_FIXED = 0, THMR_PNG_DYNAMIC = 1 };
typedef struct thmr_png_item {
    const void* pixels;                 /* element (0, 0, 0): device memory for thmr_png_encode_batch, host for thmr_png_encode_host */
    int32_t dtype;                      /* THMR_PNG_U8 / THMR_PNG_F32 */
    int32_t width, height, channels;
    int64_t stride_y, stride_x, stride_c;       /* in ELEMENTS */
    float scale;                        /* float32 input only */
    int32_t rounding;                   /* THMR_PNG_ROUND_* */
    int32_t swap_rb;
    int32_t compression;                /* THMR_PNG_FIXED / THMR_PNG_DYNAMIC (the field was `reserved`, 0: a caller that zeroed it gets the fixed mode) */
    uint8_t* out;                       /* host: the file */
    int64_t capacity;                   /* bytes at out, >= thmr_png_bound(width, height, channels) */
    int64_t written;                    /* set by the call: the file's length */
} thmr_png_item;
int thmr_png_segment_bytes(void);
/* raw + 5 bytes per segment + 6 zlib bytes + 57 container bytes; 0 for arguments the encoder refuses */
int64_t thmr_png_bound(int32_t width, int32_t height, int32_t channels);
int thmr_png_encode_host(thmr_png_item* item);
/* The code lengths of the dynamic mode, the very routine the kernels run: lens[s] for n <= 286 symbols with frequencies freq[s] (0 ...
 * 2^22 - 1), optimal under the limit max_bits (1 ... 15, with 2^max_bits >= the symbols in use), 0 where the frequency is 0; one
 * symbol in use gets length 1.  Host only.  THMR_ERR_INVALID for a null pointer or an argument outside these ranges. */
int thmr_png_code_lengths(const int32_t* freq, int32_t n, int32_t max_bits, int32_t* lens);
/* The handle owns grow-only device scratch (filtered stream, one slot per segment, the packed streams) and pinned staging.  One call
 * encodes n images of n sizes, dtypes and layouts with ONE descriptor upload and THREE launches (convert + filter of every row;
 * deflate of every segment, one wave each; gather of the segments into one packed stream), synchronises `stream`, and returns with the
 * complete files at every item's `out`.  Not inside a stream capture (THMR_ERR_STATE). */
typedef struct thmr_png thmr_png;
int  thmr_png_create(int32_t device, thmr_png** out);
void thmr_png_destroy(thmr_png* p);
const char* thmr_png_last_error(const thmr_png* p);
int  thmr_png_encode_batch(thmr_png* p, thmr_png_item* items_host, int32_t n, void* stream);

/* PNG decoding for the evaluation datasets and demo.py's imread (csrc/pngdec.hip, pngdec_host.h, pngdec_math.h): new symbols
 * under ABI 5.  A hybrid in the shape of the JPEG decoder: the host walks the chunks and inflates the zlib stream — the sequential part,
 * with an inflate of its own (the library links no zlib) — only down to the last row a WINDOW of the frame needs, and keeps only the
 * bytes that can influence the window; the device un-filters them and converts palette, grey, alpha, 16-bit samples and the channel
 * order, straight into the (win_h, win_w, 3) uint8 buffer thmr_cropper_run_frames takes.  Everything is bit-exact.
 *   result        what cv2.imread(path, IMREAD_COLOR | IMREAD_IGNORE_ORIENTATION) gives for the file: (H, W, 3) uint8, B, G, R (bgr = 0:
 *                 R, G, B).  Grey is replicated to three channels; a palette index goes through PLTE; alpha is dropped, never composited
 *                 (the alpha channel of colour types 4 and 6, and tRNS); a 16-bit sample becomes its high byte.  For every supported
 *                 8-bit file that is Pillow's Image.open(f).convert("RGB"), for 16-bit RGB(A) the array Pillow returns, for 16-bit grey
 *                 Pillow's I;16 array >> 8; for 16-bit grey + alpha the rule stands on its own.
 *   supported     non-interlaced, bit depth 8 in colour types 0, 2, 3, 4, 6 or bit depth 16 in colour types 0, 2, 4, 6; any number of
 *                 consecutive IDAT chunks with the zlib stream running across their boundaries; ancillary chunks (gAMA, sRGB, iCCP,
 *                 pHYs, tEXt, acTL, ...) are skipped and have no effect
 *   unsupported   THMR_ERR_UNSUPPORTED, the message names what was found: Adam7 interlace, bit depths 1, 2 and 4, a side above 32767,
 *                 a compression or filter method other than 0
 *   malformed     THMR_ERR_INVALID, never a read outside [data, data + len), never an unbounded loop: a bad signature; a truncated
 *                 chunk; a wrong CRC on IHDR, PLTE or an IDAT that is read; a first chunk other than IHDR; PLTE missing for colour type
 *                 3; a palette index beyond PLTE; a zlib header that is not deflate with a window of 32K or less; a stored block whose
 *                 length check fails; an over-subscribed or incomplete Huffman code (a single distance code of one bit is allowed, as
 *                 zlib allows it); a distance that reaches before the first output byte; a stream that ends before the rows needed
 *                 are out; a filter byte above 4.  The Adler-32 is checked only when the whole stream was inflated (a window that
 *                 reaches the last row).
 *   kept          a window {x0, y0, w, h} needs the unfiltered bytes [0, (x0 + w) * bpp) of the rows [row0, y0 + h): row0 is the last
 *                 row at or above y0 whose filter is None or Sub (row 0 always qualifies: its previous row is zeros) — nothing above
 *                 such a row and nothing right of the window can influence the window.  They are stored as rows of
 *                 1 + kept_row_bytes, the filter byte first.
 * The host entry points need no device, are re-entrant and keep no state; their message is in thmr_png_decoder_last_error(NULL)
 * (thread-local). */
/* The info and the plan are arrays of int32_t words, indexed by the constants below (no struct: the words are what a binding reads).
 * info: THMR_PNG_INFO_WORDS words.  BPP is the bytes per pixel in the file, 1, 2, 3, 4, 6 or 8 where supported, else 0; SUPPORTED is 1,
 * or 0 with the reason in thmr_png_decoder_last_error(NULL). */
enum { THMR_PNG_INFO_HEIGHT = 0, THMR_PNG_INFO_WIDTH = 1, THMR_PNG_INFO_BIT_DEPTH = 2, THMR_PNG_INFO_COLOUR_TYPE = 3,
       THMR_PNG_INFO_INTERLACE = 4, THMR_PNG_INFO_BPP = 5, THMR_PNG_INFO_SUPPORTED = 6, THMR_PNG_INFO_WORDS = 8 };
/* plan: THMR_PNG_PLAN_WORDS words, what thmr_png_inflate_window kept.  WIN_*: the window the plan was made for.  The rows in the buffer
 * are [ROW0, ROW0 + ROWS_KEPT) = [ROW0, WIN_Y0 + WIN_H); KEPT_ROW_BYTES is (WIN_X0 + WIN_W) * BPP, and a stored row has the filter byte
 * before them; ROWS_INFLATED rows came out of the inflate, never more than WIN_Y0 + WIN_H.  From word THMR_PNG_PLAN_PALETTE on: 768
 * BYTES, the palette as 256 x (R, G, B), zero beyond PALETTE_ENTRIES. */
enum { THMR_PNG_PLAN_HEIGHT = 0, THMR_PNG_PLAN_WIDTH = 1, THMR_PNG_PLAN_BIT_DEPTH = 2, THMR_PNG_PLAN_COLOUR_TYPE = 3, THMR_PNG_PLAN_BPP = 4,
       THMR_PNG_PLAN_WIN_X0 = 5, THMR_PNG_PLAN_WIN_Y0 = 6, THMR_PNG_PLAN_WIN_W = 7, THMR_PNG_PLAN_WIN_H = 8, THMR_PNG_PLAN_ROW0 = 9,
       THMR_PNG_PLAN_ROWS_KEPT = 10, THMR_PNG_PLAN_KEPT_ROW_BYTES = 11, THMR_PNG_PLAN_ROWS_INFLATED = 12, THMR_PNG_PLAN_PALETTE_ENTRIES = 13,
       THMR_PNG_PLAN_PALETTE = 14, THMR_PNG_PLAN_WORDS = 14 + 192 };
/* Reads the signature and IHDR only.  info is filled for an unsupported file too (the return is THMR_ERR_UNSUPPORTED then). */
int thmr_png_probe(const uint8_t* data, size_t len, int32_t* info /* [THMR_PNG_INFO_WORDS] */);
/* window: {x0, y0, w, h} inside the frame (an empty one keeps nothing and inflates nothing), NULL = the whole frame.  rows NULL: the
 * plan's geometry is filled, *bytes_needed is the bound (win_y0 + win_h) * (1 + kept_row_bytes) and nothing is inflated; otherwise
 * `capacity` >= that bound, the kept rows are written from rows[0], the plan says which they are and *bytes_needed is
 * rows_kept * (1 + kept_row_bytes).  One pass: the inflate writes rows from the top, moves its write position back to the start
 * whenever it meets a None or Sub row at or above win_y0, and stops after row win_y0 + win_h - 1. */
int thmr_png_inflate_window(const uint8_t* data, size_t len, const int32_t* window, uint8_t* rows, int64_t capacity,
                            int32_t* plan /* [THMR_PNG_PLAN_WORDS] */, int64_t* bytes_needed);
/* The inflate alone, on a whole zlib stream (header, deflate blocks, Adler-32): *written bytes at out, THMR_ERR_INVALID for a malformed
 * stream or one that holds more than `capacity` bytes.  What the tests hold against zlib. */
int thmr_png_inflate(const uint8_t* zdata, size_t len, uint8_t* out, int64_t capacity, int64_t* written);
/* The full decode of a window on the CPU, with the kernels' arithmetic (shared __host__ __device__ functions, csrc/pngdec_math.h):
 * out (win_h, win_w, 3) uint8 host, row_stride >= win_w * 3 bytes per row, bytes beyond win_w * 3 of a row untouched. */
int thmr_png_decode_host(const uint8_t* data, size_t len, const int32_t* window, int32_t bgr, uint8_t* out, int64_t row_stride);
/* The device half.  The handle owns two grow-only sets of staging (pinned host + device), used alternately, and device scratch for the
 * unfiltered bytes.  thmr_png_decode_batch decodes n items of n sizes and formats with ONE packed upload and TWO launches.  Launch 1
 * un-filters: the kept rows of an item fall into strips, each starting at a None or Sub row (or at the first kept row); strips are
 * independent, and runs of short strips are joined into units of at most thmr_png_decode_band_rows() rows.  One wave takes a unit, a
 * band of that many rows at a time: each lane owns a row and runs one pixel behind the lane above it, which hands it the upper and
 * upper-left neighbours; the last row of a band feeds the next.  Launch 2 converts every window pixel.  A staging set is rewritten
 * only after the event behind its last use — two calls back — has completed; beyond that the call synchronises only when a buffer
 * grows (never inside a stream capture: THMR_ERR_STATE then — run the call once at those sizes first; a captured call keeps reading
 * its staging set, so give it a handle of its own).
 * An item is one entry of each of five host tables of n entries: rows_host[i] (host: ROWS_KEPT rows of 1 + KEPT_ROW_BYTES),
 * plans_host[i] (host: its plan words), windows_host[4 i ...] = {x0, y0, w, h}, out_dev[i] (device: (win_h, win_w, 3) uint8) and
 * row_strides_host[i] (bytes per output row, >= win_w * 3).  Every argument is checked before the handle and the handle before any HIP
 * call: n <= 0, a null table, and per item (the message names its index) a null plan / rows, a plan that is not one
 * thmr_png_inflate_window produces, a window outside the frame or outside what the plan kept, a filter byte above 4, a first kept row
 * that needs a row above it, row_stride < win_w * 3, a null out_dev with a non-empty window.  Bytes of out_dev beyond win_w * 3 of a
 * row are not written. */
typedef struct thmr_png_decoder thmr_png_decoder;
int  thmr_png_decode_band_rows(void);
int  thmr_png_decoder_create(int32_t device, thmr_png_decoder** out);
void thmr_png_decoder_destroy(thmr_png_decoder* d);
const char* thmr_png_decoder_last_error(const thmr_png_decoder* d);
int  thmr_png_decode_batch(thmr_png_decoder* d, const uint8_t** rows_host, const int32_t** plans_host, const int32_t* windows_host,
                           uint8_t** out_dev, const int64_t* row_strides_host, int32_t n, int32_t bgr, void* stream);

/* Baseline JPEG encoding of device images: the counterpart of cv2.imwrite(".jpg") (csrc/jpegenc.hip, jpegenc_host.h,
 * jpegenc_math.h): new symbols under ABI 5.  The file is the one libjpeg (libjpeg-turbo, Pillow's save(format="JPEG", quality=q,
 * subsampling=s)) writes for the same pixels, byte for byte, header included; it is a function of the pixels and the arguments only, and
 * thmr_jpeg_encode_host — the same algorithm on the CPU, sharing its arithmetic with the kernels — writes the same bytes.  An image is
 * described by a thmr_png_item with compression == 0; quality and subsampling are passed beside it.
 *   samples       uint8 or float32, 1 / 3 / 4 channels, any element strides, converted to uint8 by the PNG encoder's rule (scale,
 *                 rounding, NaN / inf) and swapped by swap_rb as there; the alpha of a 4-channel image is dropped (as cv2 does).
 *   colour        jccolor.c, 16-bit fixed point: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B +
 *                 8388608 + 32767) >> 16, Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16.  One channel: Y is the sample.
 *   sampling      THMR_JPEG_444 (MCU 8x8) or THMR_JPEG_420 (MCU 16x16, blocks Y00 Y01 Y10 Y11 Cb Cr).  A component of w_c x h_c samples has
 *                 ceil(w_c / 8) x ceil(h_c / 8) real blocks; luma is W x H, 4:2:0 chroma ceil(W / 2) x ceil(H / 2).  Samples of a real
 *                 block beyond the image repeat luma column W - 1 and row H - 1.  4:2:0 chroma sample (r, c): r' = min(r, ceil(H / 2) - 1)
 *                 (the DOWNSAMPLED row is repeated), pixel rows 2r' and min(2r' + 1, H - 1), columns min(2c, W - 1) and min(2c + 1, W - 1),
 *                 value (sum of the four + bias) >> 2 with bias 1 for even c and 2 for odd c.  A luma block of a 4:2:0 MCU outside the
 *                 luma grid is a dummy: it codes as DC difference 0 + end-of-block and leaves the predictor alone.
 *   transform     jfdctint.c (JDCT_ISLOW) on sample - 128: CONST_BITS 13, PASS1_BITS 2, rows first, then columns.
 *   quantisation  the Annex K tables scaled by s = 5000 / q (q < 50) or 200 - 2 q: clamp((base * s + 50) / 100, 1, 255); a coefficient c
 *                 becomes sign(c) * ((|c| + 4 t) / (8 t)).
 *   entropy       the Annex K Huffman tables, no optimisation pass, no restart markers: DC difference by category, AC as (run, size) with
 *                 ZRL 0xF0 and EOB 0x00, a negative value sends the low bits of v - 1; bits MSB first, every 0xFF followed by 0x00, the
 *                 last byte padded with ones (and stuffed if that makes it 0xFF).
 *   optimised     the flag THMR_JPEG_OPTIMIZE (the *_flags entry points; libjpeg's optimize_coding, Pillow's optimize=True, cv2's
 *                 IMWRITE_JPEG_OPTIMIZE) keeps everything up to the quantised blocks and codes the scan with tables made from the image's
 *                 own statistics; the file is again Pillow's, byte for byte.  Every symbol the scan codes is counted, the DC 0 + EOB of
 *                 the dummy blocks included, into one histogram per table in use (DC0, AC0 and, with three components, DC1, AC1: the
 *                 components use the tables 0, 1, 1 as in the header).  A table is jpeg_gen_optimal_table's (csrc/jpegenc_math.h): the
 *                 symbols in use and a pseudo-symbol 256 of frequency 1, which keeps the all-ones code unused; the two least frequent
 *                 entries are merged until one is left, among equal frequencies the larger symbol first; code sizes, which may pass 16,
 *                 are limited to 16 by libjpeg's adjustment of the counts per length; the pseudo-symbol's count leaves the longest length
 *                 in use; the symbols are listed by their size before the limit, then by value, and take canonical codes (Annex C).
 *                 Pillow's bytes are the arbiter of every detail: where this text and Pillow disagree, Pillow wins (the tests hold the
 *                 files and the DHT payloads to Pillow's).  The markers stay the same, only the DHT contents and lengths and the scan
 *                 bits change.  An optimised image has at most 2^23 blocks (every frequency sum stays below libjpeg's 10^9).
 *   container     SOI; APP0 JFIF 1.01, units 0, density 1 x 1; one DQT per table (0, then 1; 8-bit, zigzag); SOF0 with components 1 / 2 /
 *                 3 at 0x22 or 0x11, 0x11, 0x11 and tables 0, 1, 1; one DHT per table in the order DC0, AC0, DC1, AC1; SOS with selectors
 *                 0x00, 0x11, 0x11, Ss 0, Se 63, Ah/Al 0; the scan; EOI.  Grey has one component, table 0, DC0 and AC0 only.
 *   refused       before any HIP call, the message names the item: THMR_ERR_UNSUPPORTED for a 16-bit dtype, 2 channels and
 *                 THMR_JPEG_422; THMR_ERR_INVALID for a quality outside 1 ... 100, width or height < 1 or > 65535, any other dtype /
 *                 channel count / rounding / subsampling, compression != 0, a null pointer, a capacity below thmr_jpeg_encode_bound()
 *                 (thmr_jpeg_encode_bound_flags() for a flagged item), an unknown flag bit, and more than 2^23 blocks with the flag. */
enum { THMR_JPEG_444 = 0, THMR_JPEG_422 = 1 /* refused by name */, THMR_JPEG_420 = 2 };
enum { THMR_JPEG_OPTIMIZE = 1 };        /* a flag bit of the *_flags entry points; every other bit is refused */
/* The largest file: every block of every MCU at its worst case — 22 bits of DC (an 11-bit code + 11 value bits) and 63 x (16 + 10) bits
 * of AC = 1660 bits — rounded up to bytes, TWICE that (each byte may be 0xFF and draw a 0x00), the header (623 bytes, grey 328) and
 * EOI.  0 for arguments the encoder refuses. */
int64_t thmr_jpeg_encode_bound(int32_t width, int32_t height, int32_t channels, int32_t subsampling);
int thmr_jpeg_encode_host(thmr_png_item* item, int32_t quality, int32_t subsampling);
/* The bound of a mode.  The choice between a second bound and a proof that the first holds went to the bound: with THMR_JPEG_OPTIMIZE a
 * DC table has up to 12 symbols and the pseudo-symbol, so a DC code can take 12 bits and a block 23 + 63 x 26 = 1661; an optimised table
 * has no more symbols than an Annex K one, so the header is no longer.  Capacity checks, the unstuffed scratch and the staging of a
 * flagged item are sized from it.  Flags 0: thmr_jpeg_encode_bound.  0 for arguments the encoder refuses, an unknown flag bit included. */
int64_t thmr_jpeg_encode_bound_flags(int32_t width, int32_t height, int32_t channels, int32_t subsampling, int32_t flags);
/* thmr_jpeg_encode_host with flags (0: the same file). */
int thmr_jpeg_encode_host_flags(thmr_png_item* item, int32_t quality, int32_t subsampling, int32_t flags);
/* The Huffman table of the optimised mode for the frequencies freq[0 ... 255] by symbol, the very routine the table kernel runs: bits[1
 * ... 16] the codes per length, bits[0] the longest code size BEFORE the limit to 16 (above 16: the adjustment ran), huffval[0 ... *nsym)
 * the symbols in code order (256 bytes of room).  Host only.  THMR_ERR_INVALID for a null pointer, a negative frequency, an all-zero
 * histogram or a sum above 10^9; THMR_ERR_UNSUPPORTED for frequencies that give a size above 32 (libjpeg refuses them too). */
int thmr_jpeg_optimal_table(const int32_t* freq, uint8_t* bits, uint8_t* huffval, int32_t* nsym);
/* The statistics the optimised encode of this item builds its tables from: freq[t * 256 + symbol] for the tables t = 0 ... 3 in the
 * order DC0, AC0, DC1, AC1 (1024 entries; grey leaves DC1 and AC1 zero).  Host only; the item's `out` is not touched. */
int thmr_jpeg_histogram_host(const thmr_png_item* item, int32_t quality, int32_t subsampling, int32_t* freq);
/* The handle owns grow-only device scratch (coefficients, bit counts, the unstuffed scans) and pinned staging that the device writes the
 * finished scans into.  One call encodes n images of n sizes, layouts, qualities and samplings with ONE descriptor upload and a fixed
 * number of launches (transform; count; two scans; pack; the 0xFF count, its scan and the scatter), synchronises `stream` ONCE, at the
 * end, and returns with the complete files at every item's `out`.  Not inside a stream capture (THMR_ERR_STATE).
 * thmr_jpeg_encode_batch_flags takes one flag word per item; flagged and unflagged items share the ONE call, upload and synchronisation.
 * Flagged items add two launches, whatever n: the symbol histogram (LDS per workgroup, integer atomics into the image's histograms,
 * which are zeroed on the stream by every call) and the table build (one wave per image and table), whose code words the count and pack
 * kernels then read for that image, chosen per workgroup; bits and huffval come back with the scans and the host writes the DHT segments.
 * A call without a flagged item launches what thmr_jpeg_encode_batch launches. */
typedef struct thmr_jpeg_encoder thmr_jpeg_encoder;
int  thmr_jpeg_encoder_create(int32_t device, thmr_jpeg_encoder** out);
void thmr_jpeg_encoder_destroy(thmr_jpeg_encoder* e);
const char* thmr_jpeg_encoder_last_error(const thmr_jpeg_encoder* e);
int  thmr_jpeg_encode_batch(thmr_jpeg_encoder* e, thmr_png_item* items_host, const int32_t* qualities, const int32_t* subsamplings, int32_t n,
                            void* stream);
int  thmr_jpeg_encode_batch_flags(thmr_jpeg_encoder* e, thmr_png_item* items_host, const int32_t* qualities, const int32_t* subsamplings,
                                  const int32_t* flags, int32_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TOKENHMR_HIP_H */
