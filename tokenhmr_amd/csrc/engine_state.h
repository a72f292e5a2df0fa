// The engine's state and what its three translation units share.  Host only, private to them: no kernel and not ops_abi.hip include it.
//   engine_weights.hip   the checkpoint contract (ONE table), both layouts, load, finalize, the split3 weight copies
//   engine_paths.hip     what a call enqueues: ViT, heads, VQ decoder, tokenizer encoder and round trip, SMPL
//   engine.hip           create / destroy, the per-device turnstile, the timeout recoveries, status, debug, profiler, the forward-type entry points
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/tokenhmr_hip.h"
#include "abi_util.h"
#include "common.h"
#include "vit_plan.h"

constexpr int HEADS = 16;                              // TOK, DIM, MLP, INNER: vit_plan.h
constexpr int E = 1024, DEC_MLP = 1024;
constexpr int TN = 160, NCLS = 2048, HID = 64, HID_INTER = 256, TOK_INTER = 64, MIX = 4;
constexpr int CODE = 256, VQW = 512, VQJ = 21;
constexpr float VIT_EPS = 1e-6f, LN_EPS = 1e-5f;
// (NV, NJ, NB, NP, FOCAL, IMG: abi_util.h)
// (the ViT's batch-size regimes — kSmallM, kMid*, kSplit3* — and every kernel choice that follows from them: vit_plan.h)

// A Conv1d of the tokenizer: its tensors are `name`.weight (co, ci, ks) and `name`.bias (co); a k > 1 conv is read as a GEMM weight
// (co, ks * cp) repacked at finalize, with the input channels zero-padded to cp.
struct Conv1d { const char* name; int ci, cp, co, ks; };
constexpr int kVqDecN = 11, kEncN = 11;      // = the lengths of HotW::vq_* / enc_*
extern const Conv1d kVqDec[kVqDecN];         // PoseSPDecoderV1, execution order (engine_weights.hip)
extern const Conv1d kEnc[kEncN];             // PoseSPEncoderV1, execution order

struct Slot {
    size_t off = 0;       // float offset in the weight arena
    int64_t numel = 0;
    bool loaded = false;
};

struct VitBlockW {      // weights of one ViT block (vit.py:128-151), pointers into the weight arena
    const float *n1w, *n1b, *qkvw, *qkvb, *pw, *pb, *n2w, *n2b, *f1w, *f1b, *f2w, *f2b;
};

// every weight a call touches that is not in VitBlockW, DecParams or MixerParams.  With those this is ALL of them: resolve_weights
// (thmr_finalize_weights) is the only place behind the layout and the load that looks a tensor up by name, and no call path builds or
// hashes a name
struct HotW {
    const float *pe_w, *pe_b, *pos, *lastn_w, *lastn_b, *cls_w, *cls_b, *init_pose, *init_betas, *init_cam;
    const float *vq_w[kVqDecN], *vq_b[kVqDecN];   // VQ decoder convs (kVqDec): the REPACKED weights where ks > 1
    const float* codebook;                        // quantizer.codebook (2048, 256); null on an HMR2 engine
    const float *enc_w[kEncN], *enc_b[kEncN];     // tokenizer encoder (kEnc), likewise; null unless enc_ready
};

struct ProfRec {
    int cls;
    double flops, bytes;
    hipEvent_t e0, e1;
};

// The weight arena as float offsets: a function of (vit_depth, dec_depth, head kind) alone — layout_weights.  It is broadcast between
// ranks byte for byte and pinned by tests/golden/arena_layout.json.
struct WeightLayout {
    std::unordered_map<std::string, Slot> slots;
    std::vector<std::string> required;      // = thmr_spec, in its order
    size_t wfloats = 0;
    // derived / constant regions
    size_t o_kv_all = 0, o_ro_w = 0, o_ro_b = 0;
    size_t o_cbT = 0, o_cnorm = 0, o_idx = 0, o_inv = 0;   // idx / inverse idx tables as int32 within the float arena
    SmplConsts smpl;                        // the SMPL constant block
    std::vector<size_t> convp;              // repacked VQ decoder convs, index by kVqDec id
    // optional tokenizer ENCODER (EncodeTokens, vanilla_pose_vqvae.py:304-346): 'encoder.encoder.*' tensors
    std::vector<std::string> enc_names;
    std::vector<size_t> enc_convp;          // repacked encoder convs, index by kEnc id
    size_t o_idx_enc = 0, o_flags = 0;
};
void layout_weights(WeightLayout& l, int vit_depth, int dec_depth, bool hmr2);

// The activation arena of an engine as float offsets: a function of (max_batch, head kind) — layout_scratch
struct ScratchLayout {
    size_t x, h, big, part;
    size_t dx, dh, dv, dq, dca, dff, ro;
    size_t mt, cf, cf2, y1, tT, u, yt, y, s, z0, zh, nl, nl2;
    size_t part_floats;       // capacity of `part`
    size_t feat, gat, gat2, act0, act1, act2, bpose, tokidx, sync;
    size_t A, pf, Jtr, vposed, rot, betas, cam, camt, verts, joints, pose6d, xv, lcnt;
    size_t total;
};
ScratchLayout layout_scratch(int max_batch, bool hmr2);

struct thmr_engine : WeightLayout {
    thmr_config cfg{};
    int vit_depth = 32, dec_depth = 6, max_batch = 0;
    float* warena = nullptr;
    float* sarena = nullptr;
    bool own_w = false, own_s = false;
    size_t sfloats = 0;
    std::vector<VitBlockW> vitw;      // filled by resolve_weights (thmr_finalize_weights)
    DecParams dec{};                  // decoder weight pointers + scratch, resolved once (finalize); the launch-chain head reads them too
    MixerParams mix{};                // MLP-Mixer stack weight pointers
    HotW hot{};
    bool counted = false;             // registered in the per-device engine count (decoder turnstile)
    bool hmr2 = false;                // THMR_CFG_HEAD_HMR2: the HMR2.0 regressor head (stacked read-out + finish) instead of the token head
    bool no_persistent = false;       // THMR_CFG_NO_PERSISTENT: launch-chain head, per-tile split3 GEMMs, no hand-over workspace
    bool legacy_head = false;         // THMR_LEGACY_HEAD=1: force the chain-of-GEMMs head at every batch size (A/B only)
    bool mixer_cluster = true;        // THMR_MIXER_CLUSTER=0: always run the mixer stack as its own one-workgroup-per-crop kernel (A/B only)
    bool tiny_gemm = true;            // THMR_TINY_GEMM=0: the VQ decoder's GEMMs stay on the ring kernel in the small-batch regime (A/B only)
    bool smpl_loaded = false, finalized = false;
    // 1 (the DEFAULT since round 5 / ABI 4: what thmr_forward, the facade and bench.py's `value` all run): the four ViT GEMMs, the attention
    // and the decoder's to_kv GEMM of batches of at least kSplit3LowMinB (3) crops run on the bf16 matrix pipe with fp32 operands carried as
    // three bf16 pieces (csrc/gemm_split16.hip, attention_b16.hip).  Engine-owned memory, built by thmr_finalize_weights: the split3 copies of
    // the ViT weights (1.5 x their fp32 size) and the split3 activation operands (M x (1280 + 5120) x 6 bytes).  thmr_set_vit_gemm(0) = the
    // opt-out: exact-fp32 MFMA everywhere.  An engine whose max_batch is below 3 never runs the mode and builds nothing for it.
    int vit_gemm_mode = 1;
    VitKnobs knobs;                   // everything an A/B knob can change about the ViT / to_kv dispatch (vit_plan.h; read_knobs, engine.hip)
    char* split_w = nullptr;          // split3 weight copies: shared, reference-counted, among the engines of one weight arena (engine_weights.hip)
    bool split_w_counted = false;     // this engine holds a reference to the shared copy
    char* split_act = nullptr;
    // tile streams of the split3 GEMMs (csrc/gemm_split3_dispatch.hip): hand-over slabs + flags, allocated with the split3 weights on a
    // 256-CU device; s3_persist: run-time state, 1 until a hand-over timeout was recovered (then the per-tile kernels, same results)
    void* s3_ws = nullptr;
    int s3_persist = 1;
    bool s3_forced_once = false;      // experiments build: THMR_SPLIT3_FORCE_TIMEOUT=1 was honoured already
    struct SplitW { const char *qkv, *proj, *fc1, *fc2; };
    std::vector<SplitW> vitw_s;
    const char* kv_s = nullptr;       // split3 copy of the decoder's stacked to_kv weights (dec_depth * 1024 rows x 1280)
    const char* pe_s = nullptr;       // split3 copy of the patch-embed Conv2d weight as a (1280, 768) matrix
    unsigned* host_err = nullptr;     // host-mapped sticky error words (hipHostMalloc, 64 bytes): [0] the persistent decoder kernel's grid barrier, [1] the persistent split3 GEMM's hand-over, [2] a code index out of range in the tokenizer's hard lookup / statistics
    unsigned* s3_host_err = nullptr;  // = host_err + 1; its ADDRESS is the stable source of the copy that binds it into the hand-over workspace
    std::string err;
    bool enc_ready = false;
    int32_t flag_host[2] = {0, 0};
    std::vector<int32_t> idx_host, eidx_host, inv_host;   // staging for the index tables (must outlive the async copy)
    int vq_len[5] = {160, 125, 90, 55, 21};
    ScratchLayout so{};
    // profiler
    int prof_on = 0;            // 0 off, 1 every kernel class, 2 only the four ViT GEMM classes, 3 only fc1 (the dominant kernel)
    std::vector<ProfRec> prof;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_next = 0;

    float* W(const std::string& name) {
        auto it = slots.find(name);
        if (it == slots.end()) { err = "internal: unknown weight " + name; return nullptr; }
        return warena + it->second.off;
    }
    float* S(size_t off) { return sarena + off; }
};

#define THMR_FAIL(code, msg) fail(e, code, msg)      // HIP_OK / LAUNCH_OK (abi_util.h): every function of the engine units has its engine `e` in scope

int validate_cfg(const thmr_config* cfg);                        // engine.hip
int reset_s3_workspace(thmr_engine* e, hipStream_t st);          // engine_weights.hip: zero the hand-over workspace, bind the error word again
void release_split_weights(thmr_engine* e);                      // engine_weights.hip: this engine's reference to the shared split3 weight copies

// engine_paths.hip: each enqueues on `st`, allocates nothing and never synchronises
// rotmat, betas, pred_cam and pred_cam_t of a call live in the caller's buffer where it gave one, else in the scratch arena
struct PoseBufs { float *rot, *betas, *cam, *camt; };
PoseBufs pose_bufs(thmr_engine* e, const thmr_outputs* out);
int vit_forward(thmr_engine* e, const float* img, int B, float* feats_out, hipStream_t st);
int head_forward_call(thmr_engine* e, const float* ctx_dev, int32_t B, const thmr_outputs* out, hipStream_t st);
int forward_call(thmr_engine* e, const float* img_dev, int32_t B, const thmr_outputs* out, hipStream_t st);
int lbs(thmr_engine* e, const float* rot, const float* betas, const float* camt, int B, float* verts, float* joints, float* kp2d, hipStream_t st);
int vq_decode(thmr_engine* e, const float* probs, int B, float* bpose, hipStream_t st);
int vq_decode_idx(thmr_engine* e, const int32_t* idx, const float* x, int B, float* bpose, hipStream_t st);
int encode_tokens_call(thmr_engine* e, const float* pose_dev, int B, int32_t* idx_dev, float* latent_dev, const float** lat_out, hipStream_t st);
int tokenizer_roundtrip_call(thmr_engine* e, const float* pose6d_dev, int B, const thmr_tokenizer_out* out, hipStream_t st);
