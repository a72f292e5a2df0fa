// TokenHMR inference engine + C ABI (include/tokenhmr_hip.h).
//
// One engine per GPU: owns a packed weight arena (reference checkpoint tensors at fixed offsets, so a
// single RCCL broadcast of the arena replicates the model) and a static activation arena sized for
// max_batch crops; thmr_forward launches the whole path on the caller's stream with no allocation
// and no host synchronisation.
//
// Hot path orchestrated here (reference: tokenhmr/lib/models/tokenhmr.py:135-188 forward_step):
//   ViT-H            vit.py:320-343          -> vit_forward()
//   decoder + head   token_head.py:65-128    -> head_forward()
//   SMPL + camera    smpl_wrapper.py:27-41, geometry.py:86-124, tokenhmr.py:165-187 -> lbs()
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/tokenhmr_hip.h"
#include "abi_util.h"
#include "common.h"
#include "vit_plan.h"

namespace {

constexpr int HEADS = 16;                              // TOK, DIM, MLP, INNER: vit_plan.h
constexpr int E = 1024, DEC_MLP = 1024;
constexpr int TN = 160, NCLS = 2048, HID = 64, HID_INTER = 256, TOK_INTER = 64, MIX = 4;
constexpr int CODE = 256, VQW = 512, VQJ = 21;
constexpr float VIT_EPS = 1e-6f, LN_EPS = 1e-5f;
// (NV, NJ, NB, NP, FOCAL, IMG: abi_util.h)
// (the ViT's batch-size regimes — kSmallM, kMid*, kSplit3* — and every kernel choice that follows from them: vit_plan.h)
// decoder + mixer stack: the persistent decoder kernel and the one-workgroup-per-crop mixer kernel win while the work is
// latency-bound (B = 1: 0.96 vs 1.01 ms, B = 64: 1.58 vs 1.93 ms per head); from a few hundred crops on the same products are
// real GEMMs (M = B and M = 160 B rows) and the tiled MFMA kernels win (B = 512: 6.7 vs 7.5 ms) — profiles/r2e_head_fused_vs_chain.log
constexpr int kFusedHeadMaxB = 128;

thread_local std::string g_last_error;

struct Slot {
    size_t off = 0;       // float offset in the weight arena
    int64_t numel = 0;
    bool loaded = false;
};

struct VitBlockW {      // weights of one ViT block (vit.py:128-151), pointers into the weight arena
    const float *n1w, *n1b, *qkvw, *qkvb, *pw, *pb, *n2w, *n2b, *f1w, *f1b, *f2w, *f2b;
};

struct ProfRec {
    int cls;
    double flops, bytes;
    hipEvent_t e0, e1;
};

}  // namespace

struct thmr_engine {
    thmr_config cfg{};
    int vit_depth = 32, dec_depth = 6, max_batch = 0;
    float* warena = nullptr;
    float* sarena = nullptr;
    bool own_w = false, own_s = false;
    size_t wfloats = 0, sfloats = 0;
    std::unordered_map<std::string, Slot> slots;
    std::vector<std::string> required;
    std::vector<VitBlockW> vitw;      // filled by resolve_weights (thmr_finalize_weights)
    DecParams dec{};                  // decoder weight pointers + scratch, resolved once (finalize); the launch-chain head reads them too
    MixerParams mix{};                // MLP-Mixer stack weight pointers
    // every other weight a call touches.  With vitw, dec and mix this is ALL of them: resolve_weights (thmr_finalize_weights) is the only
    // place behind the layout and the load that looks a tensor up by name, and no call path builds or hashes a name
    struct HotW {
        const float *pe_w, *pe_b, *pos, *lastn_w, *lastn_b, *cls_w, *cls_b, *init_pose, *init_betas, *init_cam;
        const float* conv_b[9];       // biases of the nine k = 3 convs of the VQ decoder, execution order (kConv3)
        const float *res_w[2], *res_b[2];   // the two 1x1 convs of the ResConv blocks
        const float* codebook;        // quantizer.codebook (2048, 256); null on an HMR2 engine
        const float *enc_w[11], *enc_b[11];   // tokenizer encoder, execution order (kEnc): the REPACKED weights where ks > 1; null unless enc_ready
    } hot{};
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
    VitKnobs knobs;                   // everything an A/B knob can change about the ViT / to_kv dispatch (vit_plan.h; read_knobs below)
    char* split_w = nullptr;          // split3 weight copies: shared, reference-counted, among the engines of one weight arena (split_share())
    bool split_w_counted = false;     // this engine holds a reference in split_share()
    char* split_act = nullptr;
    // tile streams of the split3 GEMMs (csrc/gemm_split_persist.hip): hand-over slabs + flags, allocated with the split3 weights on a
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
    // derived / constant regions (float offsets in weight arena)
    size_t o_kv_all = 0, o_ro_w = 0, o_ro_b = 0;
    size_t o_convp[7] = {0};      // repacked k=3 convs: 0,3,6,9,12, res0.conv1, res1.conv1, 14.1, 15 -> see conv_names
    size_t o_cbT = 0, o_cnorm = 0, o_idx = 0, o_inv = 0;   // idx / inverse idx tables as int32 within the float arena
    SmplConsts smpl;              // the SMPL constant block
    std::vector<size_t> convp;    // repacked conv offsets, index by conv id
    // optional tokenizer ENCODER (EncodeTokens, vanilla_pose_vqvae.py:304-346): 'encoder.encoder.*' tensors
    std::vector<std::string> enc_names;
    std::vector<size_t> enc_convp;   // repacked encoder convs, index by kEnc id
    size_t o_idx_enc = 0, o_flags = 0;
    bool enc_ready = false;
    int32_t flag_host[2] = {0, 0};
    std::vector<int32_t> idx_host, eidx_host, inv_host;   // staging for the index tables (must outlive the async copy)
    int vq_len[5] = {160, 125, 90, 55, 21};
    // scratch offsets (floats)
    struct {
        size_t x, h, big, part;
        size_t dx, dh, dv, dq, dca, dff, ro;
        size_t mt, cf, cf2, y1, tT, u, yt, y, s, z0, zh, nl, nl2;
        size_t part_floats;       // capacity of `part`
        size_t feat, gat, gat2, act0, act1, act2, bpose, tokidx, sync;
        size_t A, pf, Jtr, vposed, rot, betas, cam, camt, verts, joints, pose6d, xv, lcnt;
        size_t total;
    } so{};
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

// the one last-error string behind both forms of fail() (abi_util.h); thmr_last_error(nullptr) reads it
int fail(thmr_engine* e, int code, const std::string& msg) {
    if (e) e->err = msg;
    g_last_error = msg;
    return code;
}
int fail(int code, const std::string& msg) { return fail(nullptr, code, msg); }

bool device_has_256_cus() {
    static std::mutex mu;
    static std::map<int, bool> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(dev);
    if (it != cache.end()) return it->second;
    hipDeviceProp_t prop;
    const bool ok = hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount == 256;
    cache[dev] = ok;
    return ok;
}

#define THMR_FAIL(code, msg) fail(e, code, msg)      // HIP_OK / LAUNCH_OK (abi_util.h): every function here has its engine `e` in scope

namespace {

// ---- the reference checkpoint contract, mirrored by tokenhmr_amd/weights.py::spec ----
void build_spec(int vit_depth, int dec_depth, bool hmr2, std::vector<std::pair<std::string, int64_t>>& out) {
    auto add = [&](const std::string& n, int64_t numel) { out.emplace_back(n, numel); };
    auto lin = [&](const std::string& n, int64_t o, int64_t i, bool bias = true) {
        add(n + ".weight", o * i);
        if (bias) add(n + ".bias", o);
    };
    auto ln = [&](const std::string& n, int64_t d) { add(n + ".weight", d); add(n + ".bias", d); };
    add("backbone.pos_embed", (TOK + 1) * DIM);
    add("backbone.patch_embed.proj.weight", (int64_t)DIM * 768);
    add("backbone.patch_embed.proj.bias", DIM);
    for (int i = 0; i < vit_depth; ++i) {
        const std::string p = "backbone.blocks." + std::to_string(i) + ".";
        ln(p + "norm1", DIM);
        lin(p + "attn.qkv", 3 * DIM, DIM);
        lin(p + "attn.proj", DIM, DIM);
        ln(p + "norm2", DIM);
        lin(p + "mlp.fc1", MLP, DIM);
        lin(p + "mlp.fc2", DIM, MLP);
    }
    ln("backbone.last_norm", DIM);
    const std::string T = "smpl_head.transformer.";
    add(T + "pos_embedding", E);
    lin(T + "to_token_embedding", E, 1);
    for (int l = 0; l < dec_depth; ++l) {
        const std::string p = T + "transformer.layers." + std::to_string(l) + ".";
        ln(p + "0.norm", E);
        lin(p + "0.fn.to_qkv", 3 * INNER, E, false);
        lin(p + "0.fn.to_out.0", E, INNER);
        ln(p + "1.norm", E);
        lin(p + "1.fn.to_kv", 2 * INNER, DIM, false);
        lin(p + "1.fn.to_q", INNER, E, false);
        lin(p + "1.fn.to_out.0", E, INNER);
        ln(p + "2.norm", E);
        lin(p + "2.fn.net.0", DEC_MLP, E);
        lin(p + "2.fn.net.3", E, DEC_MLP);
    }
    if (hmr2) {
        // SMPLTransformerDecoderHead (heads/smpl_head.py:32-34,46-48): three read-outs of token_out and the mean parameters; no token
        // classifier and no tokenizer
        lin("smpl_head.decpose", 144, E);
        lin("smpl_head.decshape", 10, E);
        lin("smpl_head.deccam", 3, E);
        add("smpl_head.init_body_pose", 144);
        add("smpl_head.init_betas", 10);
        add("smpl_head.init_cam", 3);
        return;
    }
    lin("smpl_head.decpose_grot", 6, E);
    lin("smpl_head.decshape", 10, E);
    lin("smpl_head.deccam", 3, E);
    lin("smpl_head.decpose_hands", 12, E);
    const std::string C = "smpl_head.decpose.";
    lin(C + "mixer_trans.ff.0", (int64_t)TN * HID, E);
    ln(C + "mixer_trans.ff.1", (int64_t)TN * HID);
    for (int m = 0; m < MIX; ++m) {
        const std::string p = C + "mixer_head." + std::to_string(m) + ".";
        ln(p + "layernorm1", HID);
        lin(p + "MLP_token.ff.0", TOK_INTER, TN);
        lin(p + "MLP_token.ff.3", TN, TOK_INTER);
        ln(p + "layernorm2", HID);
        lin(p + "MLP_channel.ff.0", HID_INTER, HID);
        lin(p + "MLP_channel.ff.3", HID, HID_INTER);
    }
    lin(C + "mixer_norm_layer.ff.0", HID, HID);
    ln(C + "mixer_norm_layer.ff.1", HID);
    lin(C + "class_pred_layer", NCLS, HID);
    add("smpl_head.init_body_pose", 144);
    add("smpl_head.init_betas", 10);
    add("smpl_head.init_cam", 3);
    // tokenizer.pth ['net']
    auto conv = [&](const std::string& n, int64_t co, int64_t ci, int64_t k) { add(n + ".weight", co * ci * k); add(n + ".bias", co); };
    conv("decoder.decoder.0", VQW, CODE, 3);
    for (int i : {3, 6, 9, 12}) conv("decoder.decoder." + std::to_string(i), VQW, VQW, 3);
    for (int b : {0, 1}) {
        conv("decoder.decoder.14.0.model." + std::to_string(b) + ".conv1", VQW, VQW, 3);
        conv("decoder.decoder.14.0.model." + std::to_string(b) + ".conv2", VQW, VQW, 1);
    }
    conv("decoder.decoder.14.1", VQW, VQW, 3);
    conv("decoder.decoder.15", 6, VQW, 3);
    add("quantizer.codebook", (int64_t)NCLS * CODE);
}

// k=3 convs that need the [co][k*ci+ci] repack, in execution order
const char* const kConv3[] = {"decoder.decoder.0", "decoder.decoder.3", "decoder.decoder.6", "decoder.decoder.9",
                              "decoder.decoder.12", "decoder.decoder.14.0.model.0.conv1",
                              "decoder.decoder.14.0.model.1.conv1", "decoder.decoder.14.1", "decoder.decoder.15"};
const int kConv3Ci[] = {CODE, VQW, VQW, VQW, VQW, VQW, VQW, VQW, VQW};
const int kConv3Co[] = {VQW, VQW, VQW, VQW, VQW, VQW, VQW, VQW, 6};

// tokenizer encoder convs in execution order (PoseSPEncoderV1, vanilla_pose_vqvae.py:66-88 with the release ARCH:
// input_dim 6, width 512, token_size_mul 4, down_t 1, stride_t 2, depth 2, dilation 3, code_dim 256)
struct EncConv { const char* name; int ci, cp, co, ks; };
const EncConv kEnc[] = {
    {"encoder.encoder.0", 6, 32, VQW, 3},                      // T=21, +ReLU
    {"encoder.encoder.3", VQW, VQW, VQW, 3},                   // nearest 21->40, +ReLU
    {"encoder.encoder.6", VQW, VQW, VQW, 3},                   // x2 -> 80
    {"encoder.encoder.9", VQW, VQW, VQW, 3},                   // x2 -> 160
    {"encoder.encoder.12", VQW, VQW, VQW, 3},                  // x2 -> 320
    {"encoder.encoder.14.0", VQW, VQW, VQW, 4},                // k4 s2 p1: 320 -> 160 (no activation)
    {"encoder.encoder.14.1.model.0.conv1", VQW, VQW, VQW, 3},  // ResConv1DBlock dil 3
    {"encoder.encoder.14.1.model.0.conv2", VQW, VQW, VQW, 1},
    {"encoder.encoder.14.1.model.1.conv1", VQW, VQW, VQW, 3},  // dil 1
    {"encoder.encoder.14.1.model.1.conv2", VQW, VQW, VQW, 1},
    {"encoder.encoder.15", VQW, VQW, CODE, 3},                 // -> (B,160,256)
};
constexpr int kEncN = 11;      // = the length of thmr_engine::HotW::enc_w / enc_b

// the token head's read-outs as one (31,1024) matrix + (31) biases, from `off` (= o_ro_w); returns the offset behind them
size_t layout_readout_token(thmr_engine* e, size_t off) {
    const char* ro_names[] = {"smpl_head.decpose_grot", "smpl_head.decshape", "smpl_head.deccam", "smpl_head.decpose_hands"};
    const int ro_n[] = {6, 10, 3, 12};
    for (int i = 0; i < 4; ++i) {
        e->slots[std::string(ro_names[i]) + ".weight"] = Slot{off, (int64_t)ro_n[i] * E, false};
        off += (size_t)ro_n[i] * E;
    }
    off += E;   // 32nd (padding) row so a clamped row read stays inside the arena
    off = align64(off);
    e->o_ro_b = off;
    for (int i = 0; i < 4; ++i) {
        e->slots[std::string(ro_names[i]) + ".bias"] = Slot{off, ro_n[i], false};
        off += ro_n[i];
    }
    return align64(off + 1);
}

// the HMR2 head's stacked read-out: decpose 144 | decshape 10 | deccam 3 rows, then zero rows up to ten whole 16-column tiles; the biases
// likewise.  Nothing of the token head follows: no classifier, no VQ decoder, no codebook, no resample tables, no encoder.
size_t layout_readout_hmr2(thmr_engine* e, size_t off) {
    const char* names[] = {"smpl_head.decpose", "smpl_head.decshape", "smpl_head.deccam"};
    const int rows[] = {144, 10, 3};
    for (int i = 0; i < 3; ++i) {
        e->slots[std::string(names[i]) + ".weight"] = Slot{off, (int64_t)rows[i] * E, false};
        off += (size_t)rows[i] * E;
    }
    off = align64(off + (size_t)(THMR_HMR2_RO_LD - THMR_HMR2_RO_ROWS) * E);
    e->o_ro_b = off;
    for (int i = 0; i < 3; ++i) {
        e->slots[std::string(names[i]) + ".bias"] = Slot{off, rows[i], false};
        off += rows[i];
    }
    return align64(off + (THMR_HMR2_RO_LD - THMR_HMR2_RO_ROWS));
}

void layout_weights(thmr_engine* e) {
    std::vector<std::pair<std::string, int64_t>> spec;
    build_spec(e->vit_depth, e->dec_depth, e->hmr2, spec);
    size_t off = 0;
    // contiguous groups first: to_kv of all layers -> one (dec_depth*1024, 1280) matrix; read-outs -> (31,1024)+(31)
    e->o_kv_all = off;
    for (int l = 0; l < e->dec_depth; ++l) {
        const std::string n = "smpl_head.transformer.transformer.layers." + std::to_string(l) + ".1.fn.to_kv.weight";
        e->slots[n] = Slot{off, (int64_t)2 * INNER * DIM, false};
        off += (size_t)2 * INNER * DIM;
    }
    off = align64(off);
    e->o_ro_w = off;
    off = e->hmr2 ? layout_readout_hmr2(e, off) : layout_readout_token(e, off);
    for (auto& kv : spec) {
        e->required.push_back(kv.first);
        if (e->slots.count(kv.first)) continue;
        e->slots[kv.first] = Slot{off, kv.second, false};
        off = align64(off + (size_t)kv.second);
    }
    // derived regions
    if (!e->hmr2) {
        e->convp.resize(9);
        for (int i = 0; i < 9; ++i) {
            e->convp[i] = off;
            off = align64(off + (size_t)kConv3Co[i] * kConv3Ci[i] * 3);
        }
        e->o_cbT = off;   off = align64(off + (size_t)NCLS * CODE);
        e->o_cnorm = off; off = align64(off + NCLS);
        e->o_idx = off;   off = align64(off + 4 * 160);
        e->o_inv = off;   off = align64(off + 4 * 160);
    }
    // SMPL constants
    off = e->smpl.lay(off);
    // optional tokenizer encoder (tokenizer.pth 'encoder.encoder.*'): raw tensors, repacked convs, resample tables
    for (int i = 0; i < (e->hmr2 ? 0 : kEncN); ++i) {
        const std::string n = kEnc[i].name;
        e->enc_names.push_back(n + ".weight");
        e->enc_names.push_back(n + ".bias");
        e->slots[n + ".weight"] = Slot{off, (int64_t)kEnc[i].co * kEnc[i].ci * kEnc[i].ks, false};
        off = align64(off + (size_t)kEnc[i].co * kEnc[i].ci * kEnc[i].ks);
        e->slots[n + ".bias"] = Slot{off, kEnc[i].co, false};
        off = align64(off + kEnc[i].co);
    }
    if (!e->hmr2) {
        e->enc_convp.resize(kEncN);
        for (int i = 0; i < kEncN; ++i) {
            e->enc_convp[i] = off;
            if (kEnc[i].ks > 1) off = align64(off + (size_t)kEnc[i].co * kEnc[i].cp * kEnc[i].ks);
        }
        e->o_idx_enc = off; off = align64(off + 640);
    }
    e->o_flags = off;   off = align64(off + 64);     // int32 flag words travelling with the arena (0: encoder present)
    e->wfloats = off;
}

void layout_scratch(thmr_engine* e) {
    const size_t B = (size_t)e->max_batch, M = B * TOK;
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off = align64(off + n); return o; };
    auto& s = e->so;
    s.x = take(M * DIM);
    s.h = take(M * DIM);
    s.big = take(M * 6144);
    {   // split-K partial sums of the proj / fc2 GEMMs: 4 x M x 1280 up to kSmallM rows (ring kernel), 2 x M x 1280 up to kMidHiM rows
        const size_t m2 = M < (size_t)kMidHiM ? M : (size_t)kMidHiM, need = (size_t)kMidSplit * m2;
        s.part_floats = (need > (size_t)kSplitKMax * kSmallM ? need : (size_t)kSplitKMax * kSmallM) * DIM;
        s.part = take(s.part_floats);
    }
    s.dx = take(B * E); s.dh = take(B * E); s.dv = take(B * INNER); s.dq = take(B * INNER); s.dca = take(B * INNER);
    s.dff = take(B * DEC_MLP); s.ro = take(B * (e->hmr2 ? THMR_HMR2_RO_LD : 32));
    if (!e->hmr2) {      // the token head's classifier and VQ decoder; the HMR2 head has neither
        s.mt = take(B * TN * HID); s.cf = take(B * TN * HID); s.cf2 = take(B * TN * HID);
        s.y1 = take(B * TN * HID); s.tT = take(B * HID * TN); s.u = take(B * HID * TOK_INTER); s.yt = take(B * HID * TN);
        s.y = take(B * TN * HID); s.s = take(B * TN * HID); s.z0 = take(B * TN * HID); s.zh = take(B * TN * HID_INTER);
        s.nl = take(B * TN * HID); s.nl2 = take(B * TN * HID);
        s.feat = take(B * TN * CODE);
        s.gat = take(B * 125 * 3 * VQW);                 // largest conv operand: T=125, 3*512 (> 160*768)
        s.gat2 = take(B * 125 * 3 * VQW);                // the GEMM of conv i writes the operand of conv i+1: two buffers alternate
        s.act0 = take(B * TN * VQW); s.act1 = take(B * TN * VQW); s.act2 = take(B * TN * VQW);
        s.bpose = take(B * 128); s.tokidx = take(B * TN);
    }
    s.sync = take(512);
    s.A = take(B * NJ * 12); s.pf = take(B * THMR_LBS_XF); s.Jtr = take(B * NJ * 3); s.vposed = take(B * NV * 3);
    s.rot = take(B * NJ * 9); s.betas = take(B * NB); s.cam = take(B * 3); s.camt = take(B * 3);
    s.verts = take(B * NV * 3); s.joints = take(B * 132); s.pose6d = take(B * 144);
    s.xv = take(B * 63); s.lcnt = take(B);
    s.total = off;
    e->sfloats = off;
}

// ---- profiler helpers ----
struct ProfScope {
    thmr_engine* e;
    hipStream_t s;
    bool on;
    size_t rec = 0;
    // `sampled`: mode 3 (only the dominant kernel, live in the timed region) instruments every 4th fc1 launch — all 32 per call have
    // the same shape, and 32 event pairs are still 5 % of a one-crop call
    ProfScope(thmr_engine* e_, hipStream_t s_, int cls, double flops, double bytes, bool sampled = true) : e(e_), s(s_), on(e_->prof_on == 1 || (e_->prof_on == 2 && cls <= THMR_PROF_GEMM_FC2) || (e_->prof_on == 3 && cls == THMR_PROF_GEMM_FC1 && sampled)) {
        if (!on) return;
        if (e->ev_next + 2 > e->ev_pool.size()) {
            for (int i = 0; i < 512; ++i) {
                hipEvent_t ev;
                if (hipEventCreate(&ev) != hipSuccess) { on = false; return; }
                e->ev_pool.push_back(ev);
            }
        }
        ProfRec r{cls, flops, bytes, e->ev_pool[e->ev_next], e->ev_pool[e->ev_next + 1]};
        e->ev_next += 2;
        (void)hipEventRecord(r.e0, s);
        e->prof.push_back(r);
        rec = e->prof.size() - 1;
    }
    ~ProfScope() {
        if (on) (void)hipEventRecord(e->prof[rec].e1, s);
    }
};

// the call's plan (vit_plan.h): a few dozen integer operations, evaluated per call — s3_persist changes at run time (a recovered timeout)
VitPlan plan_of(const thmr_engine* e, int B) {
    VitPlanIn in{};
    in.mode = e->vit_gemm_mode; in.B = B; in.dec_depth = e->dec_depth;
    in.split_ready = e->split_w && e->split_act && e->pe_s && e->kv_s;
    in.streams = e->s3_ws != nullptr && e->s3_persist;
    in.part_floats = e->so.part_floats;
    return plan_vit(e->knobs, in);
}

// one GEMM as the plan chose it; `part`: the partial planes of a split-K choice
int run_gemm(thmr_engine* e, GemmChoice c, const GemmArgs& a, int epi, float* part, hipStream_t st) {
    switch (c.kind) {
        case THMR_GEMM_F32_TILE: return launch_gemm(a, epi, -1, st);
        case THMR_GEMM_F32_TILE_SPLITK: return launch_gemm_splitk(a, -1, c.ksplit, part, st);
        case THMR_GEMM_F32_RING: return launch_gemm_ring(a, epi, 4, c.ksplit, c.ksplit > 1 ? part : nullptr, st);
        case THMR_GEMM_F32_RING16: return launch_gemm_ring16(a, epi, st);
        case THMR_GEMM_S3_TILE: return launch_gemm_split3(a, epi, -1, st);
        case THMR_GEMM_S3_TILE_SPLITK: return launch_gemm_split3_splitk(a, c.ksplit, part, st);
        case THMR_GEMM_S3_STREAM_WIDE: return launch_gemm_split3_persist(a, epi, a.c_split ? 2 : 0, e->s3_ws, st);   // split3 output: swapped operand roles
        case THMR_GEMM_S3_STREAM_NARROW: return launch_gemm_split3_persist_narrow(a, epi, e->s3_ws, st);
        case THMR_GEMM_S3_SPLITK_STREAM: return launch_gemm_split3_splitk_stream(a, c.ksplit, part, e->s3_ws, st);
#ifdef THMR_EXPERIMENTS
        case THMR_GEMM_S3_RING: return launch_gemm_split3_ring(a, epi, c.ksplit, c.ksplit > 1 ? part : nullptr, st);
#endif
    }
    return -1;
}

// ---------------------------------------------------------------------------------------------- ViT-H
int vit_forward(thmr_engine* e, const float* img, int B, float* feats_out, hipStream_t st) {
    const int M = B * TOK;
    const VitPlan plan = plan_of(e, B);
    float* x = e->S(e->so.x);
    float* h = e->S(e->so.h);
    float* big = e->S(e->so.big);
    float* part = e->S(e->so.part);      // split-K partial sums of proj / fc2, reduced inside the residual + LayerNorm kernel that follows them anyway
    {   // patch embed: crop + pad + im2col, then GEMM (+bias, +pos_embed)   vit.py:341,170-176,327
        ProfScope ps(e, st, THMR_PROF_PATCH, 2.0 * M * 768.0 * DIM,
                     4.0 * (B * 3.0 * 256 * 192 + (double)M * DIM + 768.0 * DIM));
        if (plan.path == THMR_VIT_PATH_SPLIT3) {
            // default mode: the im2col operand written as three bf16 pieces (into the idle fc1 -> fc2 operand buffer) and the Conv2d as a
            // split3 product on the bf16 matrix pipe with the same bias + pos_embed epilogue (0.23 -> ~0.13 ms at 64 crops)
            char* ims = e->split_act + (size_t)M * DIM * 6;
            LAUNCH_OK(launch_im2col_patch_split3(img, ims, B, st));
            GemmArgs a = mk(reinterpret_cast<const float*>(ims), 768, reinterpret_cast<const float*>(e->pe_s), 768, e->hot.pe_b, e->hot.pos, 0, x, DIM, M, DIM, 768);
            a.tile_opts = plan.tile_opts;
            LAUNCH_OK(run_gemm(e, plan.patch, a, EPI_BIAS_POS, nullptr, st));
        } else {
            LAUNCH_OK(launch_im2col_patch(img, big, B, st));
            GemmArgs a = mk(big, 768, e->hot.pe_w, 768, e->hot.pe_b, e->hot.pos, 0, x, DIM, M, DIM, 768);
            LAUNCH_OK(run_gemm(e, plan.patch, a, EPI_BIAS_POS, nullptr, st));
        }
    }
    const float qscale = 1.0f / sqrtf(80.0f);   // head_dim ** -0.5  (vit.py:101)
    // What the plan's three paths differ in.  Every step of a block is written ONCE below, in terms of this; which kernel a GEMM or the
    // attention runs, and every split factor, is the plan's.
    //   THMR_VIT_PATH_F32: exact-fp32 MFMA; the operands h and big live in the scratch arena.
    //   THMR_VIT_PATH_SPLIT3: the four GEMMs as split3 products on the bf16 matrix pipe (csrc/gemm_split.hip); everything else — patch embed,
    //     LayerNorm arithmetic, epilogues — is the fp32 path's.  The LayerNorms, the attention kernel and fc1's GELU epilogue write their
    //     results directly as three bf16 pieces (hs [M][1280], bs [M][5120]): no conversion pass, no fp32 copy of those activations.
    //   THMR_VIT_PATH_SPLIT3_SMALL: EXPERIMENT (experiments library, THMR_SPLIT3_SMALL=1, off by default): a small-batch regime (up to six
    //     crops) of the split3 mode — the ring kernel on split3 operands (64 x 64 tiles, 4-deep LDS-DMA ring; proj / fc2 split K four ways
    //     into `part`, reduced by the residual + LayerNorm kernel as in the fp32 regime), producers writing split3 operands directly.  A
    //     wave's MFMA chain per K tile shrinks from 16 x 64 to 12 x 32 cycles, but the call gets SLOWER: 4.28 vs 3.89 ms at one crop, 6.88 vs
    //     5.84 at two, 16.3 vs 14.1 at six (profiles/r3y_split3_small_batch_regime_ab.log).  At these sizes the GEMMs are bound by the bytes
    //     a CU can keep in flight (three 24 KB stages) against a ~4 us loaded memory round trip, not by the matrix pipe, and split3 operands
    //     are 1.5x the bytes.
    struct VitPath {
        bool s3;                       // operands of the four GEMMs: split3 (6 bytes a value) or fp32
        bool tiled;                    // THMR_VIT_PATH_SPLIT3 itself.  Apart from fc1's profiler sampling it only selects GemmArgs fields that no
                                       // kernel reads (ldr / qscale / qcols of products without that epilogue, ldc next to c_split), kept as they were
        float* a;                      // A of qkv, proj and fc1 = what the LayerNorms and the attention write: hs or h
        float* mid;                    // fc1's destination = fc2's A: bs (through GemmArgs::c_split / ldcs / cs_blk) or big
        float *part_proj, *part_fc2;   // partial planes of a split-K proj / fc2
        int tile_opts;
        int a_blk;                     // fc1 -> fc2 operand in the row-blocked form (plan.bs_blk: fc2 on the 128 x 256 stream)
    };
    const bool s3 = plan.path != THMR_VIT_PATH_F32, tiled = plan.path == THMR_VIT_PATH_SPLIT3;
    // fc2's planes of the split3 path: behind the engine's operand buffers, or (3 and 4 crops: four planes) in the scratch arena's `part`
    float* part2 = tiled && !plan.part2_in_scratch ? reinterpret_cast<float*>(e->split_act + (size_t)e->max_batch * TOK * (DIM + MLP) * 6) : part;
    const VitPath pth{s3, tiled, s3 ? reinterpret_cast<float*>(e->split_act) : h,
                      s3 ? reinterpret_cast<float*>(e->split_act + (size_t)M * DIM * 6) : big, part, part2, tiled ? plan.tile_opts : 0, plan.bs_blk};
    const double ob = pth.s3 ? 6.0 : 4.0;      // bytes of one operand value, for the profiler's accounting
    // y = LayerNorm(x), written as the next GEMM's A operand (as_operand: split3 in the split3 paths) or as fp32 features (last_norm)
    auto norm = [&](const float* g, const float* bt, float* y, bool as_operand) -> int {
        ProfScope ps(e, st, THMR_PROF_LN, 0, (4.0 + ob) * M * DIM);
        if (pth.s3 && as_operand) LAUNCH_OK(launch_layernorm_split3(x, g, bt, y, M, DIM, VIT_EPS, st));
        else LAUNCH_OK(launch_layernorm(x, g, bt, y, M, DIM, VIT_EPS, 0, st));
        return 0;
    };
    // x += Linear(A) + bias;  y = LayerNorm(x)      (vit.py:149 / :150 followed by the next norm): K split into `planes` (few crops on the ring
    // kernel, the mid range on the big tiles / the tile streams) and reduced by the residual + LayerNorm kernel, or unsplit with the residual
    // in the epilogue.  The byte counts are the ones each path has always reported: a split3 path counts its planes, the fp32 path two
    // passes over x whatever the split; fc2's reduce counts an fp32 y even where it writes split3 (open items).
    auto resid_linear_ln = [&](int cls, GemmChoice c, const float* A, int K, const float* Wt, const float* bias, float* planes, int a_blk,
                               const float* g, const float* bt, float* y, bool as_operand) -> int {
        const bool split = c.ksplit > 1;
        {
            ProfScope ps(e, st, cls, 2.0 * M * DIM * (double)K, ob * ((double)M * K + (double)DIM * K) + 4.0 * (pth.s3 && split ? c.ksplit : 2.0) * M * DIM);
            GemmArgs a = split ? mk(A, K, Wt, K, nullptr, nullptr, 0, x, DIM, M, DIM, K) : mk(A, K, Wt, K, bias, x, DIM, x, DIM, M, DIM, K);
            if (pth.tiled && !split) { a.qscale = qscale; a.qcols = DIM; }
            a.a_blk = a_blk;
            a.tile_opts = pth.tile_opts;
            LAUNCH_OK(run_gemm(e, c, a, split ? EPI_NONE : EPI_BIAS_RESID, planes, st));
        }
        if (!split) return norm(g, bt, y, as_operand);
        ProfScope ps(e, st, THMR_PROF_LN, 0, 4.0 * (c.ksplit + 2.0) * M * DIM + (cls == THMR_PROF_GEMM_PROJ ? ob : 4.0) * M * DIM);
        LAUNCH_OK(launch_splitk_resid_ln(planes, c.ksplit, M, DIM, bias, x, x, g, bt, y, VIT_EPS, st, pth.s3 && as_operand));
        return 0;
    };
    if (int rc = norm(e->vitw[0].n1w, e->vitw[0].n1b, pth.a, true)) return rc;
    for (int i = 0; i < e->vit_depth; ++i) {
        const VitBlockW& w = e->vitw[i];
        const bool last = i + 1 == e->vit_depth;
        const float* nxt_w = last ? e->hot.lastn_w : e->vitw[i + 1].n1w;      // the norm that follows this block's fc2
        const float* nxt_b = last ? e->hot.lastn_b : e->vitw[i + 1].n1b;
        const float *wqkv = w.qkvw, *wproj = w.pw, *wfc1 = w.f1w, *wfc2 = w.f2w;      // the block's matrices in the path's operand kind
        if (pth.s3) {
            const thmr_engine::SplitW& ws = e->vitw_s[i];
            wqkv = reinterpret_cast<const float*>(ws.qkv); wproj = reinterpret_cast<const float*>(ws.proj);
            wfc1 = reinterpret_cast<const float*>(ws.fc1); wfc2 = reinterpret_cast<const float*>(ws.fc2);
        }
        {   // qkv Linear; q columns scaled in the epilogue (vit.py:112,116)
            ProfScope ps(e, st, THMR_PROF_GEMM_QKV, 2.0 * M * DIM * 3.0 * DIM, ob * ((double)M * DIM + 3.0 * DIM * DIM) + 12.0 * M * DIM);
            GemmArgs a = mk(pth.a, DIM, wqkv, DIM, w.qkvb, nullptr, pth.tiled ? 3 * DIM : 0, big, 3 * DIM, M, 3 * DIM, DIM);
            a.qscale = qscale; a.qcols = DIM;
            a.tile_opts = pth.tile_opts;
            LAUNCH_OK(run_gemm(e, plan.qkv, a, EPI_BIAS_QSCALE, nullptr, st));
        }
        {   // attention, its output written directly as proj's A operand
            ProfScope ps(e, st, THMR_PROF_ATTN, 4.0 * B * HEADS * 192.0 * 192.0 * 80.0, 4.0 * (3.0 * M * DIM) + ob * M * DIM);
            if (pth.s3) {
                if (plan.attn == THMR_ATTN_B16) LAUNCH_OK(launch_vit_attention_b16(big, pth.a, B, true, 0, st));
                else LAUNCH_OK(launch_vit_attention_split3(big, pth.a, B, st));
            } else {
                if (plan.attn == THMR_ATTN_F32_KEYSPLIT) LAUNCH_OK(launch_vit_attention_keysplit(big, pth.a, B, st));
                else LAUNCH_OK(launch_vit_attention(big, pth.a, B, st));
            }
        }
        // proj + residual, then norm2 (vit.py:123,149,150)
        if (int rc = resid_linear_ln(THMR_PROF_GEMM_PROJ, plan.proj, pth.a, DIM, wproj, w.pb, pth.part_proj, 0, w.n2w, w.n2b, pth.a, true)) return rc;
        {   // fc1 + exact GELU (vit.py:83-84), written as fc2's A operand — in the split3 paths directly as three bf16 pieces: no fp32 copy of
            // the hidden activations exists.  `sampled` (ProfScope): the split3 path has never passed it (open items)
            ProfScope ps(e, st, THMR_PROF_GEMM_FC1, 2.0 * M * DIM * (double)MLP, ob * ((double)M * DIM + (double)DIM * MLP + (double)M * MLP),
                         pth.tiled || (i & 3) == 0);
            GemmArgs a = mk(pth.a, DIM, wfc1, DIM, w.f1b, nullptr, 0, pth.s3 ? nullptr : pth.mid, pth.tiled ? 0 : MLP, M, MLP, DIM);
            if (pth.s3) { a.c_split = pth.mid; a.ldcs = MLP; a.cs_blk = pth.a_blk; }
            a.tile_opts = pth.tile_opts;
            LAUNCH_OK(run_gemm(e, plan.fc1, a, EPI_BIAS_GELU, nullptr, st));
        }
        // fc2 + residual (vit.py:85,150), then the next block's norm1 — or last_norm (vit.py:335), fp32 in every path and kept token-major:
        // the :337 permute is undone by token_head.py:69
        if (int rc = resid_linear_ln(THMR_PROF_GEMM_FC2, plan.fc2, pth.mid, MLP, wfc2, w.f2b, pth.part_fc2, pth.a_blk, nxt_w, nxt_b,
                                     last ? (feats_out ? feats_out : h) : pth.a, !last))
            return rc;
    }
    return 0;
}


// ---------------------------------------------------------------------------------------------- head
// DecodeTokens.forward (tokenization/models/vanilla_pose_vqvae.py:294-297): soft codebook lookup
// (quantize_cnn.py:92-93 dequantize_logits) + PoseSPDecoderV1 (:135-154).  probs (B,160,2048) -> bpose (B,21,6).
// 12 GEMMs and nothing else: every Conv1d(k = 3) is a GEMM over an im2col operand (B*T, 3*C) that the PREVIOUS GEMM's epilogue
// wrote (GemmArgs::cs_*: nearest-resample + taps + zero padding + the ResConv pre-activation ReLU), so no gather launch exists.
// The lookup in front (soft: a GEMM, vq_decode; hard: a kernel, vq_decode_idx) writes the first operand; vq_decode_convs is the rest.
//
// Up to six crops (the small-batch regime, B <= kSmallM / 192) the M = 21 B ... 160 B row products of the VQ decoder run on the tiny-M kernel
// (32x32 tiles, K split over the 8 waves of a workgroup): as 8-24 ring-kernel workgroups walking the whole K they were 13
// dependent launches of 12-32 us, a third of the head at one crop.  One choice for the whole regime: the K association differs.
int vq_tiny_variant(const thmr_engine* e, int B) { return (e->tiny_gemm && B * TOK <= kSmallM) ? 11 : -1; }

// PoseSPDecoderV1 behind the codebook lookup: the operand of decoder.0 (B*160, 3*256) is in the scratch buffer `gat`, written by the soft
// lookup's GEMM (vq_decode) or by the hard lookup kernel (vq_decode_idx, tokenizer_roundtrip) -> bpose (B,21,6)
int vq_decode_convs(thmr_engine* e, int B, float* bpose, hipStream_t st) {
    auto& so = e->so;
    const int tv = vq_tiny_variant(e, B);
    float* G[2] = {e->S(so.gat), e->S(so.gat2)};          // conv operands, alternating
    float *x0 = e->S(so.act0), *x1 = e->S(so.act1), *hid = e->S(so.act2);
    const int32_t* inv = reinterpret_cast<const int32_t*>(e->warena + e->o_inv);
    // what the consumer conv needs from its producer
    auto scatter = [&](GemmArgs& a, float* dst, const int32_t* table, int tin, int tout, int dil, int relu) {
        a.cs_out = dst; a.cs_inv = table; a.cs_tin = tin; a.cs_tout = tout; a.cs_dil = dil; a.cs_relu = relu;
    };
    // the conv itself: operand (B*T, 3*ci) x repacked weight (co, 3*ci)
    auto conv = [&](int id, const float* opnd, int T, const float* bias, float* plain) {
        const int ci = kConv3Ci[id], co = kConv3Co[id];
        return mk(opnd, 3 * ci, e->warena + e->convp[id], 3 * ci, bias, nullptr, 0, plain, co, B * T, co, 3 * ci);
    };
    int cur = 0;
    {   // decoder.0: Conv1d(256 -> 512) + ReLU at T = 160 -> operand of decoder.3 on the 160 -> 125 resample
        GemmArgs a = conv(0, G[cur], 160, e->hot.conv_b[0], nullptr);
        scatter(a, G[cur ^ 1], inv + 0 * 160, 160, e->vq_len[1], 1, 0);
        LAUNCH_OK(launch_gemm(a, EPI_BIAS_RELU, tv, st));
        cur ^= 1;
    }
    for (int i = 0; i < 4; ++i) {   // decoder.3/6/9/12: nn.Upsample(size) (a down-sampling here) + Conv1d(512 -> 512) + ReLU
        const int T = e->vq_len[i + 1];
        GemmArgs a = conv(1 + i, G[cur], T, e->hot.conv_b[1 + i], i == 3 ? x0 : nullptr);
        if (i < 3) scatter(a, G[cur ^ 1], inv + (i + 1) * 160, T, e->vq_len[i + 2], 1, 0);
        else scatter(a, G[cur ^ 1], nullptr, VQJ, VQJ, 3, 1);      // -> ResConv1DBlock 0 (dilation 3, pre-activation ReLU); x0 kept as its residual
        LAUNCH_OK(launch_gemm(a, EPI_BIAS_RELU, tv, st));
        cur ^= 1;
    }
    const int Tq = VQJ;
    float* res = x0;
    float* nres = x1;
    for (int blk = 0; blk < 2; ++blk) {   // ResConv1DBlock, resnet.py:49-69: x + conv2(relu(conv1(relu(x)))), dilation 3 then 1
        {
            GemmArgs a = conv(5 + blk, G[cur], Tq, e->hot.conv_b[5 + blk], hid);
            LAUNCH_OK(launch_gemm(a, EPI_BIAS_RELU, tv, st));
        }
        GemmArgs a = mk(hid, VQW, e->hot.res_w[blk], VQW, e->hot.res_b[blk], res, VQW, blk == 0 ? nres : nullptr, VQW, B * Tq, VQW, VQW);
        // block 0 feeds block 1's conv1 (pre-activation ReLU) and stays its residual; block 1 feeds decoder.14.1 (no activation)
        scatter(a, G[cur ^ 1], nullptr, Tq, Tq, 1, blk == 0 ? 1 : 0);
        LAUNCH_OK(launch_gemm(a, EPI_BIAS_RESID, tv, st));
        cur ^= 1;
        std::swap(res, nres);
    }
    {   // decoder.14.1: Conv1d(512 -> 512) -> operand of decoder.15
        GemmArgs a = conv(7, G[cur], Tq, e->hot.conv_b[7], nullptr);
        scatter(a, G[cur ^ 1], nullptr, Tq, Tq, 1, 0);
        LAUNCH_OK(launch_gemm(a, EPI_BIAS, tv, st));
        cur ^= 1;
    }
    GemmArgs a = conv(8, G[cur], Tq, e->hot.conv_b[8], bpose);    // decoder.15: Conv1d(512 -> 6): the 21 x 6D body pose
    LAUNCH_OK(launch_gemm(a, EPI_BIAS, tv, st));
    return 0;
}

int vq_decode(thmr_engine* e, const float* probs, int B, float* bpose, hipStream_t st) {
    // soft codebook lookup: probs @ codebook as a GEMM against codebook^T -> operand of decoder.0 (T = 160, C = 256)
    GemmArgs a = mk(probs, NCLS, e->warena + e->o_cbT, NCLS, nullptr, nullptr, 0, nullptr, CODE, B * TN, CODE, NCLS);
    a.cs_out = e->S(e->so.gat); a.cs_inv = nullptr; a.cs_tin = 160; a.cs_tout = 160; a.cs_dil = 1; a.cs_relu = 0;
    LAUNCH_OK(launch_gemm(a, EPI_NONE, vq_tiny_variant(e, B), st));
    return vq_decode_convs(e, B, bpose, st);
}

// hard codebook lookup (QuantizeEMAReset.dequantize, quantize_cnn.py:88-90) -> the same operand; x = null: the code rows themselves,
// else the straight-through value x + (c - x) of quantize_cnn.py:124.  A bad index sets the engine's host-mapped flag word [2].
int vq_decode_idx(thmr_engine* e, const int32_t* idx, const float* x, int B, float* bpose, hipStream_t st) {
    LAUNCH_OK(launch_vq_lookup(idx, x, e->hot.codebook, e->S(e->so.gat), B, e->host_err ? e->host_err + 2 : nullptr, st));
    return vq_decode_convs(e, B, bpose, st);
}

int head_forward(thmr_engine* e, const float* ctx, int B, const thmr_outputs* out, hipStream_t st) {
    auto& so = e->so;
    const int M = B * TOK;
    float* big = e->S(so.big);
    const int ldkv = e->dec_depth * 2 * INNER;
    {   // K8: to_kv of all decoder layers in ONE GEMM on the un-normalised context (pose_transformer.py:102,113)
        ProfScope ps(e, st, THMR_PROF_DEC_KV, 2.0 * M * DIM * (double)ldkv, 4.0 * ((double)M * DIM + (double)ldkv * DIM + (double)M * ldkv));
        const VitPlan plan = plan_of(e, B);
        if (plan.to_kv.kind != THMR_GEMM_F32_TILE) {
            // split3 mode: the context (fp32: it may be a caller's buffer) converted into the ViT's idle operand buffer, then the same product
            // on the bf16 matrix pipe (1.5 -> 1.0 ms at 64 crops)
            LAUNCH_OK(launch_split3(ctx, DIM, e->split_act, DIM, M, DIM, st));
            GemmArgs a = mk(reinterpret_cast<const float*>(e->split_act), DIM, reinterpret_cast<const float*>(e->kv_s), DIM, nullptr, nullptr, 0, big, ldkv, M, ldkv, DIM);
            a.tile_opts = plan.tile_opts;
            LAUNCH_OK(run_gemm(e, plan.to_kv, a, EPI_NONE, nullptr, st));
        } else {
            GemmArgs a = mk(ctx, DIM, e->warena + e->o_kv_all, DIM, nullptr, nullptr, 0, big, ldkv, M, ldkv, DIM);
            LAUNCH_OK(run_gemm(e, plan.to_kv, a, EPI_NONE, nullptr, st));
        }
    }
    ProfScope ps_head(e, st, THMR_PROF_HEAD, e->hmr2 ? 2.0 * B * (6.0 * 4.2e6 + 0.16e6) : 2.0 * B * (6.0 * 4.2e6 + 116.7e6 + 167.8e6 + 705.0e6), 0);
    float *dx = e->S(so.dx), *dh = e->S(so.dh), *dv = e->S(so.dv), *dq = e->S(so.dq), *dca = e->S(so.dca), *dff = e->S(so.dff);
    float* ro = e->S(so.ro);
    float *mt = e->S(so.mt), *cf = e->S(so.cf), *cf2 = e->S(so.cf2);
    const bool fused_head = !e->legacy_head && B <= kFusedHeadMaxB;
    bool mixer_in_decoder = false;
    if (fused_head) {
        // ONE persistent kernel: layer-0 input, the 6 decoder layers (42 dependent GEMV-class steps), the read-outs and the
        // classifier's first Linear (decoder_fused.hip)
        DecParams d = e->dec;
        d.B = B;
        if (e->hmr2) {
            // the same persistent kernel with the stacked read-out as its last step (decoder_fused.hip, THMR_HEAD_HMR2)
            d.mixer_cluster = 0;
            LAUNCH_OK(launch_decoder_fused(d, st, THMR_HEAD_HMR2));
        } else {
            // the MLP-Mixer stack runs inside the same kernel, 10 / 5 / 2 workgroups per crop while they fit one per CU (up to 25 / 51 /
            // 128 crops on 256 CUs; decoder_fused.hip mixer_cluster_stage, bit-identical to mixer_stack_kernel's one workgroup per crop)
            const int slots = d.max_blocks < 256 ? d.max_blocks : 256;
            d.mixer_cluster = !e->mixer_cluster ? 0 : 10 * B <= slots ? 10 : 5 * B <= slots ? 5 : 2 * B <= slots ? 2 : 0;
            mixer_in_decoder = d.mixer_cluster != 0;
            d.mx = e->mix;
            d.mixy[0] = cf; d.mixy[1] = cf2;
            LAUNCH_OK(launch_decoder_fused(d, st));            // the caller's Turn (thmr_forward / thmr_head_forward) orders engines
        }
    } else {
    // the launch chain: the same weights the persistent kernels read (e->dec, e->mix: resolved by resolve_weights)
    LAUNCH_OK(launch_decoder_init(e->dec.tok_bias, e->dec.pos, dx, B, E, st));
    for (int l = 0; l < e->dec_depth; ++l) {
        const DecLayerW& w = e->dec.L[l];
        // self-attention over ONE token: softmax of a single score == 1, so out = to_out(v)  (pose_transformer.py:75-86)
        LAUNCH_OK(launch_layernorm(dx, w.n0w, w.n0b, dh, B, E, LN_EPS, 0, st));
        {
            GemmArgs a = mk(dh, E, w.wv, E, nullptr, nullptr, 0, dv, INNER, B, INNER, E);
            LAUNCH_OK(launch_gemm_skinny(a, EPI_NONE, st));
        }
        {
            GemmArgs a = mk(dv, INNER, w.wo1, INNER, w.bo1, dx, E, dx, E, B, E, INNER);
            LAUNCH_OK(launch_gemm_skinny(a, EPI_BIAS_RESID, st));
        }
        // cross-attention (pose_transformer.py:111-124)
        LAUNCH_OK(launch_layernorm(dx, w.n1w, w.n1b, dh, B, E, LN_EPS, 0, st));
        {
            GemmArgs a = mk(dh, E, w.wq, E, nullptr, nullptr, 0, dq, INNER, B, INNER, E);
            LAUNCH_OK(launch_gemm_skinny(a, EPI_NONE, st));
        }
        LAUNCH_OK(launch_cross_attn(dq, big, ldkv, l * 2 * INNER, dca, B, st));
        {
            GemmArgs a = mk(dca, INNER, w.wo2, INNER, w.bo2, dx, E, dx, E, B, E, INNER);
            LAUNCH_OK(launch_gemm_skinny(a, EPI_BIAS_RESID, st));
        }
        // feed-forward (pose_transformer.py:40-52)
        LAUNCH_OK(launch_layernorm(dx, w.n2w, w.n2b, dh, B, E, LN_EPS, 0, st));
        {
            GemmArgs a = mk(dh, E, w.w1, E, w.b1, nullptr, 0, dff, DEC_MLP, B, DEC_MLP, E);
            LAUNCH_OK(launch_gemm_skinny(a, EPI_BIAS_GELU, st));
        }
        {
            GemmArgs a = mk(dff, DEC_MLP, w.w2, DEC_MLP, w.b2, dx, E, dx, E, B, E, DEC_MLP);
            LAUNCH_OK(launch_gemm_skinny(a, EPI_BIAS_RESID, st));
        }
    }
    if (e->hmr2) {
        // the stacked read-out of the HMR2 head (smpl_head.py:82-84): one (160, 1024) GEMV-class GEMM, zero rows included
        GemmArgs a = mk(dx, E, e->warena + e->o_ro_w, E, e->warena + e->o_ro_b, nullptr, 0, ro, THMR_HMR2_RO_LD, B, THMR_HMR2_RO_LD, E);
        LAUNCH_OK(launch_gemm_skinny(a, EPI_BIAS, st));
    } else {
        // read-outs: one (31,1024) GEMV-class GEMM (token_head.py:99-105)
        {
            GemmArgs a = mk(dx, E, e->warena + e->o_ro_w, E, e->warena + e->o_ro_b, nullptr, 0, ro, 32, B, 31, E);
            LAUNCH_OK(launch_gemm_skinny(a, EPI_BIAS, st));
        }
        // token classifier (token_classifier.py:89-104)
        {
            GemmArgs a = mk(dx, E, e->dec.mt_w, E, e->dec.mt_b, nullptr, 0, mt, TN * HID, B, TN * HID, E);
            LAUNCH_OK(launch_gemm_skinny(a, EPI_BIAS, st));
        }
    }
    }   // the launch chain
    if (out && out->token_out) HIP_OK(hipMemcpyAsync(out->token_out, dx, sizeof(float) * B * E, hipMemcpyDeviceToDevice, st));
    if (e->hmr2) {
        // the finish: mean parameters, 6D -> rotation matrices of all 24 joints, camera (hmr2_head.hip) — the second and last launch
        // behind the to_kv GEMM in the fused form
        float* rot = (out && out->rotmat) ? out->rotmat : e->S(so.rot);
        float* betas = (out && out->betas) ? out->betas : e->S(so.betas);
        float* cam = (out && out->pred_cam) ? out->pred_cam : e->S(so.cam);
        float* camt = (out && out->pred_cam_t) ? out->pred_cam_t : e->S(so.camt);
        LAUNCH_OK(launch_hmr2_finish(ro, THMR_HMR2_RO_LD, e->hot.init_pose, e->hot.init_betas, e->hot.init_cam, out ? out->pose6d : nullptr,
                                     rot, betas, cam, camt, out ? out->focal_length : nullptr, FOCAL, IMG, B, st));
        return 0;
    }
    const int R = B * TN;
    float *nl = e->S(so.nl), *nl2 = e->S(so.nl2);
    if (fused_head) {
        // ONE kernel, one workgroup per crop: mixer_trans LayerNorm + ReLU, the 4 MixerLayers, mixer_norm_layer (mixer_fused.hip)
        if (!mixer_in_decoder) LAUNCH_OK(launch_mixer_fused(e->mix, B, st));
    } else {
        LAUNCH_OK(launch_layernorm(mt, e->mix.tln_w, e->mix.tln_b, cf, B, TN * HID, LN_EPS, 1, st));
        for (int m = 0; m < MIX; ++m) {   // MixerLayer, heads/modules.py:55-63
            const MixerLayerW& w = e->mix.L[m];
            float *y1 = e->S(so.y1), *tT = e->S(so.tT), *u = e->S(so.u), *yt = e->S(so.yt), *y = e->S(so.y), *s = e->S(so.s),
                  *z0 = e->S(so.z0), *zh = e->S(so.zh);
            LAUNCH_OK(launch_layernorm(cf, w.ln1w, w.ln1b, y1, R, HID, LN_EPS, 0, st));
            LAUNCH_OK(launch_transpose(y1, tT, B, TN, HID, st));                                   // (B,160,64)->(B,64,160)
            {
                GemmArgs a = mk(tT, TN, w.wt1, TN, w.bt1, nullptr, 0, u, TOK_INTER, B * HID, TOK_INTER, TN);
                LAUNCH_OK(launch_gemm(a, EPI_BIAS_GELU, -1, st));
            }
            {
                GemmArgs a = mk(u, TOK_INTER, w.wt2, TOK_INTER, w.bt2, nullptr, 0, yt, TN, B * HID, TN, TOK_INTER);
                LAUNCH_OK(launch_gemm(a, EPI_BIAS, -1, st));
            }
            LAUNCH_OK(launch_transpose(yt, y, B, HID, TN, st));                                    // (B,64,160)->(B,160,64)
            LAUNCH_OK(launch_add_ln64(cf, y, w.ln2w, w.ln2b, s, z0, R, LN_EPS, st));
            {
                GemmArgs a = mk(z0, HID, w.wc1, HID, w.bc1, nullptr, 0, zh, HID_INTER, R, HID_INTER, HID);
                LAUNCH_OK(launch_gemm(a, EPI_BIAS_GELU, -1, st));
            }
            {   // out = (x + y) + z
                GemmArgs a = mk(zh, HID_INTER, w.wc2, HID_INTER, w.bc2, s, HID, cf2, HID, R, HID, HID_INTER);
                LAUNCH_OK(launch_gemm(a, EPI_BIAS_RESID, -1, st));
            }
            std::swap(cf, cf2);
        }
        {
            GemmArgs a = mk(cf, HID, e->mix.wn, HID, e->mix.bn, nullptr, 0, nl, HID, R, HID, HID);
            LAUNCH_OK(launch_gemm(a, EPI_BIAS, -1, st));
        }
        LAUNCH_OK(launch_layernorm(nl, e->mix.nln_w, e->mix.nln_b, nl2, R, HID, LN_EPS, 1, st));
    }
    // logits / softmax / token index; KV in `big` is dead after the decoder, so logits+probs live there
    float* logits = (out && out->cls_logits) ? out->cls_logits : big;
    float* probs = (out && out->cls_logits_softmax) ? out->cls_logits_softmax : big + (size_t)R * NCLS;
    int32_t* tokidx = (out && out->token_idx) ? out->token_idx : reinterpret_cast<int32_t*>(e->S(so.tokidx));
    {
        GemmArgs a = mk(nl2, HID, e->hot.cls_w, HID, e->hot.cls_b, nullptr, 0, logits, NCLS, R, NCLS, HID);
        LAUNCH_OK(launch_gemm(a, EPI_BIAS, -1, st));
    }
    LAUNCH_OK(launch_softmax_argmax2048(logits, probs, tokidx, R, st));
    float* bpose = e->S(so.bpose);
    if (int r = vq_decode(e, probs, B, bpose, st)) return r;
    // assemble + rot6d + camera (token_head.py:103-127, tokenhmr.py:165-169)
    float* rot = (out && out->rotmat) ? out->rotmat : e->S(so.rot);
    float* betas = (out && out->betas) ? out->betas : e->S(so.betas);
    float* cam = (out && out->pred_cam) ? out->pred_cam : e->S(so.cam);
    float* camt = (out && out->pred_cam_t) ? out->pred_cam_t : e->S(so.camt);
    LAUNCH_OK(launch_assemble(ro, 32, bpose, e->hot.init_pose, e->hot.init_betas, e->hot.init_cam,
                              out ? out->pose6d : nullptr, rot, betas, cam, camt,
                              out ? out->focal_length : nullptr, FOCAL, IMG, B, st));
    return 0;
}

int lbs(thmr_engine* e, const float* rot, const float* betas, const float* camt, int B, float* verts, float* joints,
        float* kp2d, hipStream_t st) {
    auto& so = e->so;
    ProfScope ps(e, st, THMR_PROF_LBS, 2.0 * B * 8.1e6, 4.0 * (B * (NV * 3.0 + 132 + 226) + 4.95e6));
    LbsArgs a{};
    e->smpl.fill(a, e->warena);
    a.rotmat = rot; a.betas = betas; a.cam_t = camt;
    a.A = e->S(so.A); a.xf = e->S(so.pf); a.Jtr = e->S(so.Jtr); a.vposed = e->S(so.vposed); a.xv = e->S(so.xv);
    a.cnt = reinterpret_cast<unsigned*>(e->S(so.lcnt));
    a.verts = verts ? verts : e->S(so.verts); a.joints = joints; a.kp2d = kp2d;
    a.focal_over_size = FOCAL / IMG; a.B = B;
    LAUNCH_OK(launch_lbs(a, st));
    return 0;
}

// nn.Upsample nearest index tables of the VQ decoder / tokenizer encoder, evaluated in fp32 exactly like ATen
// (nearest_neighbor_compute_source_index: min(floor(dst * (float)in / out), in - 1)).  They are part of the weight arena
// (so a broadcast replicates them) and are written by the engine that LOADED the weights — never by thmr_create, which
// may be handed another engine's live arena (Engine(weight_arena=...)).
void build_idx_tables(thmr_engine* e) {
    e->idx_host.assign(4 * 160, 0);
    for (int i = 0; i < 4; ++i) {
        const int tin = e->vq_len[i], tout = e->vq_len[i + 1];
        const float scale = (float)tin / (float)tout;
        for (int t = 0; t < tout; ++t) {
            int sidx = (int)floorf((float)t * scale);
            e->idx_host[i * 160 + t] = sidx < tin - 1 ? sidx : tin - 1;
        }
    }
    // inverse tables of the decoder's four down-samplings: position ts of the producer -> the resampled position tp that reads it
    // (src is strictly increasing, so at most one), -1 = dropped.  Used by the GEMM epilogue that writes the next conv's operand.
    e->inv_host.assign(4 * 160, -1);
    for (int i = 0; i < 4; ++i)
        for (int t = 0; t < e->vq_len[i + 1]; ++t) e->inv_host[i * 160 + e->idx_host[i * 160 + t]] = t;
    // encoder: nn.Upsample(size=40) from 21 (offset 0), then three nn.Upsample(scale_factor=2)
    // (ATen uses scale 1/scale_factor = 0.5: src = floor(dst*0.5)): 40->80 (offset 40), 80->160 (120), 160->320 (280)
    e->eidx_host.assign(640, 0);
    const float sc = 21.0f / 40.0f;
    for (int t = 0; t < 40; ++t) { int s0 = (int)floorf((float)t * sc); e->eidx_host[t] = s0 < 20 ? s0 : 20; }
    int o = 40;
    for (int tin = 40; tin <= 160; tin *= 2) {
        for (int t = 0; t < 2 * tin; ++t) { int s0 = (int)floorf((float)t * 0.5f); e->eidx_host[o + t] = s0 < tin - 1 ? s0 : tin - 1; }
        o += 2 * tin;
    }
}
constexpr int32_t kEncMagic = 0x454e4331;   // 'ENC1': arena flag word 0 = "tokenizer encoder tensors present"
constexpr int32_t kArenaMagic = 0x54484d32; // 'THM2': arena flag word 1 = "the non-checkpoint regions below were written by a loading engine"
constexpr int32_t kArenaMagicHmr2 = 0x48324d32; // 'H2M2': the same for an arena in the HMR2 head's layout (THMR_CFG_HEAD_HMR2)

// Everything in the weight arena that is neither a checkpoint tensor nor derived from one: the resample index tables, the zero
// padding row of the read-out matrix and the flag words.  Written by the engine that LOADS tensors, at load time — so the arena
// is complete for a broadcast the moment loading ends, whether or not the root has finalized yet (round 2 wrote them in
// thmr_finalize_weights(assume_all_loaded = 0) only: a root that broadcast BEFORE finalizing shipped uninitialised tables, and
// receivers, which finalize with assume_all_loaded = 1, never wrote them).  Receivers validate kArenaMagic instead of writing:
// their arena may be another engine's live one (Engine(weight_arena=...)).
int write_arena_constants(thmr_engine* e, hipStream_t st) {
    if (e->hmr2) {
        // HMR2 head: the zero rows / zero biases that pad the stacked read-out to whole 16-column tiles, and the magic word
        HIP_OK(hipMemsetAsync(e->warena + e->o_ro_w + (size_t)THMR_HMR2_RO_ROWS * E, 0, (size_t)(THMR_HMR2_RO_LD - THMR_HMR2_RO_ROWS) * E * sizeof(float), st));
        HIP_OK(hipMemsetAsync(e->warena + e->o_ro_b + THMR_HMR2_RO_ROWS, 0, (THMR_HMR2_RO_LD - THMR_HMR2_RO_ROWS) * sizeof(float), st));
        e->flag_host[0] = 0;
        e->flag_host[1] = kArenaMagicHmr2;
        HIP_OK(hipMemcpyAsync(e->warena + e->o_flags, e->flag_host, 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
        return 0;
    }
    build_idx_tables(e);
    HIP_OK(hipMemcpyAsync(e->warena + e->o_idx, e->idx_host.data(), e->idx_host.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(e->warena + e->o_inv, e->inv_host.data(), e->inv_host.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(e->warena + e->o_idx_enc, e->eidx_host.data(), e->eidx_host.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(e->warena + e->o_ro_w + (size_t)31 * E, 0, E * sizeof(float), st));
    // optional encoder: present only when every 'encoder.encoder.*' tensor arrived (all-or-nothing, checked by finalize)
    size_t enc_loaded = 0;
    for (auto& n : e->enc_names) enc_loaded += e->slots[n].loaded ? 1 : 0;
    e->flag_host[0] = enc_loaded == e->enc_names.size() ? kEncMagic : 0;
    e->flag_host[1] = kArenaMagic;
    HIP_OK(hipMemcpyAsync(e->warena + e->o_flags, e->flag_host, 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
    return 0;
}

// The persistent kernels need ALL their workgroups resident at once: the decoder kernel has a grid barrier and, from 49 crops on, asks
// for every CU; the persistent split3 GEMM's consumers wait for slabs their producers publish, one 147 KB workgroup per CU.  Two such
// launches issued concurrently by two engines on two streams could each grab part of the chip and wait for the rest until the bounded
// waits run out.  So when a process has more than one engine on a device, their forward-type calls are chained through one event per
// device (struct Turn below: one wait + one record per CALL since round 6, not per launch): each call waits for the previous one (of any
// engine) to finish.  One engine (the normal case) never touches the event, and a capturing stream does not either (an event from outside
// a capture cannot be waited on).  ANOTHER PROCESS on the same GPU is outside this protection: see THMR_CFG_NO_PERSISTENT (header).  (Engines of the shipped and of the experiments
// library in one process each have their own copy of this object: do not run them concurrently on one device — tests do not.)
struct DecoderTurnstile {
    std::mutex mu;
    std::map<int, int> engines;          // device -> live engines
    std::map<int, hipEvent_t> last;      // device -> event recorded at the end of the most recent forward-type call of any engine
};
DecoderTurnstile& turnstile() {
    static DecoderTurnstile t;
    return t;
}

// One TURN per forward-type call (round 6, ADVICE r5: round 5 took the mutex and waited / recorded the event around EVERY persistent launch,
// 33 and more per forward).  With more than one engine of this library on the device and no capture in progress, the call's stream first
// waits for the event the previous call (of any engine) recorded at its end, and records it again at its own end; the mutex is held for the
// host-side enqueue of the whole call (~0.3 ms), so two threads cannot both wait on the same earlier record and then overlap.  Whole
// forwards of different engines therefore run one after the other on the device — which is what kernels that need all 256 CUs resident
// amount to anyway.  One engine per device (the normal case): no lock held, no event touched.
struct Turn {
    std::unique_lock<std::mutex> lk;
    hipStream_t st = nullptr;
    hipEvent_t ev = nullptr;
    int rc = 0;
    Turn(thmr_engine* e, hipStream_t s) : lk(turnstile().mu), st(s) {
        DecoderTurnstile& t = turnstile();
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (t.engines[e->cfg.device] <= 1 || hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
            lk.unlock();
            return;
        }
        auto it = t.last.find(e->cfg.device);
        if (it == t.last.end()) {
            hipEvent_t nev;
            if (hipEventCreateWithFlags(&nev, hipEventDisableTiming) != hipSuccess) { rc = -2; lk.unlock(); return; }
            it = t.last.emplace(e->cfg.device, nev).first;
        } else if (hipStreamWaitEvent(st, it->second, 0) != hipSuccess) { rc = -2; lk.unlock(); return; }
        ev = it->second;
    }
    // records the end of the turn; returns -2 if the record failed (the launches themselves were fine)
    int end() {
        int r = 0;
        if (ev) {
            if (hipEventRecord(ev, st) != hipSuccess) r = -2;
            ev = nullptr;
        }
        if (lk.owns_lock()) lk.unlock();
        return r;
    }
    ~Turn() { (void)end(); }
};

// split3 weight copies are a pure function of the weight arena's contents: engines that SHARE an arena (thmr_create with the same
// weight_arena_dev, e.g. several engines of one process on one GPU) share ONE copy, reference-counted (round 6, ADVICE r5: eight engines on
// one device held 30 GB of duplicates).  Every finalize still runs the conversion into it — idempotent, the same bytes.
struct SplitShare {
    std::mutex mu;
    struct Ent { char* p; size_t bytes; int refs; };
    std::map<std::pair<int, const void*>, Ent> m;
};
SplitShare& split_share() {
    static SplitShare s;
    return s;
}

// The persistent decoder kernel's bounded grid barrier timed out in an earlier call (its workgroups were not resident together:
// another process on the GPU, a partition with fewer CUs than reported ...).  That call's outputs are garbage and its barrier
// words are in an undefined state.  Recover instead of staying poisoned: drain the device, zero the barrier words and the
// sticky error, and run this engine's head as the launch chain from now on (it needs no co-residency), so the caller can
// simply re-submit.  Returns the error ONCE.
int recover_decoder_timeout(thmr_engine* e, hipStream_t st = nullptr) {
    // hipDeviceSynchronize / hipMemset are illegal while a stream of this thread is being captured into a hipGraph (they would also
    // invalidate the capture): report, leave the device alone, and let the caller recover outside the capture
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (st != nullptr && hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return fail(e, THMR_ERR_HIP, "persistent decoder kernel: grid barrier timed out in a previous forward, and this call is inside a "
                                     "stream capture: end the capture, call thmr_engine_status() (it resets the engine), then re-capture");
    (void)hipDeviceSynchronize();
    (void)hipMemset(e->sarena + e->so.sync, 0, 512 * sizeof(float));
    if (e->host_err) *e->host_err = 0;
    e->legacy_head = true;
    return fail(e, THMR_ERR_HIP, "persistent decoder kernel: grid barrier timed out in a previous forward (its workgroups could not be "
                                 "resident together); that call's outputs are invalid.  The engine has reset its barrier and switched to "
                                 "the launch-chain head: re-submit the batch");
}

// zero the hand-over workspace of the persistent split3 GEMM (slabs, epochs, control words) and bind the host-mapped error word again
int reset_s3_workspace(thmr_engine* e, hipStream_t st) {
    HIP_OK(hipMemsetAsync(e->s3_ws, 0, gemm_split3_persist_ws_bytes(), st));
    if (e->s3_host_err && gemm_split3_persist_bind_host_err(e->s3_ws, &e->s3_host_err, st) != 0)
        return fail(e, THMR_ERR_HIP, "binding the host-mapped error word of the split3 hand-over workspace failed");
    return 0;
}

// A consumer of the persistent split3 GEMM gave up waiting for its producer's slab in an earlier call (the launch's workgroups were not
// resident together for ~0.5 s: another kernel held the device).  That call's outputs are invalid.  The epochs in the flags make later
// launches safe by themselves (a late producer cannot be mistaken for a later launch's), but the cause is likely to persist: report ONCE,
// reset the workspace and fall back to the one-workgroup-per-tile kernel (same results), so the caller can simply re-submit.
int recover_split3_timeout(thmr_engine* e, hipStream_t st = nullptr) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (st != nullptr && hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return fail(e, THMR_ERR_HIP, "persistent split3 GEMM: a hand-over wait timed out in a previous forward, and this call is inside a "
                                     "stream capture: end the capture, call thmr_engine_status() (it resets the engine), then re-capture");
    (void)hipDeviceSynchronize();
    if (e->s3_host_err) *e->s3_host_err = 0;
    e->s3_persist = 0;
    if (e->s3_ws) {
        if (int r = reset_s3_workspace(e, nullptr)) return r;
        (void)hipDeviceSynchronize();
    }
    return fail(e, THMR_ERR_HIP, "persistent split3 GEMM: a hand-over wait timed out in a previous forward; that call's outputs are invalid. "
                                 "The engine has reset the workspace and switched to the per-tile kernel: re-submit the batch");
}

int check_ready(thmr_engine* e, int B, hipStream_t st = nullptr) {
    if (!e) return fail(nullptr, THMR_ERR_INVALID, "null engine");
    if (e->host_err && *static_cast<volatile unsigned*>(e->host_err) != 0) return recover_decoder_timeout(e, st);
    if (e->s3_host_err && *static_cast<volatile unsigned*>(e->s3_host_err) != 0) return recover_split3_timeout(e, st);
    if (!e->finalized) return fail(e, THMR_ERR_STATE, "weights not finalized: call thmr_finalize_weights first");
    if (B < 1 || B > e->max_batch) return fail(e, THMR_ERR_INVALID, "batch " + std::to_string(B) + " outside [1, max_batch=" + std::to_string(e->max_batch) + "]");
    return 0;
}

}  // namespace

// =============================================================================================== C ABI
extern "C" {

int thmr_abi_version(void) { return THMR_ABI_VERSION; }
#ifndef THMR_SRC_HASH
#define THMR_SRC_HASH "unhashed"      // __graft_entry__.build() passes the content hash of csrc/ + include/ + flags
#endif
#ifdef THMR_EXPERIMENTS
#define THMR_BUILD_KIND " experiments"      // environment knobs, debug hooks and the kernels that lost their A/B (csrc/common.h)
#else
#define THMR_BUILD_KIND ""
#endif
const char* thmr_build_info(void) { return "tokenhmr_hip gfx950 fp32-mfma src:" THMR_SRC_HASH THMR_BUILD_KIND " " __DATE__ " " __TIME__; }

const char* thmr_last_error(const thmr_engine* e) { return e ? e->err.c_str() : g_last_error.c_str(); }

static int validate_cfg(const thmr_config* cfg) {
    if (!cfg) return fail(nullptr, THMR_ERR_INVALID, "null config");
    if (cfg->abi_version != THMR_ABI_VERSION) return fail(nullptr, THMR_ERR_INVALID, "abi_version mismatch");
    if (cfg->vit_depth < 1 || cfg->vit_depth > 64 || cfg->dec_depth < 1 || cfg->dec_depth > 6 || cfg->max_batch < 1 ||
        cfg->max_batch > 4096)
        return fail(nullptr, THMR_ERR_INVALID, "config out of range (vit_depth 1..64, dec_depth 1..6, max_batch 1..4096)");
    if ((cfg->flags & ~(THMR_CFG_VIT_GEMM_F32 | THMR_CFG_NO_PERSISTENT | THMR_CFG_HEAD_HMR2)) != 0 || cfg->reserved[0] != 0 || cfg->reserved[1] != 0)
        return fail(nullptr, THMR_ERR_INVALID, "unknown config flag / non-zero reserved field");
    return 0;
}

// the plan's knobs: their defaults in the shipped library (thmr_knob is a constant nullptr there), THMR_* environment variables in the
// experiments build
static VitKnobs read_knobs() {
    VitKnobs k;
#ifdef THMR_EXPERIMENTS
    auto off = [](const char* name) { const char* v = thmr_knob(name); return v && v[0] == '0'; };
    auto on = [](const char* name) { const char* v = thmr_knob(name); return v && v[0] == '1'; };
    auto num = [](const char* name, int& dst) { if (const char* v = thmr_knob(name)) dst = atoi(v); };
    auto digit = [](const char* name, char hi, int& dst) { const char* v = thmr_knob(name); if (v && v[0] >= '0' && v[0] <= hi) dst = v[0] - '0'; };
    k.qkv_ring16 = !off("THMR_QKV_RING16");
    k.attn_keysplit = !off("THMR_ATTN_KEYSPLIT");
    if (on("THMR_ATTN_B16") || off("THMR_ATTN_B16")) k.attn_b16 = on("THMR_ATTN_B16");
    k.split3_small = on("THMR_SPLIT3_SMALL");
    if (on("THMR_SPLIT3_FC2_SPLIT")) k.split3_fc2_split = 1;
    num("THMR_SPLIT3_MIN_B", k.split3_min_b);
    k.tile_opts = (on("THMR_SPLIT3_NARROW8") ? 1 : 0) | (on("THMR_SPLIT3_TAIL8") ? 2 : 0) | (off("THMR_SPLIT3_RING3") ? 4 : 0) | (off("THMR_SPLIT3_FRONT") ? 8 : 0);
    num("THMR_SPLIT3_PN_MASK", k.pn_mask);
    num("THMR_SPLIT3_PN_MAX", k.pn_max);
    num("THMR_SPLIT3_PN_FILL", k.pn_fill);
    num("THMR_SPLIT3_PK_MAX", k.pk_max);
    num("THMR_SPLIT3_PN_FILL_PROJ", k.pn_fill_proj);
    num("THMR_SPLIT3_PW_FILL", k.pw_fill);
    if (off("THMR_SPLIT3_PW_FC1")) k.pw_fc1 = 0;
    digit("THMR_SPLIT3_PERSIST", '1', k.persist);
    digit("THMR_SPLIT3_FC1_MODE", '2', k.fc1_mode);
    num("THMR_SPLIT3_PERSIST_MASK", k.persist_mask);
    k.bs_blk = !off("THMR_SPLIT3_BS_BLK");
    if (const char* ms = thmr_knob("THMR_MID_SPLIT")) {
        if (ms[0] && ms[1]) { k.mid_split_force[0] = ms[0] - '0'; k.mid_split_force[1] = ms[1] - '0'; }
    }
#endif
    return k;
}

// bytes of the engine-owned allocations of the split3 mode (build_split_weights): weight copies, activation operands + fc2's split-K planes
static size_t split_w_bytes_of(int vit_depth, int dec_depth) {
    const size_t per_block = (size_t)DIM * (3 * DIM) + (size_t)DIM * DIM + 2 * (size_t)DIM * MLP;      // weights of one block
    const size_t kv_rows = (size_t)dec_depth * 2 * INNER;                                              // + the decoder's to_kv of all layers
    return (per_block * vit_depth + kv_rows * DIM + (size_t)DIM * 768) * 6;                            // + the patch-embed matrix
}
static size_t split_act_bytes_of(int max_batch) {
    const size_t M = (size_t)max_batch * TOK;
    return M * (size_t)(DIM + MLP) * 6 + (size_t)kSplit3Fc2Split * M * DIM * 4;
}

int thmr_mode_bytes(const thmr_config* cfg, int32_t vit_gemm_mode, size_t* split_weight_bytes, size_t* split_act_bytes, size_t* workspace_bytes) {
    if (int r = validate_cfg(cfg)) return r;
    if (vit_gemm_mode != 0 && vit_gemm_mode != 1) return fail(nullptr, THMR_ERR_INVALID, "vit gemm mode must be 0 or 1");
    const bool on = vit_gemm_mode == 1 && cfg->max_batch >= kSplit3LowMinB;
    if (split_weight_bytes) *split_weight_bytes = on ? split_w_bytes_of(cfg->vit_depth, cfg->dec_depth) : 0;
    if (split_act_bytes) *split_act_bytes = on ? split_act_bytes_of(cfg->max_batch) : 0;
    if (workspace_bytes) *workspace_bytes = on && !(cfg->flags & THMR_CFG_NO_PERSISTENT) ? gemm_split3_persist_ws_bytes() : 0;
    return 0;
}

int thmr_arena_bytes(const thmr_config* cfg, size_t* weight_bytes, size_t* scratch_bytes) {
    if (int r = validate_cfg(cfg)) return r;
    thmr_engine tmp;
    tmp.vit_depth = cfg->vit_depth; tmp.dec_depth = cfg->dec_depth; tmp.max_batch = cfg->max_batch;
    tmp.hmr2 = (cfg->flags & THMR_CFG_HEAD_HMR2) != 0;
    layout_weights(&tmp);
    layout_scratch(&tmp);
    if (weight_bytes) *weight_bytes = tmp.wfloats * sizeof(float);
    if (scratch_bytes) *scratch_bytes = tmp.sfloats * sizeof(float);
    return 0;
}

int thmr_spec(const thmr_config* cfg, int32_t index, const char** name, int64_t* numel) {
    if (int r = validate_cfg(cfg)) return r;
    static thread_local std::vector<std::pair<std::string, int64_t>> spec;
    spec.clear();
    build_spec(cfg->vit_depth, cfg->dec_depth, (cfg->flags & THMR_CFG_HEAD_HMR2) != 0, spec);
    if (index >= 0 && index < (int32_t)spec.size()) {
        if (name) *name = spec[index].first.c_str();
        if (numel) *numel = spec[index].second;
    }
    return (int)spec.size();
}

int thmr_create(const thmr_config* cfg, void* weight_arena_dev, void* scratch_arena_dev, thmr_engine** out) {
    if (!out) return fail(nullptr, THMR_ERR_INVALID, "null out");
    *out = nullptr;
    if (int r = validate_cfg(cfg)) return r;
    thmr_engine* e = new thmr_engine();
    e->cfg = *cfg;
    e->vit_depth = cfg->vit_depth; e->dec_depth = cfg->dec_depth; e->max_batch = cfg->max_batch;
    e->hmr2 = (cfg->flags & THMR_CFG_HEAD_HMR2) != 0;
    layout_weights(e);
    layout_scratch(e);
    auto bail = [&](int code, const std::string& m) { fail(nullptr, code, m); thmr_destroy(e); return code; };
    if (hipSetDevice(cfg->device) != hipSuccess) return bail(THMR_ERR_HIP, "hipSetDevice failed");
    if (weight_arena_dev) e->warena = static_cast<float*>(weight_arena_dev);
    else {
        if (hipMalloc(&e->warena, e->wfloats * sizeof(float)) != hipSuccess) return bail(THMR_ERR_NOMEM, "hipMalloc(weights) failed");
        e->own_w = true;
    }
    if (scratch_arena_dev) e->sarena = static_cast<float*>(scratch_arena_dev);
    else {
        if (hipMalloc(&e->sarena, e->sfloats * sizeof(float)) != hipSuccess) return bail(THMR_ERR_NOMEM, "hipMalloc(scratch) failed");
        e->own_s = true;
    }
    // grid-barrier words of the persistent decoder kernel (the scratch arena is private to this engine; a caller-provided
    // one may hold garbage)
    if (hipMemset(e->sarena + e->so.sync, 0, 512 * sizeof(float)) != hipSuccess) return bail(THMR_ERR_HIP, "hipMemset(sync words) failed");
    // arrival counters of the fused skin + joints kernel (self-resetting; zero before the first call)
    if (hipMemset(e->sarena + e->so.lcnt, 0, (size_t)e->max_batch * sizeof(float)) != hipSuccess) return bail(THMR_ERR_HIP, "hipMemset(lbs counters) failed");
    // sticky error word of the persistent decoder kernel, host-mapped so that the next call sees a timeout without a D2H copy
    if (hipHostMalloc(reinterpret_cast<void**>(&e->host_err), 64, hipHostMallocMapped) != hipSuccess) return bail(THMR_ERR_NOMEM, "hipHostMalloc(error word) failed");
    e->host_err[0] = e->host_err[1] = e->host_err[2] = 0;
    e->s3_host_err = e->host_err + 1;
    { const char* lg = thmr_knob("THMR_LEGACY_HEAD"); e->legacy_head = lg && lg[0] == '1'; }
    { const char* mc = thmr_knob("THMR_MIXER_CLUSTER"); e->mixer_cluster = !(mc && mc[0] == '0'); }
    { const char* tg = thmr_knob("THMR_TINY_GEMM"); e->tiny_gemm = !(tg && tg[0] == '0'); }
    e->knobs = read_knobs();
    e->s3_persist = e->knobs.persist;
    if (cfg->flags & THMR_CFG_VIT_GEMM_F32) e->vit_gemm_mode = 0;      // created in the opt-out mode: finalize builds nothing for split3
    if (cfg->flags & THMR_CFG_NO_PERSISTENT) {                         // no kernel that needs all its workgroups resident at once
        e->s3_persist = 0;
        e->legacy_head = true;
        e->no_persistent = true;
    }
    { DecoderTurnstile& t = turnstile(); std::lock_guard<std::mutex> lk(t.mu); t.engines[cfg->device] += 1; e->counted = true; }
    *out = e;
    return 0;
}

void thmr_destroy(thmr_engine* e) {
    if (!e) return;
    if (e->counted) {
        DecoderTurnstile& t = turnstile();
        std::lock_guard<std::mutex> lk(t.mu);
        if (--t.engines[e->cfg.device] <= 0) {              // the device's last engine: its turnstile event goes with it
            auto it = t.last.find(e->cfg.device);
            if (it != t.last.end()) { (void)hipEventDestroy(it->second); t.last.erase(it); }
        }
    }
    for (auto ev : e->ev_pool) (void)hipEventDestroy(ev);
    if (e->host_err) (void)hipHostFree(e->host_err);
    if (e->split_w_counted) {
        SplitShare& sh = split_share();
        std::lock_guard<std::mutex> lk(sh.mu);
        auto it = sh.m.find({e->cfg.device, static_cast<const void*>(e->warena)});
        if (it != sh.m.end() && --it->second.refs <= 0) { (void)hipFree(it->second.p); sh.m.erase(it); }
    } else if (e->split_w) (void)hipFree(e->split_w);
    if (e->split_act) (void)hipFree(e->split_act);
    if (e->s3_ws) (void)hipFree(e->s3_ws);
    if (e->own_w && e->warena) (void)hipFree(e->warena);
    if (e->own_s && e->sarena) (void)hipFree(e->sarena);
    delete e;
}

int thmr_load_weights(thmr_engine* e, const thmr_tensor_desc* t, size_t n, void* stream) {
    if (!e || (!t && n)) return fail(e, THMR_ERR_INVALID, "null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (size_t i = 0; i < n; ++i) {
        if (!t[i].name || !t[i].data) return fail(e, THMR_ERR_INVALID, "tensor desc with null name/data");
        auto it = e->slots.find(t[i].name);
        if (it == e->slots.end()) return fail(e, THMR_ERR_INVALID, std::string("unexpected tensor '") + t[i].name + "' (strict load)");
        if (it->second.numel != t[i].numel)
            return fail(e, THMR_ERR_INVALID, std::string("tensor '") + t[i].name + "': expected " + std::to_string(it->second.numel) +
                                                 " elements, got " + std::to_string(t[i].numel));
        HIP_OK(hipMemcpyAsync(e->warena + it->second.off, t[i].data, sizeof(float) * t[i].numel,
                              t[i].on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        it->second.loaded = true;
    }
    e->finalized = false;
    return write_arena_constants(e, st);
}

int thmr_load_smpl(thmr_engine* e, const thmr_smpl_desc* s, void* stream) {
    if (!e || !s) return fail(e, THMR_ERR_INVALID, "null argument");
    if (!s->v_template || !s->shapedirs || !s->posedirs || !s->J_regressor || !s->lbs_weights || !s->J19_regressor ||
        !s->parents || !s->extra_verts || !s->joint_map)
        return fail(e, THMR_ERR_INVALID, "thmr_smpl_desc has a null field");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_OK(e->smpl.upload(e->warena, s, s->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    e->smpl_loaded = true;
    e->finalized = false;
    return 0;
}

// Every weight pointer a call reads, resolved from the name map ONCE (thmr_finalize_weights): the name map is for the layout and the load,
// and no call path looks a tensor up by name.  Also the scratch pointers, knobs and grid limit of the persistent decoder kernel, which
// travel in the same structures.  An unknown name (impossible for a valid layout) fails here instead of leaving a null pointer behind.
static int resolve_weights(thmr_engine* e) {
    bool known = true;
    auto W = [&](const std::string& name) { float* p = e->W(name); known = known && p != nullptr; return p; };
    e->hot = thmr_engine::HotW{};
    e->vitw.resize(e->vit_depth);
    for (int i = 0; i < e->vit_depth; ++i) {
        const std::string p = "backbone.blocks." + std::to_string(i) + ".";
        VitBlockW& w = e->vitw[i];
        w.n1w = W(p + "norm1.weight"); w.n1b = W(p + "norm1.bias");
        w.qkvw = W(p + "attn.qkv.weight"); w.qkvb = W(p + "attn.qkv.bias");
        w.pw = W(p + "attn.proj.weight"); w.pb = W(p + "attn.proj.bias");
        w.n2w = W(p + "norm2.weight"); w.n2b = W(p + "norm2.bias");
        w.f1w = W(p + "mlp.fc1.weight"); w.f1b = W(p + "mlp.fc1.bias");
        w.f2w = W(p + "mlp.fc2.weight"); w.f2b = W(p + "mlp.fc2.bias");
    }
    // decoder / read-out / mixer_trans: the persistent decoder kernel's parameters, and what the launch-chain head reads
    DecParams& d = e->dec;
    const std::string T = "smpl_head.transformer.";
    for (int l = 0; l < e->dec_depth; ++l) {
        const std::string p = T + "transformer.layers." + std::to_string(l) + ".";
        DecLayerW& w = d.L[l];
        w.n0w = W(p + "0.norm.weight"); w.n0b = W(p + "0.norm.bias");
        const float* qkv = W(p + "0.fn.to_qkv.weight");
        w.wv = qkv ? qkv + (size_t)2 * INNER * E : nullptr;                     // v slice of to_qkv (rows 1024..1535)
        w.wo1 = W(p + "0.fn.to_out.0.weight"); w.bo1 = W(p + "0.fn.to_out.0.bias");
        w.n1w = W(p + "1.norm.weight"); w.n1b = W(p + "1.norm.bias");
        w.wq = W(p + "1.fn.to_q.weight");
        w.wo2 = W(p + "1.fn.to_out.0.weight"); w.bo2 = W(p + "1.fn.to_out.0.bias");
        w.n2w = W(p + "2.norm.weight"); w.n2b = W(p + "2.norm.bias");
        w.w1 = W(p + "2.fn.net.0.weight"); w.b1 = W(p + "2.fn.net.0.bias");
        w.w2 = W(p + "2.fn.net.3.weight"); w.b2 = W(p + "2.fn.net.3.bias");
    }
    d.tok_bias = W(T + "to_token_embedding.bias"); d.pos = W(T + "pos_embedding");
    d.kv = e->S(e->so.big); d.ldkv = (int64_t)e->dec_depth * 2 * INNER;
    d.ro_w = e->warena + e->o_ro_w; d.ro_b = e->warena + e->o_ro_b;
    d.dx = e->S(e->so.dx); d.dv = e->S(e->so.dv); d.dq = e->S(e->so.dq); d.dca = e->S(e->so.dca); d.dff = e->S(e->so.dff);
    d.ro = e->S(e->so.ro); d.mt = e->S(e->so.mt);
    d.sync = reinterpret_cast<unsigned*>(e->S(e->so.sync));
    d.depth = e->dec_depth; d.B = 0;
    { const char* tl = thmr_knob("THMR_DEC_TIMELINE"); d.timeline = tl && tl[0] == '1'; }
    { const char* ft = thmr_knob("THMR_DEC_FORCE_TIMEOUT"); d.debug_fail = ft && ft[0] == '1'; }
    // all-to-all barrier: measured SLOWER (head 0.711 vs 0.664 ms at one crop, 2.87-2.90 vs 2.81-2.82 at 64: 128-256 workgroups x
    // 128-256 device-scope polls contend; profiles/r3k_decoder_barrier_all_to_all_ab.log) — kept behind the knob only
    { const char* bm = thmr_knob("THMR_DEC_BARRIER"); d.barrier_a2a = bm && bm[0] == '1'; }
    {
        // never more workgroups than can be resident at once (occupancy query x CUs): the grid barrier depends on it
        const int nb = decoder_max_coresident_blocks(e->cfg.device, e->hmr2 ? THMR_HEAD_HMR2 : THMR_HEAD_TOKEN);
        if (nb < 1) return fail(e, THMR_ERR_HIP, "persistent decoder kernel cannot be resident on this device (occupancy query failed)");
        d.max_blocks = nb;
        d.host_err = e->host_err;
    }
    auto& h = e->hot;
    h.pe_w = W("backbone.patch_embed.proj.weight"); h.pe_b = W("backbone.patch_embed.proj.bias");
    h.pos = W("backbone.pos_embed");
    h.lastn_w = W("backbone.last_norm.weight"); h.lastn_b = W("backbone.last_norm.bias");
    h.init_pose = W("smpl_head.init_body_pose"); h.init_betas = W("smpl_head.init_betas"); h.init_cam = W("smpl_head.init_cam");
    if (!e->hmr2) {      // the token head: mixer stack, classifier, VQ decoder, codebook
        const std::string C = "smpl_head.decpose.";
        d.mt_w = W(C + "mixer_trans.ff.0.weight"); d.mt_b = W(C + "mixer_trans.ff.0.bias");
        MixerParams& m = e->mix;
        for (int i = 0; i < MIX; ++i) {
            const std::string p = C + "mixer_head." + std::to_string(i) + ".";
            MixerLayerW& w = m.L[i];
            w.ln1w = W(p + "layernorm1.weight"); w.ln1b = W(p + "layernorm1.bias");
            w.wt1 = W(p + "MLP_token.ff.0.weight"); w.bt1 = W(p + "MLP_token.ff.0.bias");
            w.wt2 = W(p + "MLP_token.ff.3.weight"); w.bt2 = W(p + "MLP_token.ff.3.bias");
            w.ln2w = W(p + "layernorm2.weight"); w.ln2b = W(p + "layernorm2.bias");
            w.wc1 = W(p + "MLP_channel.ff.0.weight"); w.bc1 = W(p + "MLP_channel.ff.0.bias");
            w.wc2 = W(p + "MLP_channel.ff.3.weight"); w.bc2 = W(p + "MLP_channel.ff.3.bias");
        }
        m.tln_w = W(C + "mixer_trans.ff.1.weight"); m.tln_b = W(C + "mixer_trans.ff.1.bias");
        m.wn = W(C + "mixer_norm_layer.ff.0.weight"); m.bn = W(C + "mixer_norm_layer.ff.0.bias");
        m.nln_w = W(C + "mixer_norm_layer.ff.1.weight"); m.nln_b = W(C + "mixer_norm_layer.ff.1.bias");
        m.mt = e->S(e->so.mt); m.out = e->S(e->so.nl2);
        h.cls_w = W(C + "class_pred_layer.weight"); h.cls_b = W(C + "class_pred_layer.bias");
        for (int i = 0; i < 9; ++i) h.conv_b[i] = W(std::string(kConv3[i]) + ".bias");
        for (int b = 0; b < 2; ++b) {
            const std::string p = "decoder.decoder.14.0.model." + std::to_string(b) + ".";
            h.res_w[b] = W(p + "conv2.weight"); h.res_b[b] = W(p + "conv2.bias");
        }
        h.codebook = W("quantizer.codebook");
    }
    // the optional tokenizer encoder: a k > 1 conv reads its repacked copy (thmr_finalize_weights), a 1 x 1 conv the checkpoint tensor
    for (int i = 0; i < (e->enc_ready ? kEncN : 0); ++i) {
        const std::string n = kEnc[i].name;
        h.enc_w[i] = kEnc[i].ks > 1 ? e->warena + e->enc_convp[i] : W(n + ".weight");
        h.enc_b[i] = W(n + ".bias");
    }
    return known ? 0 : fail(e, THMR_ERR_STATE, e->err);      // e->err: "internal: unknown weight <name>" (thmr_engine::W)
}

// split3 copies of the four ViT GEMM weights of every block (6 bytes per weight) + the activation operand buffers, engine-owned
static int build_split_weights(thmr_engine* e, hipStream_t st) {
    if (e->max_batch < kSplit3LowMinB) return 0;      // no call of this engine can reach the mode (one and two crops run the exact-fp32 kernels)
    const size_t kv_rows = (size_t)e->dec_depth * 2 * INNER;                                           // the decoder's to_kv of all layers
    if (!e->split_w) {
        // one copy per (device, weight arena): engines that share an arena share it (split_share())
        SplitShare& sh = split_share();
        std::lock_guard<std::mutex> lk(sh.mu);
        const size_t bytes = split_w_bytes_of(e->vit_depth, e->dec_depth);
        auto key = std::make_pair(e->cfg.device, static_cast<const void*>(e->warena));
        auto it = sh.m.find(key);
        if (it != sh.m.end() && it->second.bytes == bytes) {
            it->second.refs += 1;
            e->split_w = it->second.p;
        } else {
            if (it != sh.m.end())
                return fail(e, THMR_ERR_INVALID, "another engine with a different depth holds split3 copies of this weight arena");
            char* p = nullptr;
            if (hipMalloc(reinterpret_cast<void**>(&p), bytes) != hipSuccess)
                return fail(e, THMR_ERR_NOMEM, "hipMalloc(split3 ViT weights) failed");
            sh.m[key] = SplitShare::Ent{p, bytes, 1};
            e->split_w = p;
        }
        e->split_w_counted = true;
    }
    // activations: [M][1280] + [M][5120] split3 operands, then the two fp32 partial-sum planes of fc2's split-K ([2][M][1280])
    if (!e->split_act && hipMalloc(reinterpret_cast<void**>(&e->split_act), split_act_bytes_of(e->max_batch)) != hipSuccess)
        return fail(e, THMR_ERR_NOMEM, "hipMalloc(split3 activations) failed");
    if (!e->s3_ws && !e->no_persistent) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, e->cfg.device) == hipSuccess && prop.multiProcessorCount == 256) {
            // the persistent kernel's decomposition is 8 XCDs x 32 CUs; elsewhere the per-tile kernel stays in charge (same results)
            if (hipMalloc(&e->s3_ws, gemm_split3_persist_ws_bytes()) != hipSuccess) return fail(e, THMR_ERR_NOMEM, "hipMalloc(split3 hand-over workspace) failed");
            if (int r = reset_s3_workspace(e, st)) return r;
        }
    }
    e->vitw_s.resize(e->vit_depth);
    char* p = e->split_w;
    for (int i = 0; i < e->vit_depth; ++i) {
        const VitBlockW& w = e->vitw[i];
        auto conv = [&](const float* src, int rows, int K, const char*& out) -> int {
            out = p;
            const int rc = launch_split3(src, K, p, K, rows, K, st);
            p += (size_t)rows * K * 6;
            return rc;
        };
        LAUNCH_OK(conv(w.qkvw, 3 * DIM, DIM, e->vitw_s[i].qkv));
        LAUNCH_OK(conv(w.pw, DIM, DIM, e->vitw_s[i].proj));
        LAUNCH_OK(conv(w.f1w, MLP, DIM, e->vitw_s[i].fc1));
        LAUNCH_OK(conv(w.f2w, DIM, MLP, e->vitw_s[i].fc2));
    }
    e->kv_s = p;
    LAUNCH_OK(launch_split3(e->warena + e->o_kv_all, DIM, p, DIM, (int64_t)kv_rows, DIM, st));
    p += kv_rows * DIM * 6;
    e->pe_s = p;
    LAUNCH_OK(launch_split3(e->hot.pe_w, 768, p, 768, DIM, 768, st));
    return 0;
}

int thmr_finalize_weights(thmr_engine* e, int32_t assume_all_loaded, void* stream) {
    if (!e) return fail(e, THMR_ERR_INVALID, "null engine");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!assume_all_loaded) {
        for (auto& n : e->required)
            if (!e->slots[n].loaded) return fail(e, THMR_ERR_STATE, "missing tensor '" + n + "' (strict load)");
        if (!e->smpl_loaded) return fail(e, THMR_ERR_STATE, "SMPL constants not loaded (thmr_load_smpl)");
    }
    int32_t* flags = reinterpret_cast<int32_t*>(e->warena + e->o_flags);
    if (!assume_all_loaded) {
        if (int r = write_arena_constants(e, st)) return r;      // idempotent (load time wrote them already)
        size_t enc_loaded = 0;
        for (auto& n : e->enc_names) enc_loaded += e->slots[n].loaded ? 1 : 0;
        if (enc_loaded != 0 && enc_loaded != e->enc_names.size())
            return fail(e, THMR_ERR_STATE, "tokenizer encoder partially loaded: " + std::to_string(enc_loaded) + " of " +
                                               std::to_string(e->enc_names.size()) + " tensors");
        e->enc_ready = !e->hmr2 && enc_loaded == e->enc_names.size();
    } else {
        // the arena was filled by someone else (a broadcast from the loading rank, or it is another engine's live arena): it must
        // carry the loader's magic word, otherwise the index tables / padding row / flags are uninitialised memory
        int32_t f[2] = {0, 0};
        HIP_OK(hipMemcpyAsync(f, flags, sizeof(f), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (f[1] != (e->hmr2 ? kArenaMagicHmr2 : kArenaMagic))
            return fail(e, THMR_ERR_STATE, "thmr_finalize_weights(assume_all_loaded=1): the weight arena does not carry a loaded model "
                                           "(no loader magic word of this head kind): was it broadcast before the root called thmr_load_weights, or never received?");
        e->enc_ready = !e->hmr2 && f[0] == kEncMagic;
    }
    if (!e->hmr2) {
        for (int i = 0; i < 9; ++i)
            LAUNCH_OK(launch_conv_repack(e->W(std::string(kConv3[i]) + ".weight"), e->warena + e->convp[i], kConv3Co[i], kConv3Ci[i], 3, st));
        LAUNCH_OK(launch_transpose(e->W("quantizer.codebook"), e->warena + e->o_cbT, 1, NCLS, CODE, st));
        LAUNCH_OK(launch_code_norm(e->W("quantizer.codebook"), e->warena + e->o_cnorm, NCLS, st));
    }
    LAUNCH_OK(e->smpl.derive(e->warena, st));
    if (e->enc_ready)
        for (int i = 0; i < kEncN; ++i)
            if (kEnc[i].ks > 1)
                LAUNCH_OK(launch_conv_repack_pad(e->W(std::string(kEnc[i].name) + ".weight"), e->warena + e->enc_convp[i],
                                                 kEnc[i].co, kEnc[i].ci, kEnc[i].cp, kEnc[i].ks, st));
    if (int r = resolve_weights(e)) return r;
    if (e->vit_gemm_mode == 1) {                                       // weights were (re)loaded with the split3 mode on
        if (int r = build_split_weights(e, st)) return r;              // (on failure the engine stays un-finalized: no forward can run on half-built operands)
        HIP_OK(hipStreamSynchronize(st));                              // as in thmr_set_vit_gemm: visible to forwards on any stream
    }
    e->finalized = true;
    return 0;
}

int thmr_set_vit_gemm(thmr_engine* e, int32_t mode, void* stream) {
    if (!e) return fail(e, THMR_ERR_INVALID, "null engine");
    if (mode != 0 && mode != 1) return fail(e, THMR_ERR_INVALID, "vit gemm mode must be 0 (exact-fp32 MFMA) or 1 (split3 on the bf16 matrix pipe)");
    if (mode == 1) {
        if (!e->finalized) return fail(e, THMR_ERR_STATE, "thmr_set_vit_gemm(1) needs finalized weights (thmr_finalize_weights)");
        if (hipSetDevice(e->cfg.device) != hipSuccess) return fail(e, THMR_ERR_HIP, "hipSetDevice failed");
        if (int r = build_split_weights(e, static_cast<hipStream_t>(stream))) return r;
        // the conversion (3.8 GB of writes) was enqueued on the caller's stream; a forward on ANOTHER stream right after this call must
        // not read half-converted weights: a one-time switch, so simply wait for it
        HIP_OK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    }
    e->vit_gemm_mode = mode;
    return 0;
}

int thmr_get_vit_gemm(thmr_engine* e) { return e ? e->vit_gemm_mode : -1; }

// an engine created with THMR_CFG_HEAD_HMR2 has no tokenizer: its entry points and the token outputs are refused by name
static int refuse_hmr2(thmr_engine* e, const char* what) {
    return fail(e, THMR_ERR_INVALID, std::string(what) + " does not exist on an engine created with THMR_CFG_HEAD_HMR2 (the HMR2 head has no pose tokens and no tokenizer)");
}
static int refuse_hmr2_outputs(thmr_engine* e, const thmr_outputs* out) {
    if (!e->hmr2 || !out) return 0;
    if (out->cls_logits_softmax) return refuse_hmr2(e, "thmr_outputs.cls_logits_softmax");
    if (out->cls_logits) return refuse_hmr2(e, "thmr_outputs.cls_logits");
    if (out->token_idx) return refuse_hmr2(e, "thmr_outputs.token_idx");
    return 0;
}

int thmr_vq_decode(thmr_engine* e, const float* probs_dev, int32_t B, float* pose6d_dev, void* stream) {
    if (int r = check_ready(e, B)) return r;
    if (e->hmr2) return refuse_hmr2(e, "thmr_vq_decode");
    if (!probs_dev || !pose6d_dev) return fail(e, THMR_ERR_INVALID, "null buffer");
    return vq_decode(e, probs_dev, B, pose6d_dev, static_cast<hipStream_t>(stream));
}

// EncodeTokens.forward (tokenization/models/vanilla_pose_vqvae.py:334-342): PoseSPEncoderV1 (:66-111) -> preprocess
// (quantize_cnn.py:74-78) -> QuantizeEMAReset.quantize (:80-86).  pose (B,21,6) rot6d body pose -> idx (B,160).
// Scratch of the encode path, all out of the big time-shared buffer (B*192*6144 floats; the encode path never overlaps a forward on one
// engine): [gather / distance operand B*320*1536 | a0, a1, a2: B*320*512 each | the round trip's statistics: 2048 counts, partial sums].
// None of it is touched by the VQ decoder (gat / gat2 / act0-2 are buffers of their own), so a latent left in a2 survives until the
// round trip's lookup has read it.
static float* enc_scratch_a2(thmr_engine* e, int B) { return e->S(e->so.big) + (size_t)B * 320 * 1536 + 2 * (size_t)B * 320 * VQW; }

// *lat_out: where the latent (B*160, 256) was written — latent_dev, or the scratch region a2
static int encode_tokens_call(thmr_engine* e, const float* pose_dev, int B, int32_t* idx_dev, float* latent_dev, const float** lat_out,
                              hipStream_t st) {
    float* gat = e->S(e->so.big);
    float* a0 = gat + (size_t)B * 320 * 1536;
    float* a1 = a0 + (size_t)B * 320 * VQW;
    float* a2 = a1 + (size_t)B * 320 * VQW;
    const int32_t* tab = reinterpret_cast<const int32_t*>(e->warena + e->o_idx_enc);
    auto W = [&](int i) { return e->hot.enc_w[i]; };      // the repacked weights where ks > 1
    auto Bv = [&](int i) { return e->hot.enc_b[i]; };
    // 0: Conv1d(6->512,k3,p1)+ReLU at T=21 (channels zero-padded 6->32 so that K = 96)
    LAUNCH_OK(launch_conv_gather_general(pose_dev, gat, nullptr, B, 21, 21, 21, 6, 32, 3, 1, 1, st));
    {
        GemmArgs a = mk(gat, 96, W(0), 96, Bv(0), nullptr, 0, a0, VQW, B * 21, VQW, 96);
        LAUNCH_OK(launch_gemm(a, EPI_BIAS_RELU, -1, st));
    }
    // 1-4: nearest resample (21->40, then x2 three times) + Conv1d(512,k3,p1) + ReLU
    const int tin[4] = {21, 40, 80, 160}, tout[4] = {40, 80, 160, 320}, toff[4] = {0, 40, 120, 280};
    float* cur = a0;
    float* nxt = a1;
    for (int i = 0; i < 4; ++i) {
        LAUNCH_OK(launch_conv3_gather(cur, gat, tab + toff[i], B, tin[i], tout[i], VQW, 1, 0, st));
        GemmArgs a = mk(gat, 3 * VQW, W(1 + i), 3 * VQW, Bv(1 + i), nullptr, 0, nxt, VQW, B * tout[i], VQW, 3 * VQW);
        LAUNCH_OK(launch_gemm(a, EPI_BIAS_RELU, -1, st));
        std::swap(cur, nxt);
    }
    // 5: Conv1d(512,512,k4,s2,p1): 320 -> 160, no activation
    LAUNCH_OK(launch_conv_gather_general(cur, gat, nullptr, B, 320, 320, 160, VQW, VQW, 4, 2, 1, st));
    {
        GemmArgs a = mk(gat, 4 * VQW, W(5), 4 * VQW, Bv(5), nullptr, 0, nxt, VQW, B * 160, VQW, 4 * VQW);
        LAUNCH_OK(launch_gemm(a, EPI_BIAS, -1, st));
        std::swap(cur, nxt);
    }
    // 6-9: Resnet1D (dilation 3 then 1): x + conv2(relu(conv1(relu(x))))   (resnet.py:49-69)
    for (int blk = 0; blk < 2; ++blk) {
        const int c1 = 6 + 2 * blk, c2 = 7 + 2 * blk, dil = blk == 0 ? 3 : 1;
        LAUNCH_OK(launch_conv3_gather(cur, gat, nullptr, B, 160, 160, VQW, dil, 1, st));
        GemmArgs g1 = mk(gat, 3 * VQW, W(c1), 3 * VQW, Bv(c1), nullptr, 0, a2, VQW, B * 160, VQW, 3 * VQW);
        LAUNCH_OK(launch_gemm(g1, EPI_BIAS_RELU, -1, st));
        GemmArgs g2 = mk(a2, VQW, W(c2), VQW, Bv(c2), cur, VQW, nxt, VQW, B * 160, VQW, VQW);
        LAUNCH_OK(launch_gemm(g2, EPI_BIAS_RESID, -1, st));
        std::swap(cur, nxt);
    }
    // 10: Conv1d(512->256,k3,p1): the latent, already in the (N*T, C) layout QuantizeEMAReset.preprocess produces
    float* lat = latent_dev ? latent_dev : a2;
    LAUNCH_OK(launch_conv3_gather(cur, gat, nullptr, B, 160, 160, VQW, 1, 0, st));
    {
        GemmArgs a = mk(gat, 3 * VQW, W(10), 3 * VQW, Bv(10), nullptr, 0, lat, CODE, B * 160, CODE, 3 * VQW);
        LAUNCH_OK(launch_gemm(a, EPI_BIAS, -1, st));
    }
    // argmin-L2 against the codebook; the x.C^T scores go to the gather region (B*160*2048 <= B*320*1536)
    GemmArgs d = mk(lat, CODE, e->hot.codebook, CODE, nullptr, nullptr, 0, gat, NCLS, B * 160, NCLS, CODE);
    LAUNCH_OK(launch_gemm(d, EPI_NONE, -1, st));
    LAUNCH_OK(launch_vq_argmin_rows(lat, gat, e->warena + e->o_cnorm, idx_dev, nullptr, B * 160, st));
    if (lat_out) *lat_out = lat;
    return 0;
}

int thmr_encode_tokens(thmr_engine* e, const float* pose_dev, int32_t B, int32_t* idx_dev, float* latent_dev, void* stream) {
    if (int r = check_ready(e, B)) return r;
    if (e->hmr2) return refuse_hmr2(e, "thmr_encode_tokens");
    if (!e->enc_ready) return fail(e, THMR_ERR_STATE, "tokenizer encoder weights ('encoder.encoder.*') were not loaded");
    if (!pose_dev || !idx_dev) return fail(e, THMR_ERR_INVALID, "null buffer");
    return encode_tokens_call(e, pose_dev, B, idx_dev, latent_dev, nullptr, static_cast<hipStream_t>(stream));
}

// A code index outside [0, 2048) reached a lookup / statistics kernel of this engine (clamped there, never read through): the kernels set
// the host-mapped flag word [2], and the next status read or tokenizer call reports it ONCE.  The work that carried it is invalid.
static int report_bad_code_index(thmr_engine* e) {
    if (!e->host_err || *static_cast<volatile unsigned*>(e->host_err + 2) == 0) return 0;
    e->host_err[2] = 0;
    return fail(e, THMR_ERR_INVALID, "a code index outside [0, 2048) was passed to thmr_vq_decode_idx / thmr_tokenizer_roundtrip in an earlier "
                                     "call (clamped on the device, nothing was read out of bounds); that call's outputs are invalid");
}

int thmr_vq_decode_idx(thmr_engine* e, const int32_t* idx_dev, int32_t B, float* pose6d_dev, void* stream) {
    if (int r = check_ready(e, B)) return r;
    if (e->hmr2) return refuse_hmr2(e, "thmr_vq_decode_idx");
    if (int r = report_bad_code_index(e)) return r;
    if (!idx_dev || !pose6d_dev) return fail(e, THMR_ERR_INVALID, "null buffer");
    return vq_decode_idx(e, idx_dev, nullptr, B, pose6d_dev, static_cast<hipStream_t>(stream));
}

// VanillaTokenizer.forward (vanilla_pose_vqvae.py:244-255): encoder -> QuantizeEMAReset.forward (quantize_cnn.py:95-130: quantize,
// perplexity, commit loss, straight-through) -> decoder -> rotation_6d_to_matrix (-> matrix_to_axis_angle), on one stream, no allocation,
// no host synchronisation.
int thmr_tokenizer_roundtrip(thmr_engine* e, const float* pose6d_dev, int32_t B, const thmr_tokenizer_out* out, void* stream) {
    if (int r = check_ready(e, B, static_cast<hipStream_t>(stream))) return r;
    if (e->hmr2) return refuse_hmr2(e, "thmr_tokenizer_roundtrip");
    if (!e->enc_ready) return fail(e, THMR_ERR_STATE, "tokenizer encoder weights ('encoder.encoder.*') were not loaded");
    if (int r = report_bad_code_index(e)) return r;
    if (!pose6d_dev || !out) return fail(e, THMR_ERR_INVALID, "null buffer");
    if (out->accumulate_counts && !out->code_count) return fail(e, THMR_ERR_INVALID, "accumulate_counts needs a code_count buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t* idx = out->idx ? out->idx : reinterpret_cast<int32_t*>(e->S(e->so.tokidx));
    const float* lat = nullptr;
    if (int r = encode_tokens_call(e, pose6d_dev, B, idx, out->latent, &lat, st)) return r;
    unsigned* flag = e->host_err ? e->host_err + 2 : nullptr;
    const float* cb = e->hot.codebook;
    if (out->commit_loss || out->perplexity || out->code_count) {
        float* sc = enc_scratch_a2(e, B) + (size_t)B * 320 * VQW;      // behind a2: 2048 counts, then the partial sums
        int32_t* cnt = out->code_count ? out->code_count : reinterpret_cast<int32_t*>(sc);
        LAUNCH_OK(launch_vq_stats(lat, cb, idx, B * TN, cnt, out->code_count && out->accumulate_counts, sc + NCLS, out->commit_loss,
                                  out->perplexity, flag, st));
    }
    float* pose = out->pose6d ? out->pose6d : e->S(e->so.bpose);
    if (int r = vq_decode_idx(e, idx, lat, B, pose, st)) return r;
    if (out->rotmat || out->aa) {
        float* rot = out->rotmat ? out->rotmat : e->S(e->so.rot);      // (B,24,9) scratch holds the 21 body joints
        LAUNCH_OK(launch_rot6d(pose, rot, B * VQJ, st));
        if (out->aa) LAUNCH_OK(launch_rotmat_to_aa(rot, out->aa, B * VQJ, st));
    }
    return 0;
}

int thmr_weight_arena(thmr_engine* e, void** ptr_dev, size_t* bytes) {
    if (!e) return fail(e, THMR_ERR_INVALID, "null engine");
    if (ptr_dev) *ptr_dev = e->warena;
    if (bytes) *bytes = e->wfloats * sizeof(float);
    return 0;
}

int thmr_engine_status(thmr_engine* e, void* stream) {
    if (!e) return fail(e, THMR_ERR_INVALID, "null engine");
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned words[4] = {0, 0, 0, 0};
    HIP_OK(hipMemcpyAsync(words, e->sarena + e->so.sync, sizeof(words), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (words[3] != 0 || (e->host_err && *static_cast<volatile unsigned*>(e->host_err) != 0)) return recover_decoder_timeout(e);
    if (int r = report_bad_code_index(e)) return r;
    if (e->s3_ws) {
        // persistent split3 GEMM: a consumer's bounded wait for a hand-over slab ran out (see recover_split3_timeout; the next forward-type
        // call reports it too, through the host-mapped copy of this word).  Reported once.
        unsigned err = 0;
        if (gemm_split3_persist_error(e->s3_ws, st, &err) != 0) return fail(e, THMR_ERR_HIP, "reading the split3 hand-over error word failed");
        if (e->s3_host_err && *static_cast<volatile unsigned*>(e->s3_host_err) != 0) err = 1;
#ifdef THMR_EXPERIMENTS
        // tests only: report a hand-over timeout that did not happen, once per engine, to exercise the recovery
        if (e->s3_persist && e->vit_gemm_mode == 1 && !e->s3_forced_once) {
            const char* f = thmr_knob("THMR_SPLIT3_FORCE_TIMEOUT");
            if (f && f[0] == '1') { err = 1; e->s3_forced_once = true; }
        }
#endif
        if (err != 0) return recover_split3_timeout(e);
    }
    return 0;
}

int thmr_debug_decoder_timeline(thmr_engine* e, uint64_t* stamps_host, int32_t max_stamps, void* stream) {
    if (!e || !stamps_host || max_stamps < 1 || max_stamps > 240) return fail(e, THMR_ERR_INVALID, "bad argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_OK(hipMemcpyAsync(stamps_host, e->sarena + e->so.sync + 16, sizeof(uint64_t) * max_stamps, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}

int thmr_debug_vit_plan(const thmr_config* cfg, int32_t vit_gemm_mode, int32_t B, int32_t streams_available, thmr_vit_plan_desc* out) {
    if (int r = validate_cfg(cfg)) return r;
    if (vit_gemm_mode != 0 && vit_gemm_mode != 1) return fail(nullptr, THMR_ERR_INVALID, "vit gemm mode must be 0 or 1");
    if (!out || B < 1 || B > cfg->max_batch) return fail(nullptr, THMR_ERR_INVALID, "null out / batch outside [1, max_batch]");
    thmr_engine tmp;
    tmp.max_batch = cfg->max_batch;
    layout_scratch(&tmp);
    VitPlanIn in{};
    in.mode = vit_gemm_mode; in.B = B; in.dec_depth = cfg->dec_depth;
    in.split_ready = vit_gemm_mode == 1 && cfg->max_batch >= kSplit3LowMinB;      // what thmr_finalize_weights builds (build_split_weights)
    in.streams = streams_available != 0 && !(cfg->flags & THMR_CFG_NO_PERSISTENT);
    in.part_floats = tmp.so.part_floats;
    *out = plan_vit(read_knobs(), in);
    return 0;
}

// a forward-type call = one turn of the per-device turnstile (struct Turn): r = the call's own result, then the turn's end
static int end_turn(thmr_engine* e, Turn& turn, int r) {
    const int t = turn.end();
    if (r) return r;
    return t ? fail(e, THMR_ERR_HIP, "hipEventRecord failed at the end of the call (per-device engine turnstile)") : 0;
}
#define THMR_TURN(turn, e, st)                                                                                         \
    Turn turn(e, st);                                                                                                  \
    if (turn.rc) return fail(e, THMR_ERR_HIP, "the per-device engine turnstile could not create / wait for its event")

int thmr_vit_forward(thmr_engine* e, const float* img_dev, int32_t B, float* feats_dev, void* stream) {
    if (int r = check_ready(e, B, static_cast<hipStream_t>(stream))) return r;
    if (!img_dev || !feats_dev) return fail(e, THMR_ERR_INVALID, "null buffer");
    THMR_TURN(turn, e, static_cast<hipStream_t>(stream));
    return end_turn(e, turn, vit_forward(e, img_dev, B, feats_dev, static_cast<hipStream_t>(stream)));
}

static int head_forward_call(thmr_engine* e, const float* ctx_dev, int32_t B, const thmr_outputs* out, hipStream_t st) {
    if (int r = head_forward(e, ctx_dev, B, out, st)) return r;
    if (out && (out->pred_vertices || out->pred_keypoints_3d || out->pred_keypoints_2d)) {
        const float* rot = out->rotmat ? out->rotmat : e->S(e->so.rot);
        const float* betas = out->betas ? out->betas : e->S(e->so.betas);
        const float* camt = out->pred_cam_t ? out->pred_cam_t : e->S(e->so.camt);
        return lbs(e, rot, betas, camt, B, out->pred_vertices, out->pred_keypoints_3d, out->pred_keypoints_2d, st);
    }
    return 0;
}

int thmr_head_forward(thmr_engine* e, const float* ctx_dev, int32_t B, const thmr_outputs* out, void* stream) {
    if (int r = check_ready(e, B, static_cast<hipStream_t>(stream))) return r;
    if (!ctx_dev) return fail(e, THMR_ERR_INVALID, "null buffer");
    if (int r = refuse_hmr2_outputs(e, out)) return r;
    hipStream_t st = static_cast<hipStream_t>(stream);
    THMR_TURN(turn, e, st);
    return end_turn(e, turn, head_forward_call(e, ctx_dev, B, out, st));
}

static int forward_call(thmr_engine* e, const float* img_dev, int32_t B, const thmr_outputs* out, hipStream_t st) {
    float* ctx = e->S(e->so.h);
    if (int r = vit_forward(e, img_dev, B, nullptr, st)) return r;
    if (out->vit_features)
        HIP_OK(hipMemcpyAsync(out->vit_features, ctx, sizeof(float) * (size_t)B * TOK * DIM, hipMemcpyDeviceToDevice, st));
    if (int r = head_forward(e, ctx, B, out, st)) return r;
    const float* rot = out->rotmat ? out->rotmat : e->S(e->so.rot);
    const float* betas = out->betas ? out->betas : e->S(e->so.betas);
    const float* camt = out->pred_cam_t ? out->pred_cam_t : e->S(e->so.camt);
#ifdef THMR_EXPERIMENTS
    // tests only (THMR_SPLIT3_FORCE_TIMEOUT=2): write what a timed-out hand-over consumer writes into the host-mapped error word, once per
    // engine, so that the NEXT forward-type call goes through check_ready's report-reset-fall-back path
    if (e->s3_ws && e->s3_persist && e->vit_gemm_mode == 1 && !e->s3_forced_once && e->s3_host_err) {
        const char* f = thmr_knob("THMR_SPLIT3_FORCE_TIMEOUT");
        if (f && f[0] == '2') { *e->s3_host_err = 1; e->s3_forced_once = true; }
    }
#endif
    return lbs(e, rot, betas, camt, B, out->pred_vertices, out->pred_keypoints_3d, out->pred_keypoints_2d, st);
}

int thmr_forward(thmr_engine* e, const float* img_dev, int32_t B, const thmr_outputs* out, void* stream) {
    if (int r = check_ready(e, B, static_cast<hipStream_t>(stream))) return r;
    if (!img_dev || !out) return fail(e, THMR_ERR_INVALID, "null buffer");
    if (int r = refuse_hmr2_outputs(e, out)) return r;
    hipStream_t st = static_cast<hipStream_t>(stream);
    THMR_TURN(turn, e, st);
    return end_turn(e, turn, forward_call(e, img_dev, B, out, st));
}

int thmr_lbs_forward(thmr_engine* e, const float* rotmat_dev, const float* betas_dev, const float* cam_dev, int32_t B,
                     float* verts_dev, float* joints_dev, float* cam_t_dev, float* kp2d_dev, void* stream) {
    if (int r = check_ready(e, B)) return r;
    if (!rotmat_dev || !betas_dev) return fail(e, THMR_ERR_INVALID, "null buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float* camt = nullptr;
    if (cam_dev) {
        float* ct = cam_t_dev ? cam_t_dev : e->S(e->so.camt);
        LAUNCH_OK(launch_cam_t(cam_dev, ct, FOCAL, IMG, B, st));
        camt = ct;
    }
    return lbs(e, rotmat_dev, betas_dev, camt, B, verts_dev, joints_dev, camt ? kp2d_dev : nullptr, st);
}

int thmr_vq_argmin(thmr_engine* e, const float* x_dev, int32_t rows, int32_t* idx_dev, float* dist_dev, void* stream) {
    if (!e) return fail(e, THMR_ERR_INVALID, "null engine");
    if (!e->finalized) return fail(e, THMR_ERR_STATE, "weights not finalized");
    if (e->hmr2) return refuse_hmr2(e, "thmr_vq_argmin");
    if (!x_dev || !idx_dev || rows < 1) return fail(e, THMR_ERR_INVALID, "bad argument");
    if ((size_t)rows * NCLS > (size_t)e->max_batch * TOK * 6144) return fail(e, THMR_ERR_INVALID, "rows exceed scratch capacity");
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* dot = e->S(e->so.big);
    GemmArgs a = mk(x_dev, CODE, e->hot.codebook, CODE, nullptr, nullptr, 0, dot, NCLS, rows, NCLS, CODE);
    LAUNCH_OK(launch_gemm(a, EPI_NONE, -1, st));
    LAUNCH_OK(launch_vq_argmin_rows(x_dev, dot, e->warena + e->o_cnorm, idx_dev, dist_dev, rows, st));
    return 0;
}

// ---- profiler ----
int thmr_prof_enable(thmr_engine* e, int32_t on) {
    if (!e) return fail(e, THMR_ERR_INVALID, "null engine");
    e->prof_on = on < 0 ? 0 : (on > 3 ? 1 : on);
    return 0;
}

int thmr_prof_collect(thmr_engine* e, thmr_prof_entry* entries, int32_t reset) {
    if (!e || !entries) return fail(e, THMR_ERR_INVALID, "null argument");
    for (int i = 0; i < THMR_PROF_NUM; ++i) entries[i] = thmr_prof_entry{0, 0, 0, 0};
    for (auto& r : e->prof) {
        HIP_OK(hipEventSynchronize(r.e1));
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, r.e0, r.e1));
        entries[r.cls].ms += ms;
        entries[r.cls].flops += r.flops;
        entries[r.cls].bytes += r.bytes;
        entries[r.cls].launches += 1;
    }
    if (reset) { e->prof.clear(); e->ev_next = 0; }
    return 0;
}

}  // extern "C"
