// The engine's weights: the reference checkpoint contract as ONE table, the two arena layouts derived from it, load, finalize (the
// only place that looks a tensor up by name) and the split3 weight copies.  Host code only.
#include <cmath>
#include <map>
#include <mutex>

#include "engine_state.h"

namespace {

// ---- the reference checkpoint contract, mirrored by tokenhmr_amd/weights.py::spec ----
// ONE line per tensor: its name behind the module's prefix, its element count, and the pointer that finalize resolves for it.  Three
// things derive from these tables through walk_contract / walk_convs, and from nothing else: thmr_spec with `required`, the slots
// (layout_weights) and the pointers (resolve_weights).  Table order is thmr_spec order is arena order (tests/golden/arena_layout.json pins
// it).  A new tensor is one line here — and one in weights.py.
enum Place { OWN, KV_GROUP, RO_W, RO_B };      // a slot of its own, or a row block of the stacked to_kv matrix / of the stacked read-out
// where a resolved pointer goes: the member M of the engine's weight struct that owns it (i: the block / layer of a repeated module)
inline VitBlockW& owner(thmr_engine* e, int i, const float* VitBlockW::*) { return e->vitw[i]; }
inline DecLayerW& owner(thmr_engine* e, int i, const float* DecLayerW::*) { return e->dec.L[i]; }
inline MixerLayerW& owner(thmr_engine* e, int i, const float* MixerLayerW::*) { return e->mix.L[i]; }
inline HotW& owner(thmr_engine* e, int, const float* HotW::*) { return e->hot; }
inline DecParams& owner(thmr_engine* e, int, const float* DecParams::*) { return e->dec; }
inline MixerParams& owner(thmr_engine* e, int, const float* MixerParams::*) { return e->mix; }
template <auto M> const float** at(thmr_engine* e, int i) { return &(owner(e, i, M).*M); }
struct Wt {
    const char* name;
    int64_t numel;
    const float** (*to)(thmr_engine*, int);      // null: no call reads the tensor through a pointer of its own (the line says why)
    Place place = OWN;
    int64_t skip = 0;      // floats between the tensor's first element and what `to` points at
};

const Wt kVitStem[] = {      // "backbone."
    {"pos_embed", (TOK + 1) * DIM, at<&HotW::pos>},
    {"patch_embed.proj.weight", (int64_t)DIM * 768, at<&HotW::pe_w>}, {"patch_embed.proj.bias", DIM, at<&HotW::pe_b>}};
const Wt kVitBlock[] = {     // "backbone.blocks.<i>."
    {"norm1.weight", DIM, at<&VitBlockW::n1w>}, {"norm1.bias", DIM, at<&VitBlockW::n1b>},
    {"attn.qkv.weight", (int64_t)3 * DIM * DIM, at<&VitBlockW::qkvw>}, {"attn.qkv.bias", 3 * DIM, at<&VitBlockW::qkvb>},
    {"attn.proj.weight", (int64_t)DIM * DIM, at<&VitBlockW::pw>}, {"attn.proj.bias", DIM, at<&VitBlockW::pb>},
    {"norm2.weight", DIM, at<&VitBlockW::n2w>}, {"norm2.bias", DIM, at<&VitBlockW::n2b>},
    {"mlp.fc1.weight", (int64_t)MLP * DIM, at<&VitBlockW::f1w>}, {"mlp.fc1.bias", MLP, at<&VitBlockW::f1b>},
    {"mlp.fc2.weight", (int64_t)DIM * MLP, at<&VitBlockW::f2w>}, {"mlp.fc2.bias", DIM, at<&VitBlockW::f2b>}};
const Wt kVitTail[] = {      // "backbone."
    {"last_norm.weight", DIM, at<&HotW::lastn_w>}, {"last_norm.bias", DIM, at<&HotW::lastn_b>}};
const Wt kDecStem[] = {      // "smpl_head.transformer."
    {"pos_embedding", E, at<&DecParams::pos>},
    {"to_token_embedding.weight", E, nullptr},      // in the contract, never read: the input token is zero, only the bias reaches layer 0
    {"to_token_embedding.bias", E, at<&DecParams::tok_bias>}};
const Wt kDecLayer[] = {     // "smpl_head.transformer.transformer.layers.<l>."
    {"0.norm.weight", E, at<&DecLayerW::n0w>}, {"0.norm.bias", E, at<&DecLayerW::n0b>},
    {"0.fn.to_qkv.weight", (int64_t)3 * INNER * E, at<&DecLayerW::wv>, OWN, (int64_t)2 * INNER * E},      // read only as its v slice (rows 1024..1535)
    {"0.fn.to_out.0.weight", (int64_t)E * INNER, at<&DecLayerW::wo1>}, {"0.fn.to_out.0.bias", E, at<&DecLayerW::bo1>},
    {"1.norm.weight", E, at<&DecLayerW::n1w>}, {"1.norm.bias", E, at<&DecLayerW::n1b>},
    {"1.fn.to_kv.weight", (int64_t)2 * INNER * DIM, nullptr, KV_GROUP},      // all layers: ONE (dec_depth * 1024, 1280) matrix at o_kv_all
    {"1.fn.to_q.weight", (int64_t)INNER * E, at<&DecLayerW::wq>},
    {"1.fn.to_out.0.weight", (int64_t)E * INNER, at<&DecLayerW::wo2>}, {"1.fn.to_out.0.bias", E, at<&DecLayerW::bo2>},
    {"2.norm.weight", E, at<&DecLayerW::n2w>}, {"2.norm.bias", E, at<&DecLayerW::n2b>},
    {"2.fn.net.0.weight", (int64_t)DEC_MLP * E, at<&DecLayerW::w1>}, {"2.fn.net.0.bias", DEC_MLP, at<&DecLayerW::b1>},
    {"2.fn.net.3.weight", (int64_t)E * DEC_MLP, at<&DecLayerW::w2>}, {"2.fn.net.3.bias", E, at<&DecLayerW::b2>}};
// "smpl_head.": the read-outs are stacked at o_ro_w / o_ro_b (RO_W / RO_B, in table order) and read through DecParams::ro_w / ro_b —
// token head: 6 + 10 + 3 + 12 = 31 rows and a zero padding row so that a clamped row read stays inside the arena; HMR2 head
// (SMPLTransformerDecoderHead, heads/smpl_head.py:32-34,46-48): 144 + 10 + 3 rows, zero rows up to ten whole 16-column tiles
const Wt kRoToken[] = {{"decpose_grot.weight", 6 * E, nullptr, RO_W}, {"decpose_grot.bias", 6, nullptr, RO_B}};
const Wt kRoHmr2[] = {{"decpose.weight", 144 * E, nullptr, RO_W}, {"decpose.bias", 144, nullptr, RO_B}};
const Wt kRoBoth[] = {{"decshape.weight", 10 * E, nullptr, RO_W}, {"decshape.bias", 10, nullptr, RO_B}, {"deccam.weight", 3 * E, nullptr, RO_W}, {"deccam.bias", 3, nullptr, RO_B}};
const Wt kTokenHead[] = {    // the token head behind the shared read-outs: the last read-out, then the token classifier up to its mixer layers
    {"decpose_hands.weight", 12 * E, nullptr, RO_W}, {"decpose_hands.bias", 12, nullptr, RO_B},
    {"decpose.mixer_trans.ff.0.weight", (int64_t)TN * HID * E, at<&DecParams::mt_w>}, {"decpose.mixer_trans.ff.0.bias", TN * HID, at<&DecParams::mt_b>},
    {"decpose.mixer_trans.ff.1.weight", TN * HID, at<&MixerParams::tln_w>}, {"decpose.mixer_trans.ff.1.bias", TN * HID, at<&MixerParams::tln_b>}};
const Wt kMixerLayer[] = {   // "smpl_head.decpose.mixer_head.<m>."
    {"layernorm1.weight", HID, at<&MixerLayerW::ln1w>}, {"layernorm1.bias", HID, at<&MixerLayerW::ln1b>},
    {"MLP_token.ff.0.weight", TOK_INTER * TN, at<&MixerLayerW::wt1>}, {"MLP_token.ff.0.bias", TOK_INTER, at<&MixerLayerW::bt1>},
    {"MLP_token.ff.3.weight", TN * TOK_INTER, at<&MixerLayerW::wt2>}, {"MLP_token.ff.3.bias", TN, at<&MixerLayerW::bt2>},
    {"layernorm2.weight", HID, at<&MixerLayerW::ln2w>}, {"layernorm2.bias", HID, at<&MixerLayerW::ln2b>},
    {"MLP_channel.ff.0.weight", HID_INTER * HID, at<&MixerLayerW::wc1>}, {"MLP_channel.ff.0.bias", HID_INTER, at<&MixerLayerW::bc1>},
    {"MLP_channel.ff.3.weight", HID * HID_INTER, at<&MixerLayerW::wc2>}, {"MLP_channel.ff.3.bias", HID, at<&MixerLayerW::bc2>}};
const Wt kTokenTail[] = {    // "smpl_head.decpose."
    {"mixer_norm_layer.ff.0.weight", HID * HID, at<&MixerParams::wn>}, {"mixer_norm_layer.ff.0.bias", HID, at<&MixerParams::bn>},
    {"mixer_norm_layer.ff.1.weight", HID, at<&MixerParams::nln_w>}, {"mixer_norm_layer.ff.1.bias", HID, at<&MixerParams::nln_b>},
    {"class_pred_layer.weight", NCLS * HID, at<&HotW::cls_w>}, {"class_pred_layer.bias", NCLS, at<&HotW::cls_b>}};
const Wt kMeanParams[] = {   // "smpl_head.", both heads
    {"init_body_pose", 144, at<&HotW::init_pose>}, {"init_betas", 10, at<&HotW::init_betas>}, {"init_cam", 3, at<&HotW::init_cam>}};
const Wt kCodebook[] = {{"quantizer.codebook", NCLS * CODE, at<&HotW::codebook>}};      // tokenizer.pth ['net'], behind kVqDec

}  // namespace

// tokenizer.pth ['net'] decoder (PoseSPDecoderV1, vanilla_pose_vqvae.py:135-154): five Conv1d + ReLU on the 160 -> 125 -> 90 -> 55 -> 21
// resamples, two ResConv1DBlocks (conv1 k = 3, conv2 1 x 1), two more convs
const Conv1d kVqDec[kVqDecN] = {
    {"decoder.decoder.0", CODE, CODE, VQW, 3},
    {"decoder.decoder.3", VQW, VQW, VQW, 3},
    {"decoder.decoder.6", VQW, VQW, VQW, 3},
    {"decoder.decoder.9", VQW, VQW, VQW, 3},
    {"decoder.decoder.12", VQW, VQW, VQW, 3},
    {"decoder.decoder.14.0.model.0.conv1", VQW, VQW, VQW, 3},  // ResConv1DBlock dil 3
    {"decoder.decoder.14.0.model.0.conv2", VQW, VQW, VQW, 1},
    {"decoder.decoder.14.0.model.1.conv1", VQW, VQW, VQW, 3},  // dil 1
    {"decoder.decoder.14.0.model.1.conv2", VQW, VQW, VQW, 1},
    {"decoder.decoder.14.1", VQW, VQW, VQW, 3},
    {"decoder.decoder.15", VQW, VQW, 6, 3},                    // -> (B,21,6)
};
// tokenizer encoder (PoseSPEncoderV1, vanilla_pose_vqvae.py:66-88 with the release ARCH: input_dim 6, width 512, token_size_mul 4,
// down_t 1, stride_t 2, depth 2, dilation 3, code_dim 256).  Optional, all or nothing; not part of thmr_spec
const Conv1d kEnc[kEncN] = {
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

namespace {

struct Ent { std::string name; int64_t numel; Place place; const float** dst; int64_t skip; };

// the tensors of a conv list; w / b (null: none): where the resolved pointers go.  A k > 1 conv is read through its repacked copy, which
// resolve_weights points w[i] at
template <class F>
void walk_convs(const Conv1d* c, int n, const float** w, const float** b, F&& f) {
    for (int i = 0; i < n; ++i) {
        f(Ent{std::string(c[i].name) + ".weight", (int64_t)c[i].co * c[i].ci * c[i].ks, OWN, w && c[i].ks == 1 ? w + i : nullptr, 0});
        f(Ent{std::string(c[i].name) + ".bias", c[i].co, OWN, b ? b + i : nullptr, 0});
    }
}

// every tensor of thmr_spec, in its order; e (may be null): the engine whose pointers Ent::dst names
template <class F>
void walk_contract(int vit_depth, int dec_depth, bool hmr2, thmr_engine* e, F&& f) {
    auto tab = [&](const auto& t, const std::string& prefix, int i = 0) {
        for (const Wt& w : t) f(Ent{prefix + w.name, w.numel, w.place, e && w.to ? w.to(e, i) : nullptr, w.skip});
    };
    tab(kVitStem, "backbone.");
    for (int i = 0; i < vit_depth; ++i) tab(kVitBlock, "backbone.blocks." + std::to_string(i) + ".", i);
    tab(kVitTail, "backbone.");
    tab(kDecStem, "smpl_head.transformer.");
    for (int l = 0; l < dec_depth; ++l) tab(kDecLayer, "smpl_head.transformer.transformer.layers." + std::to_string(l) + ".", l);
    if (hmr2) {      // nothing of the token head follows: no classifier, no VQ decoder, no codebook
        tab(kRoHmr2, "smpl_head.");
        tab(kRoBoth, "smpl_head.");
        tab(kMeanParams, "smpl_head.");
        return;
    }
    tab(kRoToken, "smpl_head.");
    tab(kRoBoth, "smpl_head.");
    tab(kTokenHead, "smpl_head.");
    for (int m = 0; m < MIX; ++m) tab(kMixerLayer, "smpl_head.decpose.mixer_head." + std::to_string(m) + ".", m);
    tab(kTokenTail, "smpl_head.decpose.");
    tab(kMeanParams, "smpl_head.");
    walk_convs(kVqDec, kVqDecN, e ? e->hot.vq_w : nullptr, e ? e->hot.vq_b : nullptr, f);
    tab(kCodebook, "");
}

}  // namespace

void layout_weights(WeightLayout& l, int vit_depth, int dec_depth, bool hmr2) {
    size_t off = 0;
    auto group = [&](Place g) {      // the tensors of one stacked group, back to back
        walk_contract(vit_depth, dec_depth, hmr2, nullptr, [&](const Ent& t) {
            if (t.place != g) return;
            l.slots[t.name] = Slot{off, t.numel, false};
            off += (size_t)t.numel;
        });
    };
    // contiguous groups first: to_kv of all layers -> one (dec_depth*1024, 1280) matrix; read-outs -> (31,1024)+(31) / (160,1024)+(160)
    const size_t ro_pad = hmr2 ? THMR_HMR2_RO_LD - THMR_HMR2_RO_ROWS : 1;      // zero rows behind the read-outs (write_arena_constants)
    l.o_kv_all = off;
    group(KV_GROUP);
    off = align64(off);
    l.o_ro_w = off;
    group(RO_W);
    off = align64(off + ro_pad * E);
    l.o_ro_b = off;
    group(RO_B);
    off = align64(off + ro_pad);
    walk_contract(vit_depth, dec_depth, hmr2, nullptr, [&](const Ent& t) {
        l.required.push_back(t.name);
        if (t.place != OWN) return;
        l.slots[t.name] = Slot{off, t.numel, false};
        off = align64(off + (size_t)t.numel);
    });
    // derived regions
    if (!hmr2) {
        l.convp.resize(kVqDecN);
        for (int i = 0; i < kVqDecN; ++i) {
            l.convp[i] = off;
            if (kVqDec[i].ks > 1) off = align64(off + (size_t)kVqDec[i].co * kVqDec[i].cp * kVqDec[i].ks);
        }
        l.o_cbT = off;   off = align64(off + (size_t)NCLS * CODE);
        l.o_cnorm = off; off = align64(off + NCLS);
        l.o_idx = off;   off = align64(off + 4 * 160);
        l.o_inv = off;   off = align64(off + 4 * 160);
    }
    // SMPL constants
    off = l.smpl.lay(off);
    // optional tokenizer encoder (tokenizer.pth 'encoder.encoder.*'): raw tensors, repacked convs, resample tables
    if (!hmr2) {
        walk_convs(kEnc, kEncN, nullptr, nullptr, [&](const Ent& t) {
            l.enc_names.push_back(t.name);
            l.slots[t.name] = Slot{off, t.numel, false};
            off = align64(off + (size_t)t.numel);
        });
        l.enc_convp.resize(kEncN);
        for (int i = 0; i < kEncN; ++i) {
            l.enc_convp[i] = off;
            if (kEnc[i].ks > 1) off = align64(off + (size_t)kEnc[i].co * kEnc[i].cp * kEnc[i].ks);
        }
        l.o_idx_enc = off; off = align64(off + 640);
    }
    l.o_flags = off;   off = align64(off + 64);     // int32 flag words travelling with the arena (0: encoder present)
    l.wfloats = off;
}

ScratchLayout layout_scratch(int max_batch, bool hmr2) {
    const size_t B = (size_t)max_batch, M = B * TOK;
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off = align64(off + n); return o; };
    ScratchLayout s{};
    s.x = take(M * DIM);
    s.h = take(M * DIM);
    s.big = take(M * 6144);
    {   // split-K partial sums of the proj / fc2 GEMMs: 4 x M x 1280 up to kSmallM rows (ring kernel), 2 x M x 1280 up to kMidHiM rows
        const size_t m2 = M < (size_t)kMidHiM ? M : (size_t)kMidHiM, need = (size_t)kMidSplit * m2;
        s.part_floats = (need > (size_t)kSplitKMax * kSmallM ? need : (size_t)kSplitKMax * kSmallM) * DIM;
        s.part = take(s.part_floats);
    }
    s.dx = take(B * E); s.dh = take(B * E); s.dv = take(B * INNER); s.dq = take(B * INNER); s.dca = take(B * INNER);
    s.dff = take(B * DEC_MLP); s.ro = take(B * (hmr2 ? THMR_HMR2_RO_LD : 32));
    if (!hmr2) {      // the token head's classifier and VQ decoder; the HMR2 head has neither
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
    return s;
}

namespace {

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

// Every weight pointer a call reads, resolved from the name map ONCE (thmr_finalize_weights): the name map is for the layout and the load,
// and no call path looks a tensor up by name.  Also the scratch pointers, knobs and grid limit of the persistent decoder kernel, which
// travel in the same structures.  An unknown name (impossible for a valid layout) fails here instead of leaving a null pointer behind.
int resolve_weights(thmr_engine* e) {
    bool known = true;
    auto resolve = [&](const Ent& t) {
        if (!t.dst) return;
        const float* p = e->W(t.name);
        known = known && p != nullptr;
        *t.dst = p ? p + t.skip : nullptr;
    };
    e->hot = HotW{};
    e->vitw.resize(e->vit_depth);
    walk_contract(e->vit_depth, e->dec_depth, e->hmr2, e, resolve);
    // the optional tokenizer encoder
    if (e->enc_ready) walk_convs(kEnc, kEncN, e->hot.enc_w, e->hot.enc_b, resolve);
    // a k > 1 conv reads its repacked copy (thmr_finalize_weights), a 1 x 1 conv the checkpoint tensor (resolved above)
    for (int i = 0; i < kVqDecN; ++i)
        if (!e->hmr2 && kVqDec[i].ks > 1) e->hot.vq_w[i] = e->warena + e->convp[i];
    for (int i = 0; i < kEncN; ++i)
        if (e->enc_ready && kEnc[i].ks > 1) e->hot.enc_w[i] = e->warena + e->enc_convp[i];
    // decoder / read-out / mixer_trans: the persistent decoder kernel's parameters, and what the launch-chain head reads
    DecParams& d = e->dec;
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
    if (!e->hmr2) { e->mix.mt = e->S(e->so.mt); e->mix.out = e->S(e->so.nl2); }
    return known ? 0 : fail(e, THMR_ERR_STATE, e->err);      // e->err: "internal: unknown weight <name>" (thmr_engine::W)
}

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

// bytes of the engine-owned allocations of the split3 mode (build_split_weights): weight copies, activation operands + fc2's split-K planes
size_t split_w_bytes_of(int vit_depth, int dec_depth) {
    const size_t per_block = (size_t)DIM * (3 * DIM) + (size_t)DIM * DIM + 2 * (size_t)DIM * MLP;      // weights of one block
    const size_t kv_rows = (size_t)dec_depth * 2 * INNER;                                              // + the decoder's to_kv of all layers
    return (per_block * vit_depth + kv_rows * DIM + (size_t)DIM * 768) * 6;                            // + the patch-embed matrix
}
size_t split_act_bytes_of(int max_batch) {
    const size_t M = (size_t)max_batch * TOK;
    return M * (size_t)(DIM + MLP) * 6 + (size_t)kSplit3Fc2Split * M * DIM * 4;
}

// split3 copies of the four ViT GEMM weights of every block (6 bytes per weight) + the activation operand buffers, engine-owned
int build_split_weights(thmr_engine* e, hipStream_t st) {
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

}  // namespace

// zero the hand-over workspace of the persistent split3 GEMM (slabs, epochs, control words) and bind the host-mapped error word again
int reset_s3_workspace(thmr_engine* e, hipStream_t st) {
    HIP_OK(hipMemsetAsync(e->s3_ws, 0, gemm_split3_persist_ws_bytes(), st));
    if (e->s3_host_err && gemm_split3_persist_bind_host_err(e->s3_ws, &e->s3_host_err, st) != 0)
        return fail(e, THMR_ERR_HIP, "binding the host-mapped error word of the split3 hand-over workspace failed");
    return 0;
}

void release_split_weights(thmr_engine* e) {
    if (e->split_w_counted) {
        SplitShare& sh = split_share();
        std::lock_guard<std::mutex> lk(sh.mu);
        auto it = sh.m.find({e->cfg.device, static_cast<const void*>(e->warena)});
        if (it != sh.m.end() && --it->second.refs <= 0) { (void)hipFree(it->second.p); sh.m.erase(it); }
    } else if (e->split_w) (void)hipFree(e->split_w);
}

extern "C" {

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
    const bool hmr2 = (cfg->flags & THMR_CFG_HEAD_HMR2) != 0;
    WeightLayout wl;
    layout_weights(wl, cfg->vit_depth, cfg->dec_depth, hmr2);
    if (weight_bytes) *weight_bytes = wl.wfloats * sizeof(float);
    if (scratch_bytes) *scratch_bytes = layout_scratch(cfg->max_batch, hmr2).total * sizeof(float);
    return 0;
}

int thmr_spec(const thmr_config* cfg, int32_t index, const char** name, int64_t* numel) {
    if (int r = validate_cfg(cfg)) return r;
    static thread_local std::vector<std::pair<std::string, int64_t>> spec;
    spec.clear();
    walk_contract(cfg->vit_depth, cfg->dec_depth, (cfg->flags & THMR_CFG_HEAD_HMR2) != 0, nullptr,
                  [&](const Ent& t) { spec.emplace_back(t.name, t.numel); });
    if (index >= 0 && index < (int32_t)spec.size()) {
        if (name) *name = spec[index].first.c_str();
        if (numel) *numel = spec[index].second;
    }
    return (int)spec.size();
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
        for (int i = 0; i < kVqDecN; ++i)
            if (kVqDec[i].ks > 1)
                LAUNCH_OK(launch_conv_repack(e->W(std::string(kVqDec[i].name) + ".weight"), e->warena + e->convp[i], kVqDec[i].co, kVqDec[i].ci, 3, st));
        LAUNCH_OK(launch_transpose(e->W(kCodebook[0].name), e->warena + e->o_cbT, 1, NCLS, CODE, st));
        LAUNCH_OK(launch_code_norm(e->W(kCodebook[0].name), e->warena + e->o_cnorm, NCLS, st));
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

int thmr_weight_arena(thmr_engine* e, void** ptr_dev, size_t* bytes) {
    if (!e) return fail(e, THMR_ERR_INVALID, "null engine");
    if (ptr_dev) *ptr_dev = e->warena;
    if (bytes) *bytes = e->wfloats * sizeof(float);
    return 0;
}

}  // extern "C"
