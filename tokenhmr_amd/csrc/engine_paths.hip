// What a call of the engine enqueues on the caller's stream, with no allocation and no host synchronisation
// (reference: tokenhmr/lib/models/tokenhmr.py:135-188 forward_step):
//   ViT-H            vit.py:320-343          -> vit_forward()
//   decoder + head   token_head.py:65-128    -> head_forward()
//   SMPL + camera    smpl_wrapper.py:27-41, geometry.py:86-124, tokenhmr.py:165-187 -> lbs()
//   tokenizer        vanilla_pose_vqvae.py   -> vq_decode(), vq_decode_idx(), encode_tokens_call(), tokenizer_roundtrip_call()
// Every weight pointer was resolved at finalize (engine_weights.hip); host code only.
#include <cmath>

#include "engine_state.h"

namespace {

// decoder + mixer stack: the persistent decoder kernel and the one-workgroup-per-crop mixer kernel win while the work is
// latency-bound (B = 1: 0.96 vs 1.01 ms, B = 64: 1.58 vs 1.93 ms per head); from a few hundred crops on the same products are
// real GEMMs (M = B and M = 160 B rows) and the tiled MFMA kernels win (B = 512: 6.7 vs 7.5 ms) — profiles/r2e_head_fused_vs_chain.log
constexpr int kFusedHeadMaxB = 128;

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

}  // namespace

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
    //   THMR_VIT_PATH_SPLIT3: the four GEMMs as split3 products on the bf16 matrix pipe (csrc/gemm_split16.hip); everything else — patch embed,
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
static int vq_tiny_variant(const thmr_engine* e, int B) { return (e->tiny_gemm && B * TOK <= kSmallM) ? 11 : -1; }

// PoseSPDecoderV1 behind the codebook lookup: the operand of decoder.0 (B*160, 3*256) is in the scratch buffer `gat`, written by the soft
// lookup's GEMM (vq_decode) or by the hard lookup kernel (vq_decode_idx, tokenizer_roundtrip) -> bpose (B,21,6)
static int vq_decode_convs(thmr_engine* e, int B, float* bpose, hipStream_t st) {
    auto& so = e->so;
    const int tv = vq_tiny_variant(e, B);
    float* G[2] = {e->S(so.gat), e->S(so.gat2)};          // conv operands, alternating
    float *x0 = e->S(so.act0), *x1 = e->S(so.act1), *hid = e->S(so.act2);
    const int32_t* inv = reinterpret_cast<const int32_t*>(e->warena + e->o_inv);
    // what the consumer conv needs from its producer
    auto scatter = [&](GemmArgs& a, float* dst, const int32_t* table, int tin, int tout, int dil, int relu) {
        a.cs_out = dst; a.cs_inv = table; a.cs_tin = tin; a.cs_tout = tout; a.cs_dil = dil; a.cs_relu = relu;
    };
    // the k = 3 conv `id` of kVqDec itself: operand (B*T, 3*ci) x repacked weight (co, 3*ci)
    auto conv = [&](int id, const float* opnd, int T, float* plain) {
        const int ci = kVqDec[id].ci, co = kVqDec[id].co;
        return mk(opnd, 3 * ci, e->hot.vq_w[id], 3 * ci, e->hot.vq_b[id], nullptr, 0, plain, co, B * T, co, 3 * ci);
    };
    int cur = 0;
    {   // decoder.0: Conv1d(256 -> 512) + ReLU at T = 160 -> operand of decoder.3 on the 160 -> 125 resample
        GemmArgs a = conv(0, G[cur], 160, nullptr);
        scatter(a, G[cur ^ 1], inv + 0 * 160, 160, e->vq_len[1], 1, 0);
        LAUNCH_OK(launch_gemm(a, EPI_BIAS_RELU, tv, st));
        cur ^= 1;
    }
    for (int i = 0; i < 4; ++i) {   // decoder.3/6/9/12: nn.Upsample(size) (a down-sampling here) + Conv1d(512 -> 512) + ReLU
        const int T = e->vq_len[i + 1];
        GemmArgs a = conv(1 + i, G[cur], T, i == 3 ? x0 : nullptr);
        if (i < 3) scatter(a, G[cur ^ 1], inv + (i + 1) * 160, T, e->vq_len[i + 2], 1, 0);
        else scatter(a, G[cur ^ 1], nullptr, VQJ, VQJ, 3, 1);      // -> ResConv1DBlock 0 (dilation 3, pre-activation ReLU); x0 kept as its residual
        LAUNCH_OK(launch_gemm(a, EPI_BIAS_RELU, tv, st));
        cur ^= 1;
    }
    const int Tq = VQJ;
    float* res = x0;
    float* nres = x1;
    for (int blk = 0; blk < 2; ++blk) {   // ResConv1DBlock, resnet.py:49-69: x + conv2(relu(conv1(relu(x)))), dilation 3 then 1
        const int c1 = 5 + 2 * blk, c2 = 6 + 2 * blk;      // kVqDec ids of its conv1 (k = 3) and conv2 (1 x 1)
        {
            GemmArgs a = conv(c1, G[cur], Tq, hid);
            LAUNCH_OK(launch_gemm(a, EPI_BIAS_RELU, tv, st));
        }
        GemmArgs a = mk(hid, VQW, e->hot.vq_w[c2], VQW, e->hot.vq_b[c2], res, VQW, blk == 0 ? nres : nullptr, VQW, B * Tq, VQW, VQW);
        // block 0 feeds block 1's conv1 (pre-activation ReLU) and stays its residual; block 1 feeds decoder.14.1 (no activation)
        scatter(a, G[cur ^ 1], nullptr, Tq, Tq, 1, blk == 0 ? 1 : 0);
        LAUNCH_OK(launch_gemm(a, EPI_BIAS_RESID, tv, st));
        cur ^= 1;
        std::swap(res, nres);
    }
    {   // decoder.14.1: Conv1d(512 -> 512) -> operand of decoder.15
        GemmArgs a = conv(9, G[cur], Tq, nullptr);
        scatter(a, G[cur ^ 1], nullptr, Tq, Tq, 1, 0);
        LAUNCH_OK(launch_gemm(a, EPI_BIAS, tv, st));
        cur ^= 1;
    }
    GemmArgs a = conv(10, G[cur], Tq, bpose);    // decoder.15: Conv1d(512 -> 6): the 21 x 6D body pose
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

PoseBufs pose_bufs(thmr_engine* e, const thmr_outputs* out) {
    const auto& so = e->so;
    return {out && out->rotmat ? out->rotmat : e->S(so.rot), out && out->betas ? out->betas : e->S(so.betas),
            out && out->pred_cam ? out->pred_cam : e->S(so.cam), out && out->pred_cam_t ? out->pred_cam_t : e->S(so.camt)};
}

static int head_forward(thmr_engine* e, const float* ctx, int B, const thmr_outputs* out, hipStream_t st) {
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
    const PoseBufs pb = pose_bufs(e, out);
    if (e->hmr2) {
        // the finish: mean parameters, 6D -> rotation matrices of all 24 joints, camera (hmr2_head.hip) — the second and last launch
        // behind the to_kv GEMM in the fused form
        LAUNCH_OK(launch_hmr2_finish(ro, THMR_HMR2_RO_LD, e->hot.init_pose, e->hot.init_betas, e->hot.init_cam, out ? out->pose6d : nullptr,
                                     pb.rot, pb.betas, pb.cam, pb.camt, out ? out->focal_length : nullptr, FOCAL, IMG, B, st));
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
    LAUNCH_OK(launch_assemble(ro, 32, bpose, e->hot.init_pose, e->hot.init_betas, e->hot.init_cam,
                              out ? out->pose6d : nullptr, pb.rot, pb.betas, pb.cam, pb.camt,
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

// EncodeTokens.forward (tokenization/models/vanilla_pose_vqvae.py:334-342): PoseSPEncoderV1 (:66-111) -> preprocess
// (quantize_cnn.py:74-78) -> QuantizeEMAReset.quantize (:80-86).  pose (B,21,6) rot6d body pose -> idx (B,160).
// Scratch of the encode path, all out of the big time-shared buffer (B*192*6144 floats; the encode path never overlaps a forward on one
// engine): [gather / distance operand B*320*1536 | a0, a1, a2: B*320*512 each | the round trip's statistics: 2048 counts, partial sums].
// None of it is touched by the VQ decoder (gat / gat2 / act0-2 are buffers of their own), so a latent left in a2 survives until the
// round trip's lookup has read it.
static float* enc_scratch_a2(thmr_engine* e, int B) { return e->S(e->so.big) + (size_t)B * 320 * 1536 + 2 * (size_t)B * 320 * VQW; }

// *lat_out: where the latent (B*160, 256) was written — latent_dev, or the scratch region a2
int encode_tokens_call(thmr_engine* e, const float* pose_dev, int B, int32_t* idx_dev, float* latent_dev, const float** lat_out, hipStream_t st) {
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

// VanillaTokenizer.forward (vanilla_pose_vqvae.py:244-255): encoder -> QuantizeEMAReset.forward (quantize_cnn.py:95-130: quantize,
// perplexity, commit loss, straight-through) -> decoder -> rotation_6d_to_matrix (-> matrix_to_axis_angle), on one stream, no allocation,
// no host synchronisation.
int tokenizer_roundtrip_call(thmr_engine* e, const float* pose6d_dev, int B, const thmr_tokenizer_out* out, hipStream_t st) {
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

int head_forward_call(thmr_engine* e, const float* ctx_dev, int32_t B, const thmr_outputs* out, hipStream_t st) {
    if (int r = head_forward(e, ctx_dev, B, out, st)) return r;
    if (out && (out->pred_vertices || out->pred_keypoints_3d || out->pred_keypoints_2d)) {
        const PoseBufs pb = pose_bufs(e, out);
        return lbs(e, pb.rot, pb.betas, pb.camt, B, out->pred_vertices, out->pred_keypoints_3d, out->pred_keypoints_2d, st);
    }
    return 0;
}

int forward_call(thmr_engine* e, const float* img_dev, int32_t B, const thmr_outputs* out, hipStream_t st) {
    float* ctx = e->S(e->so.h);
    if (int r = vit_forward(e, img_dev, B, nullptr, st)) return r;
    if (out->vit_features)
        HIP_OK(hipMemcpyAsync(out->vit_features, ctx, sizeof(float) * (size_t)B * TOK * DIM, hipMemcpyDeviceToDevice, st));
    if (int r = head_forward(e, ctx, B, out, st)) return r;
    const PoseBufs pb = pose_bufs(e, out);
#ifdef THMR_EXPERIMENTS
    // tests only (THMR_SPLIT3_FORCE_TIMEOUT=2): write what a timed-out hand-over consumer writes into the host-mapped error word, once per
    // engine, so that the NEXT forward-type call goes through check_ready's report-reset-fall-back path
    if (e->s3_ws && e->s3_persist && e->vit_gemm_mode == 1 && !e->s3_forced_once && e->s3_host_err) {
        const char* f = thmr_knob("THMR_SPLIT3_FORCE_TIMEOUT");
        if (f && f[0] == '2') { *e->s3_host_err = 1; e->s3_forced_once = true; }
    }
#endif
    return lbs(e, pb.rot, pb.betas, pb.camt, B, out->pred_vertices, out->pred_keypoints_3d, out->pred_keypoints_2d, st);
}
