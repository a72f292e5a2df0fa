// Which kernel and which K split every ViT GEMM (and the decoder's to_kv GEMM) of a call runs with: ONE pure function of
// (mode, batch size, static configuration, "are the tile streams available"), evaluated by vit_forward / head_forward at their top and by
// thmr_debug_vit_plan without a GPU.  Host only: no HIP runtime call, no allocation, no engine pointer.
//   * The SPLIT FACTORS of proj / fc2 decide the association of the K sums, i.e. the bits of the result: one factor per RANGE of batch
//     sizes, so a crop's result does not depend on the batch it rides in within a range (batch invariance).
//   * The DECOMPOSITION (one workgroup per tile, the 128 x 256 tile stream, the 128 x 128 tile stream, split K through the stream) decides
//     only time: all are bit-identical for one split factor.
// Every batch-size or tile-count threshold of that dispatch lives here; the shape predicates stay with the launchers
// (gemm_split3_dispatch.hip).  Which tile grid a one-workgroup-per-tile split3 launch then runs on is the second rule, a pure host function
// as well: split3_rule::choose in gemm_split3_rule.h.  (launch_gemm's cost model for the exact-fp32 kernels is still its own.)
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/tokenhmr_hip.h"
#include "common.h"

// shapes of the ViT-H and of the decoder's to_kv that the plan needs (fixed by the reference: vit.py:12-24)
constexpr int TOK = 192, DIM = 1280, MLP = 5120, INNER = 512;

// small-batch ViT path (gemm_ring_kernel): used while M = 192*B <= kSmallM; crossovers measured in profiles/r1_small_gemm_variants.log
constexpr int kSmallM = 1152, kSplitKMax = 4;     // B <= 6
constexpr int kRingWideM = 384;                   // qkv / fc1 use the ring kernel up to two crops
constexpr int kKeysplitMaxB = 2;                  // key-split attention kernel: one and two crops
constexpr bool kAttnB16 = true;                   // split3 mode's attention: true = attention_b16.hip (the mode's arithmetic: three bf16 pieces per operand on the bf16
                                                  // matrix pipe; 4.03 -> 3.48 ms per 64-crop step, profiles/r4r_engine_b64_attention_b16_ab.log), false = the fp32-MFMA kernels with split3 output
// mid-size batches: from 7 to 16 crops proj / fc2 (N = 1280: 110-240 output tiles of 128x128 on 512 resident slots) run split-K 2
// on the big LDS-DMA tiles (measured per batch size and per GEMM, profiles/r3d_mid_batch_splitk_sweep.log, r3f_mid_batch_forced_tile.log:
// -10 % per call at 9 and 10 crops, -2.5 ... -3.7 % at 11 ... 16, -2 % at 7 and 8 with the 64x128 tile; from 17 on the unsplit launch
// is the faster one, and 4 ways never beats 2).  That range is its own regime of the K sum.
constexpr int kMidLoM = 7 * 192, kMidHiM = 16 * 192, kMidSplit = 2;
// thmr_set_vit_gemm(1): the split3 mode serves calls of kSplit3LowMinB (3) crops and more, in ranges.  From THIS many crops on the
// N = 1280 GEMM proj runs with its K sum unsplit (128 x 256 tiles, one workgroup per CU); below it proj / fc2 split K (next constants)
constexpr int kSplit3MinB = 16;
// ... and 5 ... 15 crops run them with proj / fc2 split K two ways (60-120 tiles of 128 x 256 otherwise): the mode's own mid regime
constexpr int kSplit3MidMinB = 5, kSplit3MidSplit = 2;
// ... and 3 and 4 crops four ways (100-120 workgroups of 128 x 128 otherwise: fc2 3.3 vs 2.0 ms per call for the exact-fp32 ring kernel);
// with them 5 / 6 crops run at 447 / 478 crops/s against 413 / 423 (profiles/r3am_split3_mid_regime_3_to_6_crops.log).  One and two
// crops (2-3 row tiles of 128) stay with the exact-fp32 kernels.
constexpr int kSplit3LowMinB = 3, kSplit3LowSplit = 4;
// fc2 (K = 5120) splits K two ways up to 31 crops: 128 x 256 tiles of K = 5120 are ~400 us blocks, and halving them shortens the ragged
// last round — op level 198 vs 229 us at 16 crops, 547 vs 666 at 40, 596 vs 741 at 48 incl. the reduce
// (profiles/r3af_split3_n1280_tile_splitk_sweep.log); per call 702 vs 658 crops/s at 16 crops, 756 vs 707 at 48 — but 773 vs 784 at 32 and
// 775 vs 784 at 64, whose 240 / 480 tiles fill the rounds anyway and where the LayerNorm kernel then reads two partial planes for nothing
// (profiles/r3ag_split3_fc2_splitk_all_batches.log).  One factor per RANGE (batch invariance): split up to 31 crops, unsplit from 32 on —
// the boundary keeps the reference README's batch of 32 at its best (784) and gives up the 7 % at 40-48 crops.
// proj (K = 1280) splits only up to 15 crops.
constexpr int kSplit3Fc2Split = 2, kSplit3Fc2MaxB = 31;
// workgroups of a tile stream = compute units of the device it is offered on: a "round" of a per-tile grid is this many tiles
constexpr long kStreamWgs = 256;

// Every A/B-knob-backed value that influences a ViT / to_kv decision; the defaults are what the shipped library runs (it reads no
// environment: engine.hip read_knobs fills this from THMR_* variables in the experiments build only).
struct VitKnobs {
    bool qkv_ring16 = true;           // THMR_QKV_RING16=0: one and two crops keep the 64x64 ring kernel for qkv
    bool attn_keysplit = true;        // THMR_ATTN_KEYSPLIT=0: one and two crops keep the 64-query attention workgroups
    bool attn_b16 = kAttnB16;         // THMR_ATTN_B16=0 / 1: split3 mode's attention on the bf16 matrix pipe too (csrc/attention_b16.hip)
    int mid_split_force[2] = {-1, -1};   // THMR_MID_SPLIT=<p><f> (digits 0|2|4): force the split factors of proj and fc2 above 6 crops (exact-fp32 path) where the partial-sum buffer allows
    bool split3_small = false;        // THMR_SPLIT3_SMALL=1: the split3 mode also serves up to six crops (ring kernel on split3 operands) — measured SLOWER
    int split3_fc2_split = kSplit3Fc2Split;   // THMR_SPLIT3_FC2_SPLIT=1: fc2 of the split3 mode unsplit from 5 crops on
    int split3_min_b = 0;             // THMR_SPLIT3_MIN_B=<n>: the smallest batch the split3 mode serves (0 = kSplit3LowMinB)
    int tile_opts = 0;                // GemmArgs::tile_opts of the split3 GEMMs (the bits of gemm_split3_rule.h, from split3_tile_knobs())
    // persistent split3 GEMM = the 128 x 256 tile stream (csrc/gemm_split16.hip; bit-identical to the one-workgroup-per-tile kernel, so
    // purely a matter of time).  THMR_SPLIT3_PERSIST=0: no stream of either width (the engine's run-time copy also drops to 0 after a
    // recovered hand-over timeout)
    int persist = 1;
    // THMR_SPLIT3_FC1_MODE=0: fc1 stays off the 128 x 256 stream whatever the rules below say (non-zero: its split3 output leaves the stream
    // through swapped operand roles)
    int fc1_mode = 2;
    // THMR_SPLIT3_PERSIST_MASK: which GEMMs run the 128 x 256 stream WHEREVER its shape predicate holds: bit 0 qkv, 1 proj, 2 fc1, 3 fc2, 4 the
    // decoder's to_kv.  It pays per tile boundary
    // (hand-over slabs, segment bookkeeping, register spills around its epilogue) and wins the ragged last round: with the 16x16x32
    // kernel it is the faster one for fc2 (K = 5120: 671 vs 715 us) and ties or loses at K = 1280 (qkv 518 vs 515, proj 199 vs 187,
    // fc1 with split3 output 728 vs 702; profiles/r4k_split3_gemm_b64_mfma16.jsonl; whole path 834 vs 822 crops/s with all four,
    // profiles/r4l_engine_b64_persist_min_k_ab.log).  Round 5, same-box interleaved, the whole path at 64 crops (profiles/r5j_ab_mask8_vs_*):
    // + proj +0.33 ms per step (a build whose proj instantiation had NO scratch access in its K loop), + qkv +0.96 ms: at 40 K tiles per
    // tile the hand-over costs more than the ragged round's 6 %.  Same bits either way.
    int persist_mask = 8;
    // THMR_SPLIT3_PN_MASK, round 6: qkv (bit 0), fc1 (bit 1) and proj (bit 2, OFF) of few-crop calls as 256 persistent workgroups over the
    // 128 x 128 tile stream (three-stage ring) when that grid is more than one round, at most pn_max tiles, and the 128 x 256 grid would
    // fill its rounds to at most pn_fill per cent (gemm_split16.hip launch_split16_persist narrow); bit 3: split-K launches (proj / fc2
    // partial sums) as (tile, K slice) units of the same stream, up to pk_max units
    int pn_mask = 11;
    int pn_max = 600;                 // THMR_SPLIT3_PN_MAX: most 128 x 128 tiles the stream takes (it loses from ~700 on: qkv at 16 crops +0.25 ms)
    int pn_fill = 72;                 // THMR_SPLIT3_PN_FILL: use the 128 x 128 stream when the 128 x 256 grid fills its rounds to at most this many per cent
    int pn_fill_proj = 60;            // THMR_SPLIT3_PN_FILL_PROJ: the same for proj (mask bit 2, OFF — 36-40 crops: proj -0.46 ... -0.59 ms per call, the call as a whole equal: profiles/r6x_*)
    int pk_max = 1000;                // THMR_SPLIT3_PK_MAX: most (tile, K slice) units of a split-K launch through the stream
    int pw_fill = 72;                 // THMR_SPLIT3_PW_FILL: the 128 x 256 stream for qkv when its per-tile grid fills its rounds to at most this many per cent
    // THMR_SPLIT3_PW_FC1=0: off.  fc1 takes the 128 x 256 stream where its grid is MORE than two rounds and at most pw_fill per cent full
    // (17 / 18 crops: 520 / 540 tiles = three rounds of time for 2.03 / 2.1 of work: fc1 -0.43 / -0.75 ms per call, profiles/r6z_*); below two
    // rounds its GELU + split3 epilogue (spills in the persistent form) loses what the rounds gain (12 crops: +0.16)
    int pw_fc1 = 1;
    bool bs_blk = true;               // THMR_SPLIT3_BS_BLK=0: fc1 -> fc2 operand row-major even where fc2 runs the 128 x 256 stream
};

struct VitPlanIn {                    // facts of this engine and this call
    int mode;                         // 0 exact fp32, 1 split3 (vit_gemm_mode)
    int B, dec_depth;
    bool split_ready;                 // the split3 weight copies and operand buffers exist (mode 1, max_batch >= kSplit3LowMinB, finalized)
    bool streams;                     // hand-over workspace allocated (256-CU device, not THMR_CFG_NO_PERSISTENT) and no hand-over timeout recovered
    size_t part_floats;               // capacity of the scratch arena's partial-sum buffer
};

using GemmChoice = thmr_gemm_choice;  // { kind (THMR_GEMM_*), ksplit (1 = unsplit) }
using VitPlan = thmr_vit_plan_desc;   // the plan IS what thmr_debug_vit_plan reports (include/tokenhmr_hip.h)

namespace vit_plan_detail {

inline GemmChoice choice(int kind, int ksplit = 1) { return GemmChoice{kind, ksplit}; }
// shape-only GemmArgs for the predicates of gemm_split3_dispatch.hip: row-major operands of leading dimension K, optional split3 output
inline GemmArgs shape(int M, int N, int K, int ksplit = 1, int ldcs = 0) {
    GemmArgs a{};
    a.M = M; a.N = N; a.K = K; a.lda = K; a.ldw = K; a.ldc = N; a.ldr = N; a.ldcs = ldcs; a.ksplit = ksplit;
    return a;
}
inline long tiles(const GemmArgs& a, int bn) { return (long)((a.M + 127) / 128) * ((a.N + bn - 1) / bn); }
// the one-workgroup-per-tile grid of `wide` tiles fills its rounds to at most `fill` per cent
inline bool badly_filled(long wide, int fill) { return 100 * wide <= fill * kStreamWgs * ((wide + kStreamWgs - 1) / kStreamWgs); }

// The 128 x 128 grid is more than one round of 256 workgroups, and the 128 x 256 grid it would otherwise run fills its rounds badly:
// then the stream over 128 x 128 tiles wins (a K tile costs it ~1.3 us + ~10 us per launch, against 2.15 us per wide K tile and whole
// rounds).  Measured per class, same box (profiles/r6k_*): qkv at 6 / 12 crops (135 / 270 wide tiles, rounds 53 % full) 2.75 -> 2.13 and
// 4.87 -> 3.64 ms per call, fc1 at 6 / 10 crops (70 % / 59 %) 2.92 -> 2.63 and 5.10 -> 3.94; at 8 crops qkv (70 %) 2.70 -> 2.62; it
// LOSES where the wide rounds are full (fc1 at 8 crops, 94 %: +0.26; qkv at 10, 88 %: +0.34) and from ~700 tiles on (qkv at 16: +0.25).
inline bool narrow_stream(const VitKnobs& k, const GemmArgs& a, int fill) {
    const long t128 = tiles(a, 128);
    return t128 > kStreamWgs && t128 <= k.pn_max && badly_filled(tiles(a, 256), fill) && gemm_split3_persist_narrow_ok(a);
}
// ... and the stream over 128 x 256 tiles (round 4's persistent kernel; until round 6 fc2's only, where it wins at every size) for qkv
// too WHEN its one-workgroup-per-tile grid fills its rounds badly and the 128 x 128 stream above does not apply: at 64 crops (94 % full)
// the hand-overs cost qkv +6 %; at 24 crops its 540 tiles are 2.1 rounds = three rounds of time: 7.49 -> 6.93 ms per call, at 14 crops
// (315 tiles, 62 %) 5.02 -> 4.45 (profiles/r6m_*).  fc1 only above two rounds (pw_fc1); not proj: measured equal or slower (+0.12 at 36)
inline bool wide_stream(const VitKnobs& k, const GemmArgs& a, long min_tiles) {
    const long wide = tiles(a, 256);
    return wide >= min_tiles && badly_filled(wide, k.pw_fill) && gemm_split3_persist_ok(a);
}
// split-K launches (proj / fc2 below 16 / 32 crops) through the 128 x 128 stream: units = (tile, K slice); taken where the grid the rule would
// launch fills its rounds badly — e.g. fc2 at 18 crops = 270 workgroups of 128 x 256 x (K / 2) = two rounds for 1.05 rounds of work
inline GemmChoice splitk(const VitKnobs& k, bool streams, int M, int N, int K, int ks) {
    const GemmArgs a = shape(M, N, K, ks);
    const long units = tiles(a, 128) * ks;
    const bool stream = streams && (k.pn_mask & 8) && units > kStreamWgs && units <= k.pk_max && badly_filled(tiles(a, 256) * ks, k.pn_fill) &&
                        gemm_split3_persist_narrow_ok(a);
    return choice(stream ? THMR_GEMM_S3_SPLITK_STREAM : THMR_GEMM_S3_TILE_SPLITK, ks);
}

}  // namespace vit_plan_detail

inline VitPlan plan_vit(const VitKnobs& k, const VitPlanIn& in) {
    using namespace vit_plan_detail;
    const int B = in.B, M = B * TOK;
    const bool streams = in.streams && k.persist;
    const bool s3_on = in.mode == 1 && B >= (k.split3_min_b > 0 ? k.split3_min_b : kSplit3LowMinB) && in.split_ready;
    // Few crops (M <= kSmallM): the N = 1280 GEMMs run split-K on the 64x64 ring kernel and their partial sums are reduced
    // inside the residual + LayerNorm kernel that follows them anyway; qkv / fc1 use the ring kernel up to M = 384.
    const bool small = M <= kSmallM, ring_wide = M <= kRingWideM;
    VitPlan p{};
    p.tile_opts = k.tile_opts;
    // the decoder's to_kv of all layers (N = dec_depth * 1024, K = 1280): a split3 product wherever the ViT's are
    p.to_kv = choice(THMR_GEMM_F32_TILE);
    if (s3_on) {
        const bool ws = streams && (k.persist_mask & 16) && gemm_split3_persist_ok(shape(M, in.dec_depth * 2 * INNER, DIM));
        p.to_kv = choice(ws ? THMR_GEMM_S3_STREAM_WIDE : THMR_GEMM_S3_TILE);
    }
    if (s3_on) {
        p.path = THMR_VIT_PATH_SPLIT3;
        p.patch = choice(THMR_GEMM_S3_TILE);
        p.attn = k.attn_b16 ? THMR_ATTN_B16 : THMR_ATTN_F32_SPLIT3_OUT;
        // 3 ... 4 / 5 ... 15 crops: proj / fc2 split K four / two ways, reduced (in a fixed order) by the residual + LayerNorm kernel, as in
        // the exact-fp32 path's regimes; 16 ... 31: only fc2 (two ways); 32 and more: unsplit.  One factor per range: a crop's result is
        // batch-independent within it.
        const bool low = B < kSplit3MidMinB;                     // 3 and 4 crops: both N = 1280 GEMMs four ways
        const int ks_proj = low ? kSplit3LowSplit : B < kSplit3MinB ? kSplit3MidSplit : 1;
        const int ks_fc2 = low ? kSplit3LowSplit : B <= kSplit3Fc2MaxB ? k.split3_fc2_split : 1;
        // fc2's partial sums: the engine-owned planes behind the operand buffers (two planes for any batch size); the four planes of
        // 3 and 4 crops fit the scratch arena's `part` (4 x 1152 rows)
        p.part2_in_scratch = low;
        // a GEMM whose persist_mask bit is set runs the 128 x 256 stream wherever the kernel serves its shape
        auto forced_wide = [&](int bit, const GemmArgs& a) { return streams && (k.persist_mask & bit) && gemm_split3_persist_ok(a); };
        const GemmArgs qkv = shape(M, 3 * DIM, DIM), proj = shape(M, DIM, DIM), fc2 = shape(M, DIM, MLP);
        const GemmArgs fc1 = shape(M, MLP, DIM, 1, MLP);         // split3 output (GemmArgs::c_split) of leading dimension 5120: nothing the predicates refuse
        p.qkv = choice(forced_wide(1, qkv)                                              ? THMR_GEMM_S3_STREAM_WIDE
                       : streams && (k.pn_mask & 1) && narrow_stream(k, qkv, k.pn_fill) ? THMR_GEMM_S3_STREAM_NARROW
                       : streams && wide_stream(k, qkv, kStreamWgs)                     ? THMR_GEMM_S3_STREAM_WIDE
                                                                                        : THMR_GEMM_S3_TILE);
        // proj unsplit (from 16 crops on; K = 1280, 5 wide column tiles): the 128 x 128 stream only where its wide rounds are at most
        // pn_fill_proj per cent full, and only with mask bit 2
        const int fill_proj = k.pn_fill_proj ? k.pn_fill_proj : k.pn_fill;
        p.proj = ks_proj > 1 ? splitk(k, streams, M, DIM, DIM, ks_proj)
                 : choice(forced_wide(2, proj)                                               ? THMR_GEMM_S3_STREAM_WIDE
                          : streams && (k.pn_mask & 4) && narrow_stream(k, proj, fill_proj) ? THMR_GEMM_S3_STREAM_NARROW
                                                                                             : THMR_GEMM_S3_TILE);
        p.fc1 = choice(streams && k.fc1_mode && ((k.persist_mask & 4) || (k.pw_fc1 && wide_stream(k, fc1, 2 * kStreamWgs))) && gemm_split3_persist_ok(fc1)
                           ? THMR_GEMM_S3_STREAM_WIDE
                       : streams && (k.pn_mask & 2) && narrow_stream(k, fc1, k.pn_fill) ? THMR_GEMM_S3_STREAM_NARROW
                                                                                        : THMR_GEMM_S3_TILE);
        p.fc2 = ks_fc2 > 1 ? splitk(k, streams, M, DIM, MLP, ks_fc2) : choice(forced_wide(8, fc2) ? THMR_GEMM_S3_STREAM_WIDE : THMR_GEMM_S3_TILE);
        // fc1's output = fc2's A in the ROW-BLOCKED form (common.h GemmArgs::a_blk) when fc2 runs the 128 x 256 stream: the epilogue (one output
        // row per lane) then writes 256-512 contiguous bytes per 16-32 lanes instead of a different line per lane (same box: 830-832 -> 846-848
        // crops/s at 64 crops, profiles/r4h_row_blocked_ab_same_box_b64.log; with the 16x16x32 kernel fc1 718 -> 702 us and fc2 677 -> 671,
        // r4k_split3_gemm_b64_mfma16.jsonl).  A per-tile fc2 measured SLOWER with a blocked A (778 vs 715 us) and keeps the row-major form
        // (fewer than 32 crops, odd batches).  Same values either way.
        p.bs_blk = k.bs_blk && p.fc2.kind == THMR_GEMM_S3_STREAM_WIDE;
        return p;
    }
    p.patch = choice(THMR_GEMM_F32_TILE);
    if (in.mode == 1 && small && k.split3_small && in.split_ready) {
        // EXPERIMENT (THMR_SPLIT3_SMALL=1): up to six crops on the ring kernel over split3 operands, proj / fc2 four ways as in the fp32 regime
        p.path = THMR_VIT_PATH_SPLIT3_SMALL;
        p.attn = THMR_ATTN_F32_SPLIT3_OUT;
        p.qkv = p.fc1 = choice(THMR_GEMM_S3_RING);
        p.proj = p.fc2 = choice(THMR_GEMM_S3_RING, kSplitKMax);
        return p;
    }
    p.path = THMR_VIT_PATH_F32;
    // one and two crops: qkv on 64 x 48 tiles of 16x16x4 MFMAs (240 / 480 workgroups whose waves walk 12.8 us chains) instead of 64x64
    // tiles of 32x32x2 (180 / 360 workgroups, 17.1 us chains); another order of the K sum, hence tied to that regime
    p.qkv = choice(B <= kKeysplitMaxB && k.qkv_ring16 ? THMR_GEMM_F32_RING16 : ring_wide ? THMR_GEMM_F32_RING : THMR_GEMM_F32_TILE);
    // one or two crops: keys split over the waves of a workgroup (192 / 96 workgroups per crop instead of 48, 120 / 240 instead
    // of 480 dependent MFMAs per wave): -3.9 % per call at one crop, -1 % at two, slower from three on, where its four-fold
    // re-reads of K / V cost more than the shorter chain saves (profiles/r3j_attention_keysplit_ab.log).  Its own association of
    // the key sum, hence its own regime {1, 2} inside the small-batch regime.
    p.attn = B <= kKeysplitMaxB && k.attn_keysplit ? THMR_ATTN_F32_KEYSPLIT : THMR_ATTN_F32;
    p.fc1 = choice(ring_wide ? THMR_GEMM_F32_RING : THMR_GEMM_F32_TILE);
    // proj / fc2: one split factor for the whole small regime (B <= 6, ring kernel), and ONE factor for the mid range (7 ... 16 crops, big
    // tiles) and both GEMMs, so a crop's result does not depend on the batch it rides in within a range
    auto n1280 = [&](int forced) {
        if (small) return choice(THMR_GEMM_F32_RING, kSplitKMax);
        int sp = forced >= 0 ? (forced > 1 ? forced : 1) : (M >= kMidLoM && M <= kMidHiM) ? kMidSplit : 1;
        if ((size_t)sp * M * DIM > in.part_floats) sp = 1;      // only reachable with the A/B knob
        return choice(sp > 1 ? THMR_GEMM_F32_TILE_SPLITK : THMR_GEMM_F32_TILE, sp);
    };
    p.proj = n1280(k.mid_split_force[0]);
    p.fc2 = n1280(k.mid_split_force[1]);
    return p;
}
