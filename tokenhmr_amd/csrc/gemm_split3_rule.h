// Which tile grid a one-workgroup-per-tile split3 GEMM launch runs on: ONE pure function of (M, N, ksplit, row-blocked A, epilogue id,
// variant id, option bits, compute units).  Host only — no HIP header, not common.h — so a plain C++ program can include it
// (tests/test_split3_rule_host.py pins its answers without a GPU).  The tiles are bit-identical (same K order per element), so every
// choice here is purely a matter of time.  gemm_split3_dispatch.hip executes the answer; vit_plan.h decides what comes BEFORE it
// (split factors, tile streams).
#pragma once

namespace split3_rule {

// GemmArgs::tile_opts (A/B only: zero in the shipped library; the experiments build's THMR_SPLIT3_* knobs, gemm_split3_dispatch.hip)
constexpr int kOptNarrow8 = 1;     // the 128 x 128 tile on eight waves of 64 x 32 instead of four of 64 x 64
constexpr int kOptTail8 = 2;       // the half tiles of the tail grid likewise
constexpr int kOptRing2 = 4;       // the 128 x 128 tile with round 5's TWO-stage K ring instead of three stages
constexpr int kOptNoFront = 8;     // small 128 x 256 grids keep their copies spread over the K tile
constexpr int kOptNoTail = 16;     // the ragged last round of a 128 x 256 grid stays whole tiles

// epilogue ids as in common.h GemmEpi (the dispatch file asserts the match): what the tail kernel is instantiated for, and what a
// row-blocked A (fc2's operand) runs with
constexpr int kEpiNone = 0, kEpiBiasResid = 4;
constexpr unsigned kTailEpis = 1u << 0 | 1u << 1 | 1u << 2 | 1u << 4 | 1u << 5;      // none, bias, bias + GELU, bias + residual, bias + q scale

// 128 x 256 (8 waves) unless the whole grid of 128 x 128 tiles still fits ONE round of 256 CUs (the N = 1280 GEMMs at 16 crops, and at
// 7-8 crops with their K split two ways: 240 workgroups instead of 120).  A rounds x tile-time model over both shapes (a 128 x 128 tile
// takes 0.55 of a 128 x 256 one) was tried and is worse wherever it differs — 640 vs 669 crops/s at 15 crops, 665 vs 707 at 48: a partly
// filled last round of big tiles costs less than a full round (profiles/r3ae_split3_tile_rule_ab.log)
constexpr long kOneRound128 = 256;
// round 6: a 128 x 256 grid of at most two rounds issues every copy of a K tile right behind the barrier (gemm_split16.hip FRONT): its
// period is the weights' round trip, not the MFMA time.  Same box, per call (profiles/r6o_*): fc2 at 32 crops (240 tiles) 10.83 -> 10.38
// ms, fc1 / fc2 at 16 crops -0.12 / -0.16, fc1 at 8 -0.08; equal at 64 crops (not used there: more rounds); the three-stage
// 128 x 128 tile LOSES with it (12 copies in a row stall its one wave per SIMD: +0.1 ... +0.26 ms per class at 4 / 8 crops)
constexpr long kFrontMaxTiles = 512;
// round 5: the 128 x 256 grid with its ragged last round as 128 x 128 half tiles (gemm_split16_tail_kernel; fc1 of a 64-crop batch: 1920
// tiles = 7.5 rounds of 256 CUs).  Each tile an XCD has left after its full rounds becomes this many blocks, one per CU, so the left-over
// may be at most half a round: kTailBlocksPerTile rem <= per, below.
constexpr int kTailBlocksPerTile = 2;

struct Choice {
    enum Kind { REFUSE, TILES, TAIL, EXP } kind;
    int shape;              // TILES: the shape of launch_split16_tiles; EXP: the variant id (a 32x32x16 kernel of gemm_split3_exp.hip)
    int q, tail_from;       // TAIL: tiles per XCD, and how many of them stay whole 128 x 256 tiles
    bool tail8;             // TAIL: the half tiles on eight waves (experiments build)
};

// variant: -1 = by the rule   0 = 8 waves of 64x64 on 128x256   2 = 4 waves of 64x64 on 128x128   6 = 8 waves of 64x32 on 128x128
// 8 / 9 = 2 / 6 with a three-stage K ring   10 / 11 = 0 / 8 with front-loaded copies   5 / 7 = 128x256 with the ragged last round as half
// tiles on 4 / 8 waves (refused where that does not apply)   anything else = an id of the experiments build
inline Choice choose(int M, int N, int ksplit, bool a_blk, int epi, int variant, int opts, int cus) {
    const Choice refuse{Choice::REFUSE, 0, 0, 0, false};
    if (a_blk && epi != kEpiNone && epi != kEpiBiasResid) return refuse;      // row-blocked A: raw partial sums and bias + residual only
    const long ks = ksplit > 1 ? ksplit : 1, tiles_m = (M + 127) / 128;
    const bool by_rule = variant < 0;
    if (by_rule) {
        // round 6: the 128 x 128 tile on EIGHT waves of 64 x 32 (variant 6) was built to put two waves on every SIMD where that tile is what
        // runs (few crops) and measured SLOWER than the four-wave form, same box, interleaved, whole path (profiles/r6d_ab_narrow8_*):
        // +5.9 % per call at 4 crops (fc2 +0.19 ms, fc1 +0.14, qkv +0.12 of 8.1), +3.7 % at 8 (fc2 +0.42), +2.9 % at 3, +3.2 % at 5, +0.6 % at
        // 16.  The few-crop K loop is not short of waves: it waits for its LDS-DMA copies (one 48 KB stage in flight per CU against a 1.5 us
        // loaded round trip = the 1.55 us per K tile measured), and eight waves add barrier cost without adding bytes in flight.  Kept as
        // variant 6 / kOptNarrow8 (bit-identical, tested).  The THREE-stage K ring (variant 8: two stages of copies in flight per CU) is
        // what answers that, and what runs.
        const bool n8 = opts & kOptNarrow8, r3 = !(opts & kOptRing2);
        variant = tiles_m * ((N + 127) / 128) * ks <= kOneRound128 ? (n8 ? (r3 ? 9 : 6) : r3 ? 8 : 2) : 0;
    }
    const bool wide_by_rule = by_rule && variant == 0, tail_asked = variant == 5 || variant == 7;
    if (tail_asked || (wide_by_rule && !(opts & kOptNoTail))) {
        // Bit-identical to the plain grid.  On all eight waves (variant 7 / kOptTail8) the half tiles measured equal (fc1 +0.09 ms of 22.1
        // per 64-crop step, whole step +0.1 %: profiles/r6d_ab_narrow8_or_tail8_b64.json); round 5's four-wave form stays.
        if (ksplit <= 1 && N % 256 == 0 && cus >= 16 && cus % 8 == 0 && epi >= 0 && epi < 32 && (kTailEpis >> epi & 1)) {
            const long T = tiles_m * (N / 256), per = cus / 8, q = T / 8, rem = q % per;
            if (T % 8 == 0 && q >= per && rem >= 1 && kTailBlocksPerTile * rem <= per)
                return Choice{Choice::TAIL, 0, (int)q, (int)(q - rem), variant == 7 || (opts & kOptTail8)};
        }
    }
    if (tail_asked) return refuse;                                            // asked for explicitly: fails where the shape does not qualify
    if (wide_by_rule && !(opts & kOptNoFront) && !a_blk && tiles_m * ((N + 255) / 256) * ks <= kFrontMaxTiles) variant = 10;
    constexpr int kShapeIds[7] = {0, 2, 6, 8, 9, 10, 11};                     // the variant id of launch_split16_tiles' shape 0 ... 6
    for (int shape = 0; shape < 7; ++shape)
        if (variant == kShapeIds[shape]) return Choice{Choice::TILES, shape, 0, 0, false};
    return Choice{Choice::EXP, variant, 0, 0, false};
}

}  // namespace split3_rule
