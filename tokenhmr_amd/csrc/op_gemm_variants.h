// The `variant` ids of the three stateless GEMM operators (thmr_op_gemm, thmr_op_gemm_split3, thmr_op_gemm_split3_out_split3;
// include/tokenhmr_hip.h, tokenhmr_amd/ops.py VARIANT / SPLIT3_VARIANT) as tables: which launcher an id runs, what it hands that launcher,
// which epilogues it takes, whether it exists in the experiments build only and whether it takes a row-blocked operand (+ 1000).
// op_gemm_decode() answers from the tables alone, refusal texts included, so an accepted set is written once.  Host only: what vit_plan.h
// is to the engine's ViT, this is to the operators (ops_abi.hip op_gemm_run does the launches).
#pragma once
#include <array>
#include <string>

#include "../../include/tokenhmr_hip.h"
#include "common.h"

// launcher kinds: the engine's (THMR_GEMM_*, run_gemm in engine.hip) and, behind them, what only the operators reach
constexpr int OPK_F32_SKINNY = 100;      // launch_gemm_skinny (M <= 64)

constexpr unsigned epi_bit(int epi) { return 1u << epi; }
constexpr unsigned kEpiAll = (1u << EPI_NUM) - 1, kEpiNoPos = kEpiAll & ~epi_bit(EPI_BIAS_POS);
constexpr unsigned kS3 = kEpiAll & ~epi_bit(EPI_BIAS_RELU), kS3NoPos = kS3 & kEpiNoPos;      // what the split3 kernels have: 0, 1, 2, 4, 5 (, 6)
constexpr unsigned kS3Out = kS3NoPos & ~epi_bit(EPI_BIAS_RESID);                               // ... with a split3 result: 0, 1, 2, 5
constexpr unsigned kNone = epi_bit(EPI_NONE), kNoneGelu = kNone | epi_bit(EPI_BIAS_GELU);
constexpr unsigned kEpiBlkA = kNone | epi_bit(EPI_BIAS_RESID);                                 // row-blocked A: what fc2 runs

struct OpGemmRow {
    int code;           // the id as callers pass it, without the + 1000 of a row-blocked operand
    int kind;           // THMR_GEMM_* / OPK_*; < 0: a refusal (op_gemm_decode)
    int sub;            // what the launcher gets beside the kind: its own variant (tiles), the LDS ring depth (f32 ring), the mode (wide stream)
    int ksplit;         // > 1: partial planes in op_partial_ws, then launch_splitk_epilogue
    unsigned epis[2];   // bit i = epilogue id i, for an fp32 result / for a split3 result (..._out_split3); 0 = the operator has no such id
    bool exp_only;      // exists in libtokenhmr_hip_exp.so only
    bool blk_a;         // takes a row-blocked A (+ 1000 in thmr_op_gemm_split3; in ..._out_split3 + 1000 is the row-blocked RESULT, any id)
};

// ---- thmr_op_gemm: exact fp32 (gemm_f32.hip, gemm_skinny.hip).  100 + 10 (ring == 8) + log2(ksplit): the small-M ring kernel; 200 + tile /
// 400 + tile: split-K 2 / 4 on a big LDS-DMA tile (0 = cost model).  An id without a row is NOT refused: it is launch_gemm's own (-1 = cost
// model, 0 / 1, 7 ... 13), and what launch_gemm does not know runs its default 128 x 128 tile, as it always has.
constexpr auto kOpGemmF32 = [] {
    std::array<OpGemmRow, 2 + 20 + 300> t{};
    int n = 0;
    t[n++] = {2, OPK_F32_SKINNY, 0, 1, {kEpiAll, 0}, false, false};
    t[n++] = {120, THMR_GEMM_F32_RING16, 0, 1, {kEpiNoPos & ~epi_bit(EPI_BIAS_RESID), 0}, false, false};
    for (int c = 100; c < 120; ++c) t[n++] = {c, THMR_GEMM_F32_RING, c >= 110 ? 8 : 4, 1 << (c % 10), {kEpiNoPos, 0}, false, false};
    for (int c = 200; c < 500; ++c) t[n++] = {c, THMR_GEMM_F32_TILE_SPLITK, c % 100 ? c % 100 : -1, c >= 400 ? 4 : 2, {kEpiNoPos, 0}, false, false};
    return t;
}();

// ---- thmr_op_gemm_split3 / ..._out_split3: split3 operands (gemm_split16.hip; experiments: gemm_split3_exp.hip)
constexpr OpGemmRow kOpGemmS3[] = {
    //code kind                      sub ks  fp32 C    split3 C    exp    blk_a
    {-1,  THMR_GEMM_S3_TILE,          -1, 1, {kS3,      kS3Out},    false, false},     // the engine's rule
    {0,   THMR_GEMM_S3_TILE,           0, 1, {kS3,      kS3Out},    false, true},      // 128 x 256, 8 waves
    {2,   THMR_GEMM_S3_TILE,           2, 1, {kS3,      kS3Out},    false, true},      // 128 x 128, 4 waves
    {5,   THMR_GEMM_S3_TILE,           5, 1, {kS3NoPos, kS3Out},    false, false},     // 128 x 256, the ragged last round as half tiles
    {8,   THMR_GEMM_S3_TILE,           8, 1, {kS3,      kS3Out},    false, true},      // 128 x 128, three-stage ring
    {10,  THMR_GEMM_S3_TILE,          10, 1, {kS3,      kS3Out},    false, false},     // 128 x 256, copies up front
    {202, THMR_GEMM_S3_TILE_SPLITK,    0, 2, {kS3NoPos, 0},         false, true},
    {204, THMR_GEMM_S3_TILE_SPLITK,    0, 4, {kS3NoPos, 0},         false, true},
    {300, THMR_GEMM_S3_STREAM_WIDE,    0, 1, {kS3NoPos, 0},         false, true},      // 256 persistent workgroups, 128 x 256 tile stream
    {302, THMR_GEMM_S3_STREAM_WIDE,    2, 1, {0,        kS3Out},    false, false},     // ... split3 result through swapped operand roles
    {320, THMR_GEMM_S3_STREAM_NARROW,  0, 1, {kS3NoPos, kS3Out},    false, false},     // ... 128 x 128 tile stream
    {322, THMR_GEMM_S3_SPLITK_STREAM,  0, 2, {kS3NoPos, 0},         false, false},
    {324, THMR_GEMM_S3_SPLITK_STREAM,  0, 4, {kS3NoPos, 0},         false, false},
    {1,   THMR_GEMM_S3_TILE,           1, 1, {kS3NoPos, kS3Out},    true,  false},     // 128 x 256, 4 waves
    {4,   THMR_GEMM_S3_TILE,           4, 1, {kS3NoPos, kS3Out},    true,  false},     // 256 x 256
    {6,   THMR_GEMM_S3_TILE,           6, 1, {kS3,      kS3Out},    true,  true},      // 128 x 128, 8 waves
    {7,   THMR_GEMM_S3_TILE,           7, 1, {kS3NoPos, kS3Out},    true,  false},     // the tail's half tiles on 8 waves
    {9,   THMR_GEMM_S3_TILE,           9, 1, {kS3,      kS3Out},    true,  true},      // 128 x 128, 8 waves, three-stage ring
    {11,  THMR_GEMM_S3_TILE,          11, 1, {kS3,      kS3Out},    true,  false},     // 128 x 128, three-stage ring, copies up front
    {20,  THMR_GEMM_S3_TILE,          20, 1, {kS3NoPos, kS3Out},    true,  false},     // round 4's 32x32x16 kernels: 128 x 256 / 128 x 128
    {22,  THMR_GEMM_S3_TILE,          22, 1, {kS3NoPos, kS3Out},    true,  false},
    {3,   THMR_GEMM_S3_TILE,           3, 1, {kNone,    0},         true,  false},     // schedule experiments; 31 ... 37 timing-only
    {31,  THMR_GEMM_S3_TILE,          31, 1, {kNone,    0},         true,  false},
    {32,  THMR_GEMM_S3_TILE,          32, 1, {kNone,    0},         true,  false},
    {34,  THMR_GEMM_S3_TILE,          34, 1, {kNone,    0},         true,  false},
    {37,  THMR_GEMM_S3_TILE,          37, 1, {kNone,    0},         true,  false},
    {100, THMR_GEMM_S3_RING,           0, 1, {kS3NoPos, kS3Out},    true,  false},     // the small-M ring kernel on split3 operands
    {101, THMR_GEMM_S3_RING,           0, 2, {kS3NoPos, 0},         true,  false},
    {102, THMR_GEMM_S3_RING,           0, 4, {kS3NoPos, 0},         true,  false},
    {310, THMR_GEMM_S3_STREAM_WIDE,   10, 1, {kS3NoPos, 0},         true,  false},     // round 4's persistent kernel on 32x32x16 MFMAs:
    {311, THMR_GEMM_S3_STREAM_WIDE,   11, 1, {0,        kNoneGelu}, true,  false},     // fp32 / LDS / swapped-role epilogue
    {312, THMR_GEMM_S3_STREAM_WIDE,   12, 1, {0,        kNoneGelu}, true,  false},
};

enum OpGemmEntry { OP_GEMM_F32 = 0, OP_GEMM_S3 = 1, OP_GEMM_S3_OUT = 2 };
struct OpGemmTable { const char* op; const OpGemmRow* rows; int n; };
constexpr OpGemmTable kOpGemmTables[3] = {{"thmr_op_gemm", kOpGemmF32.data(), (int)kOpGemmF32.size()},
                                          {"thmr_op_gemm_split3", kOpGemmS3, (int)(sizeof(kOpGemmS3) / sizeof(OpGemmRow))},
                                          {"thmr_op_gemm_split3_out_split3", kOpGemmS3, (int)(sizeof(kOpGemmS3) / sizeof(OpGemmRow))}};

inline std::string op_gemm_epi_list(unsigned mask) {
    std::string s;
    for (int i = 0; i < EPI_NUM; ++i)
        if (mask & epi_bit(i)) s += (s.empty() ? "" : ", ") + std::to_string(i);
    return s;
}

// the operator's ids by build, and the ones that take + 1000: the text of a "bad variant" refusal
inline std::string op_gemm_valid_text(const OpGemmTable& t, int out) {
    std::string now, exp, blks;
    for (int i = 0; i < t.n; ++i) {
        const OpGemmRow& x = t.rows[i];
        if (!x.epis[out]) continue;
        std::string& s = x.exp_only ? exp : now;
        s += (s.empty() ? "" : ", ") + std::to_string(x.code);
        if ((out || x.blk_a) && x.code >= 0) blks += (blks.empty() ? "" : ", ") + std::to_string(x.code + 1000);
    }
    return "valid: " + now + "; in the experiments build (libtokenhmr_hip_exp.so) only: " + exp + "; with a row-blocked " +
           (out ? "result: " : "A (epilogues " + op_gemm_epi_list(kEpiBlkA) + "): ") + blks;
}

// the row of (variant, epi); kind < 0 = refused, the reason in `why`.  *blk: the id carried the + 1000 of a row-blocked operand (stripped here, once)
inline OpGemmRow op_gemm_decode(OpGemmEntry entry, int variant, int epi, bool* blk, std::string* why) {
    const OpGemmTable& t = kOpGemmTables[entry];
    const int out = entry == OP_GEMM_S3_OUT;
    *blk = entry != OP_GEMM_F32 && variant >= 1000;
    const int code = *blk ? variant - 1000 : variant;
    const OpGemmRow* r = nullptr;
    unsigned all = entry == OP_GEMM_F32 ? kEpiAll : 0;      // the operator's epilogues: what any of its ids takes
    for (int i = 0; i < t.n; ++i) {
        if (!t.rows[i].epis[out]) continue;
        all |= t.rows[i].epis[out];
        if (t.rows[i].code == code) r = &t.rows[i];
    }
    auto refuse = [&](const std::string& msg) { *why = std::string(t.op) + ": " + msg; return OpGemmRow{variant, -1, 0, 0, {0, 0}, false, false}; };
    if (epi < 0 || epi >= EPI_NUM || !(all & epi_bit(epi))) return refuse("epilogue must be one of " + op_gemm_epi_list(all));
    if (!r && entry == OP_GEMM_F32) return {code, THMR_GEMM_F32_TILE, code, 1, {kEpiAll, 0}, false, false};
    if (!r || (*blk && !out && !r->blk_a)) return refuse("bad variant " + std::to_string(variant) + "; " + op_gemm_valid_text(t, out));
    const unsigned epis = r->epis[out] & (*blk && !out ? kEpiBlkA : kEpiAll);
    if (!(epis & epi_bit(epi))) return refuse("variant " + std::to_string(variant) + " takes epilogues " + op_gemm_epi_list(epis) + " only");
#ifndef THMR_EXPERIMENTS
    if (r->exp_only) return refuse("variant " + std::to_string(variant) + " exists only in the experiments build (libtokenhmr_hip_exp.so)");
#endif
    return *r;
}
