// The stateless C entry points of include/tokenhmr_hip.h: every thmr_op_* operator, the loss values and the evaluation metrics.  None of
// them takes a handle (engine.hip owns the thmr_engine calls, body_model_abi.hip the thmr_smpl / thmr_smplh ones): each validates its
// arguments before any HIP call and then launches what the engine launches, through the same launch_* functions (common.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <map>
#include <mutex>

#include "abi_util.h"
#include "op_gemm_variants.h"
#include "vit_plan.h"      // DIM, INNER

#define THMR_FAIL(code, msg) fail(code, msg)      // HIP_OK / LAUNCH_OK (abi_util.h)

namespace {

// The partial planes of a split-K operator call: one grow-only buffer per (device, stream), whichever kernel writes it — launches on one
// stream are ordered, so they may share a buffer; different streams never do.  (The engine uses its own scratch arena instead.)  `held` is
// locked here and stays locked across the caller's launches that use the buffer; the device is synchronised before a buffer is replaced.
// nullptr: a HIP call failed.
float* op_partial_ws(int dev, void* stream, size_t floats, std::unique_lock<std::mutex>& held) {
    static std::mutex mu;
    static std::map<std::pair<int, void*>, std::pair<float*, size_t>> pool;
    held = std::unique_lock<std::mutex>(mu);
    auto& slot = pool[{dev, stream}];
    if (floats <= slot.second) return slot.first;
    if (slot.first && (hipDeviceSynchronize() != hipSuccess || hipFree(slot.first) != hipSuccess)) return nullptr;
    slot = {nullptr, 0};
    if (hipMalloc(&slot.first, floats * sizeof(float)) != hipSuccess) return slot.first = nullptr;
    slot.second = floats;
    return slot.first;
}

// one GEMM as its table row says (op_gemm_variants.h); the refusals that depend on the shape or the device are written here, once per kind
int op_gemm_run(const OpGemmRow& r, const GemmArgs& a, int epi, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool s3 = r.kind >= THMR_GEMM_S3_TILE && r.kind <= THMR_GEMM_S3_RING;
    const bool wide = r.kind == THMR_GEMM_S3_STREAM_WIDE, narrow = r.kind == THMR_GEMM_S3_STREAM_NARROW;
    if (s3 && r.ksplit > 1 && (a.K % (32 * r.ksplit)) != 0) return fail(THMR_ERR_INVALID, "split3 split-K GEMM: K must be a multiple of 32 * ksplit");
    if (r.ksplit > 1 && ((a.N & 3) || (a.ldc & 3) || ((uintptr_t)a.C & 15)))      // launch_splitk_epilogue's rule, said before anything is launched
        return fail(THMR_ERR_INVALID, "split-K GEMM: the reduce stores 16-byte vectors: N % 4 == 0, ldc % 4 == 0 and C 16-byte aligned");
    if (narrow && !gemm_split3_persist_narrow_ok(a)) return fail(THMR_ERR_INVALID, "persistent 128 x 128 split3 GEMM: N % 128 == 0, >= 256 tiles, K >= 96, row-major A");
    if (wide && !gemm_split3_persist_ok(a))
        return fail(THMR_ERR_INVALID, "persistent split3 GEMM: M % 32 == 0 (a ragged M is served in whole 32-row blocks), N % 256 == 0, ceil(M / 128) * N / 256 >= 256, K >= 64");
    if ((wide || narrow) && !device_has_256_cus())
        return fail(THMR_ERR_INVALID, "persistent split3 GEMM: its 8 x 32 workgroup decomposition needs a 256-CU device (use variant 0 / 2)");
    std::unique_lock<std::mutex> held;       // the partial planes stay ours until the reduce that reads them is launched
    float* part = nullptr;
    if (r.ksplit > 1) {
        int dev = 0;
        HIP_OK(hipGetDevice(&dev));
        part = op_partial_ws(dev, stream, (size_t)r.ksplit * a.M * a.N, held);
        if (!part) return fail(THMR_ERR_HIP, std::string("split-K partial-sum workspace: ") + hipGetErrorString(hipGetLastError()));
    }
    void* ws = nullptr;                      // hand-over workspace of the tile streams
    if (wide || narrow || r.kind == THMR_GEMM_S3_SPLITK_STREAM) {
        ws = gemm_split3_persist_op_ws(st);
        if (!ws) return fail(THMR_ERR_NOMEM, "persistent split3 GEMM: workspace allocation failed");
    }
    switch (r.kind) {
        case THMR_GEMM_F32_TILE: LAUNCH_OK(launch_gemm(a, epi, r.sub, st)); break;
        case OPK_F32_SKINNY: LAUNCH_OK(launch_gemm_skinny(a, epi, st)); break;
        case THMR_GEMM_F32_RING16: LAUNCH_OK(launch_gemm_ring16(a, epi, st)); break;
        case THMR_GEMM_F32_RING: LAUNCH_OK(launch_gemm_ring(a, epi, r.sub, r.ksplit, part, st)); break;
        case THMR_GEMM_F32_TILE_SPLITK: LAUNCH_OK(launch_gemm_splitk(a, r.sub, r.ksplit, part, st)); break;
        case THMR_GEMM_S3_TILE: LAUNCH_OK(launch_gemm_split3(a, epi, r.sub, st)); break;
        case THMR_GEMM_S3_TILE_SPLITK: LAUNCH_OK(launch_gemm_split3_splitk(a, r.ksplit, part, st)); break;
        case THMR_GEMM_S3_STREAM_WIDE: LAUNCH_OK(launch_gemm_split3_persist(a, epi, r.sub, ws, st)); break;
        case THMR_GEMM_S3_STREAM_NARROW: LAUNCH_OK(launch_gemm_split3_persist_narrow(a, epi, ws, st)); break;
        case THMR_GEMM_S3_SPLITK_STREAM:
            if (launch_gemm_split3_splitk_stream(a, r.ksplit, part, ws, st) != 0)
                return fail(THMR_ERR_INVALID, "split-K through the 128 x 128 stream: N % 128 == 0, >= 256 (tile, slice) units, >= 3 K tiles per slice, row-major A");
            break;
#ifdef THMR_EXPERIMENTS
        case THMR_GEMM_S3_RING: LAUNCH_OK(launch_gemm_split3_ring(a, epi, r.ksplit, part, st)); break;
#endif
        default: return fail(THMR_ERR_INVALID, "internal: GEMM kind without a launcher in this build");
    }
    // the fixed-order reduce + epilogue over the partial planes (what the engine fuses into its residual + LayerNorm kernel)
    if (r.ksplit > 1) LAUNCH_OK(launch_splitk_epilogue(a, epi, part, r.ksplit, st));
    return 0;
}

// the checks the three operators share, then the table: fills `r` and `blk`, or refuses
int op_gemm_prepare(OpGemmEntry entry, bool buffers, int epi, const float* bias, const float* resid, int variant, OpGemmRow* r, bool* blk) {
    if (!buffers) return fail(THMR_ERR_INVALID, "null buffer");
    std::string why;
    *r = op_gemm_decode(entry, variant, epi, blk, &why);
    if (r->kind < 0) return fail(THMR_ERR_INVALID, why);
    if (epi != EPI_NONE && !bias) return fail(THMR_ERR_INVALID, "epilogue needs bias");
    if ((epi == EPI_BIAS_RESID || epi == EPI_BIAS_POS) && !resid) return fail(THMR_ERR_INVALID, "epilogue needs resid");
    return 0;
}

}  // namespace

extern "C" {

// ---- the three GEMM operators: validate, decode the variant id (op_gemm_variants.h), launch (op_gemm_run) ----
int thmr_op_gemm(const float* A, int64_t lda, const float* W, const float* bias, const float* resid, float* C, int64_t ldc,
                 int32_t M, int32_t N, int32_t K, int32_t epi, float qscale, int32_t qcols, int32_t variant, void* stream) {
    OpGemmRow r;
    bool blk;
    if (int rc = op_gemm_prepare(OP_GEMM_F32, A && W && C, epi, bias, resid, variant, &r, &blk)) return rc;
    if (M <= 0 || N <= 0 || K <= 0 || lda < K || ldc < N) return fail(THMR_ERR_INVALID, "fp32 GEMM: M, N, K >= 1, lda >= K, ldc >= N");
    GemmArgs a = mk(A, lda, W, K, bias, resid, ldc, C, ldc, M, N, K);
    a.qscale = qscale; a.qcols = qcols;
    return op_gemm_run(r, a, epi, stream);
}

int thmr_op_split3(const float* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows, int32_t K, void* stream) {
    if (!src || !dst) return fail(THMR_ERR_INVALID, "null buffer");
    if (rows <= 0 || K <= 0 || (K % 8) != 0 || (ld_src % 4) != 0 || (ld_dst % 8) != 0 || ld_dst < K || ld_src < K)
        return fail(THMR_ERR_INVALID, "split3: K % 8, ld_src % 4, ld_dst % 8 must be 0 and the strides >= K");
    LAUNCH_OK(launch_split3(src, ld_src, dst, ld_dst, rows, K, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_gemm_split3(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const float* resid, float* C,
                        int64_t ldc, int32_t M, int32_t N, int32_t K, int32_t epi, float qscale, int32_t qcols, int32_t variant,
                        void* stream) {
    OpGemmRow r;
    bool blk;      // A is a ROW-BLOCKED split3 operand ([M / 32][K / 8][3][32][8], rows padded to 32; GemmArgs::a_blk)
    if (int rc = op_gemm_prepare(OP_GEMM_S3, A && W && C, epi, bias, resid, variant, &r, &blk)) return rc;
    if (epi == EPI_BIAS_POS && (N % 4) != 0) return fail(THMR_ERR_INVALID, "split3 GEMM: the pos-embed epilogue needs N % 4 == 0");
    if (M <= 0 || N <= 0 || K <= 0 || (K % 32) != 0 || (lda % 8) != 0 || (ldw % 8) != 0 || lda < K || ldw < K || ldc < N)
        return fail(THMR_ERR_INVALID, "split3 GEMM: K % 32 == 0, lda / ldw multiples of 8 and >= K, ldc >= N");
    GemmArgs a = mk(static_cast<const float*>(A), lda, static_cast<const float*>(W), ldw, bias, resid, ldc, C, ldc, M, N, K);
    a.qscale = qscale; a.qcols = qcols;
    a.a_blk = blk;
    return op_gemm_run(r, a, epi, stream);
}

int thmr_op_gemm_split3_out_split3(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* Cs, int64_t ldcs,
                                   int32_t M, int32_t N, int32_t K, int32_t epi, float qscale, int32_t qcols, int32_t variant, void* stream) {
    OpGemmRow r;
    bool blk;      // the result in the ROW-BLOCKED form ([M / 32][N / 8][3][32][8], Cs holds ceil(M / 32) * 32 rows; GemmArgs::cs_blk)
    if (int rc = op_gemm_prepare(OP_GEMM_S3_OUT, A && W && Cs, epi, bias, nullptr, variant, &r, &blk)) return rc;
    if (M <= 0 || N <= 0 || K <= 0 || (K % 32) != 0 || (lda % 8) != 0 || (ldw % 8) != 0 || lda < K || ldw < K || (N % 8) != 0 ||
        (ldcs % 8) != 0 || ldcs < N)
        return fail(THMR_ERR_INVALID, "split3 GEMM: K % 32 == 0, N % 8 == 0, lda / ldw / ldcs multiples of 8 and >= K / K / N");
    GemmArgs a = mk(static_cast<const float*>(A), lda, static_cast<const float*>(W), ldw, bias, nullptr, 0, nullptr, 0, M, N, K);
    a.qscale = qscale; a.qcols = qcols;
    a.c_split = Cs; a.ldcs = ldcs;
    a.cs_blk = blk;
    return op_gemm_run(r, a, epi, stream);
}

int thmr_op_layernorm(const float* x, const float* g, const float* b, float* y, int32_t rows, int32_t D, float eps,
                      int32_t relu, void* stream) {
    if (!x || !g || !b || !y) return fail(THMR_ERR_INVALID, "null buffer");
    LAUNCH_OK(launch_layernorm(x, g, b, y, rows, D, eps, relu, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_vit_attention(const float* qkv, float* out, int32_t B, void* stream) {
    if (!qkv || !out) return fail(THMR_ERR_INVALID, "null buffer");
    LAUNCH_OK(launch_vit_attention(qkv, out, B, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_vit_attention_split3(const float* qkv, void* out_split, int32_t B, void* stream) {
    if (!qkv || !out_split || B <= 0) return fail(THMR_ERR_INVALID, "bad argument");
    LAUNCH_OK(launch_vit_attention_split3(qkv, out_split, B, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_vit_attention_b16(const float* qkv, void* out, int32_t B, int32_t out_split, int32_t qt, void* stream) {
    if (!qkv || !out || B <= 0) return fail(THMR_ERR_INVALID, "bad argument");
    LAUNCH_OK(launch_vit_attention_b16(qkv, out, B, out_split != 0, qt, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_vit_attention_variant(const float* qkv, float* out, int32_t B, int32_t variant, void* stream) {
    if (!qkv || !out) return fail(THMR_ERR_INVALID, "null buffer");
    LAUNCH_OK(launch_vit_attention_variant(qkv, out, B, variant, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_rot6d(const float* x, float* R, int32_t n, void* stream) {
    if (!x || !R || n < 1) return fail(THMR_ERR_INVALID, "bad argument");
    LAUNCH_OK(launch_rot6d(x, R, n, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_rot6d_backward(const float* x, const float* grad_R, float* grad_x, int32_t n, void* stream) {
    if (!x || !grad_R || !grad_x) return fail(THMR_ERR_INVALID, "rot6d_backward: null buffer");
    if (n < 1) return fail(THMR_ERR_INVALID, "rot6d_backward: n >= 1 is required");
    LAUNCH_OK(launch_rot6d_backward(x, grad_R, grad_x, n, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_aa_to_rotmat(const float* aa, float* R, int32_t n, void* stream) {
    if (!aa || !R || n < 1) return fail(THMR_ERR_INVALID, "bad argument");
    LAUNCH_OK(launch_aa_to_rotmat(aa, R, n, static_cast<hipStream_t>(stream)));
    return 0;
}

// ---- stateless entry points of the row, glue and head kernels (tests/test_gpu_rowops.py): thin wrappers over the launch_* functions the
// engine calls; every argument is validated here, before any HIP call, because several of those launchers validate nothing ----
int thmr_op_splitk_resid_ln(const float* part, int32_t S, int32_t rows, int32_t D, const float* bias, const float* resid, float* xout,
                            const float* gamma, const float* beta, void* y, float eps, int32_t y_is_split3, void* stream) {
    if (!part || !bias || !resid || !xout || !gamma || !beta || !y) return fail(THMR_ERR_INVALID, "splitk_resid_ln: null buffer");
    if (rows <= 0 || S < 1 || D != DIM) return fail(THMR_ERR_INVALID, "splitk_resid_ln: rows >= 1, S >= 1 and D == 1280 are required");
    if (y_is_split3 && S != 2 && S != 4) return fail(THMR_ERR_INVALID, "splitk_resid_ln: the split3 output exists for S = 2 and 4 only");
    LAUNCH_OK(launch_splitk_resid_ln(part, S, rows, D, bias, resid, xout, gamma, beta, static_cast<float*>(y), eps,
                                     static_cast<hipStream_t>(stream), y_is_split3 != 0));
    return 0;
}

int thmr_op_add_ln64(const float* x, const float* y, const float* gamma, const float* beta, float* s_out, float* z_out, int32_t rows,
                     float eps, void* stream) {
    if (!x || !y || !gamma || !beta || !s_out || !z_out) return fail(THMR_ERR_INVALID, "add_ln64: null buffer");
    if (rows <= 0) return fail(THMR_ERR_INVALID, "add_ln64: rows >= 1 is required");
    LAUNCH_OK(launch_add_ln64(x, y, gamma, beta, s_out, z_out, rows, eps, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_transpose(const float* in, float* out, int32_t Bn, int32_t R, int32_t C, void* stream) {
    if (!in || !out) return fail(THMR_ERR_INVALID, "transpose: null buffer");
    if (Bn <= 0 || R <= 0 || C <= 0 || Bn > 65535 || (R + 31) / 32 > 65535)
        return fail(THMR_ERR_INVALID, "transpose: Bn, R, C >= 1, Bn <= 65535 and R <= 32 * 65535 are required (grid y / z)");
    LAUNCH_OK(launch_transpose(in, out, Bn, R, C, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_softmax_argmax(const float* logits, float* probs, int32_t* idx, int32_t rows, void* stream) {
    if (!logits) return fail(THMR_ERR_INVALID, "softmax_argmax: null buffer");
    if (!probs && !idx) return fail(THMR_ERR_INVALID, "softmax_argmax: probs and idx are both null");
    if (rows <= 0) return fail(THMR_ERR_INVALID, "softmax_argmax: rows >= 1 is required");
    LAUNCH_OK(launch_softmax_argmax2048(logits, probs, idx, rows, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_cross_attn(const float* q, const float* kv, int64_t ldkv, int32_t koff, float* out, int32_t B, void* stream) {
    if (!q || !kv || !out) return fail(THMR_ERR_INVALID, "cross_attn: null buffer");
    if (B <= 0 || B > (1 << 24)) return fail(THMR_ERR_INVALID, "cross_attn: 1 <= B <= 2^24 is required");
    if (ldkv <= 0 || koff < 0 || (ldkv % 4) != 0 || (koff % 4) != 0 || (int64_t)koff + 2 * INNER > ldkv)
        return fail(THMR_ERR_INVALID, "cross_attn: ldkv % 4 == 0, koff % 4 == 0 and koff + 1024 <= ldkv are required");
    LAUNCH_OK(launch_cross_attn(q, kv, ldkv, koff, out, B, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_im2col_patch(const float* img, void* A, int32_t B, int32_t out_split, void* stream) {
    if (!img || !A) return fail(THMR_ERR_INVALID, "im2col_patch: null buffer");
    if (B <= 0) return fail(THMR_ERR_INVALID, "im2col_patch: B >= 1 is required");
    if (out_split) LAUNCH_OK(launch_im2col_patch_split3(img, A, B, static_cast<hipStream_t>(stream)));
    else LAUNCH_OK(launch_im2col_patch(img, static_cast<float*>(A), B, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_conv3_gather(const float* in, float* out, const int32_t* src, int32_t Bn, int32_t Tin, int32_t Tout, int32_t C, int32_t dil,
                         int32_t prerelu, void* stream) {
    if (!in || !out) return fail(THMR_ERR_INVALID, "conv3_gather: null buffer");
    if (Bn <= 0 || Tin <= 0 || Tout <= 0 || C <= 0 || (C % 4) != 0 || dil < 1)
        return fail(THMR_ERR_INVALID, "conv3_gather: Bn, Tin, Tout >= 1, C % 4 == 0 and dil >= 1 are required");
    if (!src && Tin < Tout) return fail(THMR_ERR_INVALID, "conv3_gather: without an index table Tin >= Tout is required");
    LAUNCH_OK(launch_conv3_gather(in, out, src, Bn, Tin, Tout, C, dil, prerelu, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_conv_gather(const float* in, float* out, const int32_t* src, int32_t Bn, int32_t Tin, int32_t Tsrc, int32_t Tout, int32_t C,
                        int32_t Cp, int32_t ks, int32_t stride, int32_t pad, void* stream) {
    if (!in || !out) return fail(THMR_ERR_INVALID, "conv_gather: null buffer");
    if (Bn <= 0 || Tin <= 0 || Tsrc <= 0 || Tout <= 0 || C <= 0 || Cp < C || ks < 1 || stride < 1 || pad < 0)
        return fail(THMR_ERR_INVALID, "conv_gather: counts >= 1, Cp >= C, ks >= 1, stride >= 1 and pad >= 0 are required");
    if (!src && Tin < Tsrc) return fail(THMR_ERR_INVALID, "conv_gather: without an index table Tin >= Tsrc is required");
    LAUNCH_OK(launch_conv_gather_general(in, out, src, Bn, Tin, Tsrc, Tout, C, Cp, ks, stride, pad, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_conv_repack(const float* w, float* wp, int32_t co, int32_t ci, int32_t cp, int32_t kk, void* stream) {
    if (!w || !wp) return fail(THMR_ERR_INVALID, "conv_repack: null buffer");
    if (co <= 0 || ci <= 0 || kk <= 0 || cp < ci) return fail(THMR_ERR_INVALID, "conv_repack: co, ci, kk >= 1 and cp >= ci are required");
    if (cp == ci) LAUNCH_OK(launch_conv_repack(w, wp, co, ci, kk, static_cast<hipStream_t>(stream)));
    else LAUNCH_OK(launch_conv_repack_pad(w, wp, co, ci, cp, kk, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_vq_argmin_rows(const float* x, const float* dot, const float* cnorm, int32_t* idx, float* dist, int32_t rows, void* stream) {
    if (!x || !dot || !cnorm || !idx) return fail(THMR_ERR_INVALID, "vq_argmin_rows: null buffer");
    if (rows <= 0) return fail(THMR_ERR_INVALID, "vq_argmin_rows: rows >= 1 is required");
    LAUNCH_OK(launch_vq_argmin_rows(x, dot, cnorm, idx, dist, rows, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_code_norm(const float* cb, float* cn, int32_t ncode, void* stream) {
    if (!cb || !cn) return fail(THMR_ERR_INVALID, "code_norm: null buffer");
    if (ncode <= 0) return fail(THMR_ERR_INVALID, "code_norm: ncode >= 1 is required");
    LAUNCH_OK(launch_code_norm(cb, cn, ncode, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_vq_stats(const float* x, const float* codebook, const int32_t* idx, int32_t rows, int32_t* code_count, int32_t accumulate,
                     float* partial_scratch, float* commit, float* perplexity, void* stream) {
    if (!x || !codebook || !idx || !code_count || !partial_scratch) return fail(THMR_ERR_INVALID, "vq_stats: null buffer");
    if (rows <= 0) return fail(THMR_ERR_INVALID, "vq_stats: rows >= 1 is required");
    LAUNCH_OK(launch_vq_stats(x, codebook, idx, rows, code_count, accumulate != 0, partial_scratch, commit, perplexity, nullptr,
                              static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_aa_to_rotmat_backward(const float* aa, const float* grad_R, float* grad_aa, int32_t n, void* stream) {
    if (!aa || !grad_R || !grad_aa) return fail(THMR_ERR_INVALID, "aa_to_rotmat_backward: null buffer");
    if (n <= 0) return fail(THMR_ERR_INVALID, "aa_to_rotmat_backward: n >= 1 is required");
    LAUNCH_OK(launch_rodrigues_backward(aa, grad_R, grad_aa, n, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_rotmat_to_aa(const float* R, float* aa, int32_t n, void* stream) {
    if (!R || !aa) return fail(THMR_ERR_INVALID, "rotmat_to_aa: null buffer");
    if (n <= 0) return fail(THMR_ERR_INVALID, "rotmat_to_aa: n >= 1 is required");
    LAUNCH_OK(launch_rotmat_to_aa(R, aa, n, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_head_finish(int32_t kind, const float* ro, int32_t ldro, const float* bpose, const float* init_pose, const float* init_betas,
                        const float* init_cam, float* pose6d, float* rotmat, float* betas, float* cam, float* cam_t, float* focal,
                        float focal_length, float img_size, int32_t B, void* stream) {
    if (kind != 0 && kind != 1) return fail(THMR_ERR_INVALID, "head_finish: kind is 0 (token head) or 1 (HMR2 head)");
    if (!ro || !init_pose || !init_betas || !init_cam || !rotmat || !betas || !cam) return fail(THMR_ERR_INVALID, "head_finish: null buffer");
    if (kind == 0 && !bpose) return fail(THMR_ERR_INVALID, "head_finish: the token head needs the VQ-decoded body pose");
    if (B <= 0) return fail(THMR_ERR_INVALID, "head_finish: B >= 1 is required");
    if (ldro < (kind == 0 ? 31 : THMR_HMR2_RO_ROWS))
        return fail(THMR_ERR_INVALID, "head_finish: ldro is below the read-out's column count (31 token head, 157 HMR2 head)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (kind == 0)
        LAUNCH_OK(launch_assemble(ro, ldro, bpose, init_pose, init_betas, init_cam, pose6d, rotmat, betas, cam, cam_t, focal, focal_length,
                                  img_size, B, st));
    else
        LAUNCH_OK(launch_hmr2_finish(ro, ldro, init_pose, init_betas, init_cam, pose6d, rotmat, betas, cam, cam_t, focal, focal_length,
                                     img_size, B, st));
    return 0;
}

int thmr_op_decoder_init(const float* bias, const float* pos, float* x, int32_t B, int32_t E, void* stream) {
    if (!bias || !pos || !x) return fail(THMR_ERR_INVALID, "decoder_init: null buffer");
    if (B <= 0 || E <= 0 || (int64_t)B * E > (int64_t)1 << 30) return fail(THMR_ERR_INVALID, "decoder_init: B, E >= 1 and B * E <= 2^30 are required");
    LAUNCH_OK(launch_decoder_init(bias, pos, x, B, E, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_mean_row_dist(const float* a, const float* b, int32_t n_rows_per_item, int32_t row_lo, int32_t row_hi, int32_t B, float* out,
                          float* workspace, void* stream) {
    if (!a || !b || !out || !workspace) return fail(THMR_ERR_INVALID, "mean_row_dist: null buffer");
    if (B < 1 || n_rows_per_item < 1 || row_lo < 0 || row_hi <= row_lo || row_hi > n_rows_per_item)
        return fail(THMR_ERR_INVALID, "mean_row_dist: B >= 1 and 0 <= row_lo < row_hi <= n_rows_per_item are required");
    if ((int64_t)B * n_rows_per_item > ((int64_t)1 << 29))
        return fail(THMR_ERR_INVALID, "mean_row_dist: B * n_rows_per_item <= 2^29 is required");
    LAUNCH_OK(launch_mean_row_dist(a, b, n_rows_per_item, row_lo, row_hi, B, out, workspace, static_cast<hipStream_t>(stream)));
    return 0;
}

// ---- the forward value of the loss and its gradient (stateless; csrc/loss.hip) ----
// What thmr_val_loss and thmr_val_loss_grad refuse alike, without the entry point's name in front; null when the arguments pass.
static const char* val_loss_refusal(const thmr_val_loss_desc* d, const thmr_val_loss_in* in, int32_t B) {
    if (!in->pred_keypoints_2d || !in->pred_keypoints_3d || !in->pred_rotmat || !in->pred_betas || !in->gt_keypoints_2d ||
        !in->gt_keypoints_3d || !in->gt_pose || !in->gt_betas || !in->has_global_orient || !in->has_body_pose || !in->has_betas)
        return "null input buffer";
    if (B < 1 || B > (1 << 24)) return "1 <= B <= 2^24 is required";
    if (d->mode != THMR_VAL_LOSS_PLAIN && d->mode != THMR_VAL_LOSS_LOOSE) return "mode is THMR_VAL_LOSS_PLAIN (0) or THMR_VAL_LOSS_LOOSE (1)";
    if (d->mode == THMR_VAL_LOSS_LOOSE && (!in->valid_3d || !in->kp2d_thresh || !in->angle_thresh))
        return "the loose mode needs valid_3d, kp2d_thresh and angle_thresh";
    if (d->pelvis_id < 0 || d->pelvis_id >= 44) return "pelvis_id outside [0, 44)";
    if (d->gt_pose_is_rotmat != 0 && d->gt_pose_is_rotmat != 1) return "gt_pose_is_rotmat is 0 or 1";
    if (reinterpret_cast<uintptr_t>(in->gt_keypoints_3d) % 16 != 0 || reinterpret_cast<uintptr_t>(in->pred_keypoints_2d) % 8 != 0)
        return "gt_keypoints_3d must be 16-byte and pred_keypoints_2d 8-byte aligned";
    return nullptr;
}

// the inputs, weights and mode of both launches
static void val_loss_inputs(ValLossArgs& a, const thmr_val_loss_desc* d, const thmr_val_loss_in* in, int32_t B) {
    a.pred_kp2d = in->pred_keypoints_2d; a.pred_kp3d = in->pred_keypoints_3d; a.pred_rotmat = in->pred_rotmat; a.pred_betas = in->pred_betas;
    a.gt_kp2d = in->gt_keypoints_2d; a.gt_kp3d = in->gt_keypoints_3d; a.gt_pose = in->gt_pose; a.gt_betas = in->gt_betas;
    a.has_global_orient = in->has_global_orient; a.has_body_pose = in->has_body_pose; a.has_betas = in->has_betas;
    a.valid_3d = in->valid_3d; a.kp2d_thresh = in->kp2d_thresh; a.angle_thresh = in->angle_thresh;
    a.w[0] = d->w_keypoints_2d; a.w[1] = d->w_keypoints_3d; a.w[2] = d->w_global_orient; a.w[3] = d->w_body_pose; a.w[4] = d->w_betas;
    a.loose_weight = (float)d->loose_weight;
    a.B = B; a.pelvis_id = d->pelvis_id; a.mode = d->mode; a.gt_pose_is_rotmat = d->gt_pose_is_rotmat;
}

int thmr_val_loss(const thmr_val_loss_desc* d, const thmr_val_loss_in* in, int32_t B, const thmr_val_loss_out* out, float* workspace,
                  void* stream) {
    if (!d || !in || !out) return fail(THMR_ERR_INVALID, "val_loss: null descriptor, input or output struct");
    if (const char* why = val_loss_refusal(d, in, B)) return fail(THMR_ERR_INVALID, std::string("val_loss: ") + why);
    if (!workspace) return fail(THMR_ERR_INVALID, "val_loss: null workspace");
    if (reinterpret_cast<uintptr_t>(out->running) % 8 != 0) return fail(THMR_ERR_INVALID, "val_loss: running (7 doubles) must be 8-byte aligned");
    ValLossArgs a{};
    val_loss_inputs(a, d, in, B);
    a.losses = out->losses; a.per_item = out->per_item; a.running = out->running;
    if (d->mode == THMR_VAL_LOSS_LOOSE) {
        a.kp2d_err = out->kp2d_err; a.angle_err = out->angle_err; a.valid2d = out->valid2d; a.weak2d = out->weak2d;
        a.valid_rot = out->valid_rot; a.weak_rot = out->weak_rot; a.conf2d_used = out->conf2d_used; a.conf3d_used = out->conf3d_used;
        a.has_betas_used = out->has_betas_used;
    }
    a.partial = workspace;
    LAUNCH_OK(launch_val_loss(a, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_val_loss_grad(const thmr_val_loss_desc* d, const thmr_val_loss_in* in, const float* pred_cam, double focal_length, double image_size,
                       int32_t B, float** grads_host, void* stream) {
    if (!d || !in || !grads_host) return fail(THMR_ERR_INVALID, "val_loss_grad: null descriptor, input struct or gradient table");
    if (const char* why = val_loss_refusal(d, in, B)) return fail(THMR_ERR_INVALID, std::string("val_loss_grad: ") + why);
    bool any = false;
    for (int i = 0; i < THMR_LOSS_GRAD_SLOTS; ++i) any = any || grads_host[i];
    if (!any) return fail(THMR_ERR_INVALID, "val_loss_grad: every slot of the gradient table is null");
    if (!pred_cam && (grads_host[THMR_LOSS_GRAD_JOINTS] || grads_host[THMR_LOSS_GRAD_CAM]))
        return fail(THMR_ERR_INVALID, "val_loss_grad: the JOINTS and CAM slots need pred_cam (the projection's adjoint)");
    if (pred_cam && !(std::isfinite(focal_length) && focal_length > 0.0 && std::isfinite(image_size) && image_size > 0.0))
        return fail(THMR_ERR_INVALID, "val_loss_grad: focal_length and image_size must be finite and positive when pred_cam is given");
    ValLossGradArgs g{};
    val_loss_inputs(g.in, d, in, B);
    g.pred_cam = pred_cam;
    g.g_kp2d = grads_host[THMR_LOSS_GRAD_KP2D]; g.g_kp3d = grads_host[THMR_LOSS_GRAD_KP3D]; g.g_joints = grads_host[THMR_LOSS_GRAD_JOINTS];
    g.g_cam = grads_host[THMR_LOSS_GRAD_CAM]; g.g_rotmat = grads_host[THMR_LOSS_GRAD_ROTMAT]; g.g_betas = grads_host[THMR_LOSS_GRAD_BETAS];
    g.focal_length = (float)focal_length; g.img_size = (float)image_size;
    LAUNCH_OK(launch_val_loss_grad(g, static_cast<hipStream_t>(stream)));
    return 0;
}

// ---- PoseReConsLoss, value and gradient (stateless; csrc/loss.hip) ----
int thmr_tok_recon_loss(const float* pred_rotmat, const float* gt_rotmat, const float* pred_verts, const float* gt_verts,
                        const float* pred_joints, const float* gt_joints, const float* vert_weights, const float* commit, int32_t pose_kind,
                        int32_t mesh_kind, int32_t joint_kind, int32_t joint_lo, int32_t joint_hi, double w_pose, double w_mesh,
                        double w_joint, double w_commit, double w_total, int32_t B, float* losses, float* grad_rotmat, float* grad_verts,
                        float* grad_joints, float* workspace, void* stream) {
    if (!losses || !workspace) return fail(THMR_ERR_INVALID, "tok_recon_loss: null losses or workspace");
    if (!pred_rotmat != !gt_rotmat || !pred_verts != !gt_verts || !pred_joints != !gt_joints)
        return fail(THMR_ERR_INVALID, "tok_recon_loss: a term's prediction and ground truth are given together or not at all");
    if (!pred_rotmat && !pred_verts && !pred_joints) return fail(THMR_ERR_INVALID, "tok_recon_loss: every term is absent");
    if ((!pred_rotmat && grad_rotmat) || (!pred_verts && grad_verts) || (!pred_joints && grad_joints))
        return fail(THMR_ERR_INVALID, "tok_recon_loss: a gradient is asked for a term that is absent");
    if (B < 1 || B > (1 << 16)) return fail(THMR_ERR_INVALID, "tok_recon_loss: 1 <= B <= 2^16 is required");
    const int32_t kinds[3] = {pose_kind, mesh_kind, joint_kind};
    for (int i = 0; i < 3; ++i) {
        if (kinds[i] == THMR_RECON_GEODESIC)
            return fail(THMR_ERR_UNSUPPORTED, "tok_recon_loss: 'geodesic' is not differentiated here (acos at its clamp has no finite gradient)");
        if (kinds[i] == THMR_RECON_ROTDIST)
            return fail(THMR_ERR_UNSUPPORTED, "tok_recon_loss: 'rotdist' is not differentiated here (acos at its clamp has no finite gradient)");
        if (kinds[i] < THMR_RECON_L1 || kinds[i] > THMR_RECON_WT_L2)
            return fail(THMR_ERR_INVALID, "tok_recon_loss: a kind is THMR_RECON_L1, _L2, _L1_SMOOTH or _WT_L2");
    }
    if (pred_verts && mesh_kind == THMR_RECON_WT_L2 && !vert_weights) return fail(THMR_ERR_INVALID, "tok_recon_loss: 'wt_l2' on the mesh needs the vertex weights");
    if (joint_lo < 0 || joint_hi <= joint_lo || joint_hi > THMR_SMPLH_NOUT)
        return fail(THMR_ERR_INVALID, "tok_recon_loss: 0 <= joint_lo < joint_hi <= 73 is required");
    ReconLossArgs a{};
    a.pred_rot = pred_rotmat; a.gt_rot = gt_rotmat; a.pred_verts = pred_verts; a.gt_verts = gt_verts; a.pred_joints = pred_joints;
    a.gt_joints = gt_joints; a.vert_w = vert_weights; a.commit = commit;
    a.losses = losses; a.grad_rot = grad_rotmat; a.grad_verts = grad_verts; a.grad_joints = grad_joints; a.partial = workspace;
    // WeightedMSE on the pose or the joints has all-ones weights in the reference (losses.py:93-100): it is l2
    a.kind[0] = pose_kind == THMR_RECON_WT_L2 ? THMR_RECON_L2 : pose_kind; a.kind[1] = mesh_kind;
    a.kind[2] = joint_kind == THMR_RECON_WT_L2 ? THMR_RECON_L2 : joint_kind;
    a.jlo = joint_lo; a.jhi = joint_hi; a.B = B;
    a.w[0] = w_pose; a.w[1] = w_mesh; a.w[2] = w_joint; a.w[3] = w_commit; a.w[4] = w_total;
    LAUNCH_OK(launch_recon_loss(a, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_op_token_ce(const float* x, const int32_t* target, int32_t rows, float* out, float* workspace, void* stream) {
    if (!x || !target || !out || !workspace) return fail(THMR_ERR_INVALID, "token_ce: null buffer");
    if (rows < 1) return fail(THMR_ERR_INVALID, "token_ce: rows >= 1 is required");
    if (reinterpret_cast<uintptr_t>(x) % 16 != 0) return fail(THMR_ERR_INVALID, "token_ce: x must be 16-byte aligned");
    LAUNCH_OK(launch_token_ce(x, target, rows, out, workspace, static_cast<hipStream_t>(stream)));
    return 0;
}

// ---- the pose / shape discriminator and its gradient by the inputs (stateless; csrc/discriminator.hip) ----
static_assert(DiscWeights::total == THMR_DISC_WEIGHT_FLOATS && kDiscKpad == THMR_DISC_KPAD, "the header states the weight block's size");
static_assert(THMR_DISC_WS_PER_ITEM == 2 * THMR_DISC_KPAD + 4 * 1024 + 32 + 1, "the header states the workspace");

// What both calls refuse, without the entry point's name in front; fills the inputs and the workspace's regions when the arguments pass.
static const char* disc_prepare(DiscArgs& a, const float* weights, const float* poses, int64_t pose_stride, const float* betas, int32_t B,
                                int32_t loss_div, float** bufs) {
    if (!weights || !poses || !betas || !bufs) return "null weights, poses, betas or buffer table";
    float* ws = bufs[THMR_DISC_WORKSPACE];
    if (!ws) return "null workspace";
    if (B < 1 || B > THMR_DISC_MAX_BATCH) return "1 <= B <= THMR_DISC_MAX_BATCH (256) is required";
    if (loss_div < 0) return "loss_div >= 0 is required (0 = B)";
    if (pose_stride < 207) return "pose_stride >= 207 is required";
    if (reinterpret_cast<uintptr_t>(weights) % 16 != 0 || reinterpret_cast<uintptr_t>(ws) % 16 != 0)
        return "the weight block and the workspace must be 16-byte aligned";
    a.w = weights; a.poses = poses; a.betas = betas; a.pose_stride = pose_stride; a.B = B;
    a.div = (float)(loss_div > 0 ? loss_div : B);
    const size_t n = (size_t)B;
    a.h = ws; a.a1 = a.h + n * THMR_DISC_KPAD; a.a2 = a.a1 + n * 1024; a.dz2 = a.a2 + n * 1024; a.dz1 = a.dz2 + n * 1024;
    a.dh = a.dz1 + n * 1024;
    float* own_out = a.dh + n * THMR_DISC_KPAD;
    a.partial = own_out + n * 32;
    a.want_out = bufs[THMR_DISC_OUT] != nullptr;
    a.out = a.want_out ? bufs[THMR_DISC_OUT] : own_out;
    a.loss = bufs[THMR_DISC_LOSS];
    return nullptr;
}

int thmr_disc_forward(const float* weights, const float* poses, int64_t pose_stride, const float* betas, int32_t B, int32_t loss_div,
                      double target, float** bufs, void* stream) {
    DiscArgs a{};
    if (const char* why = disc_prepare(a, weights, poses, pose_stride, betas, B, loss_div, bufs)) return fail(THMR_ERR_INVALID, std::string("disc_forward: ") + why);
    if (!a.want_out) return fail(THMR_ERR_INVALID, "disc_forward: the OUT slot is null");
    if (a.loss && !std::isfinite(target)) return fail(THMR_ERR_INVALID, "disc_forward: the target must be finite");
    a.target = (float)target;
    LAUNCH_OK(launch_disc_forward(a, static_cast<hipStream_t>(stream)));
    return 0;
}

int thmr_disc_backward(const float* weights, const float* poses, int64_t pose_stride, const float* betas, const float* grad_out, int32_t B,
                       int32_t loss_div, double target, float** bufs, void* stream) {
    DiscArgs a{};
    if (const char* why = disc_prepare(a, weights, poses, pose_stride, betas, B, loss_div, bufs)) return fail(THMR_ERR_INVALID, std::string("disc_backward: ") + why);
    a.grad_poses = bufs[THMR_DISC_GRAD_POSES]; a.grad_betas = bufs[THMR_DISC_GRAD_BETAS]; a.grad_out = grad_out;
    if (!a.grad_poses && !a.grad_betas) return fail(THMR_ERR_INVALID, "disc_backward: the GRAD_POSES and GRAD_BETAS slots are both null");
    if ((a.loss || !grad_out) && !std::isfinite(target)) return fail(THMR_ERR_INVALID, "disc_backward: the target must be finite");
    a.target = (float)target;
    LAUNCH_OK(launch_disc_backward(a, static_cast<hipStream_t>(stream)));
    return 0;
}

// ---- evaluation metrics (stateless) ----
int thmr_eval_pose(const float* pred_j, const float* gt_j, int32_t nj, int32_t gt_stride, const int32_t* kp, int32_t nkp,
                   int32_t pelvis_ind, int32_t pelvis_mode, const float* pred_v, const float* gt_v, int32_t nv, int32_t B,
                   float* mpjpe, float* re, float* pve, float* pelv, void* stream) {
    if (!pred_j || !gt_j || !kp || !mpjpe || !re || !pelv) return fail(THMR_ERR_INVALID, "null buffer");
    if (nkp < 1 || nkp > 64 || gt_stride < 3 || B < 1 || pelvis_ind < 0 || pelvis_ind >= nj || nj < 3)
        return fail(THMR_ERR_INVALID, "bad evaluator arguments (1 <= n_kp <= 64, gt_stride >= 3)");
    if (pelvis_mode != 0 && pelvis_mode != 1) return fail(THMR_ERR_INVALID, "bad evaluator arguments (pelvis_mode is 0 or 1)");
    if (pred_v && gt_v && pve && nv < 1) return fail(THMR_ERR_INVALID, "bad evaluator arguments (PVE needs n_verts >= 1)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    LAUNCH_OK(launch_eval_pose(pred_j, gt_j, nj, gt_stride, kp, nkp, pelvis_ind, pelvis_mode, mpjpe, re, pelv, B, st));
    if (pred_v && gt_v && pve) LAUNCH_OK(launch_eval_pve(pred_v, gt_v, pelv, nv, pve, B, st));
    return 0;
}

int thmr_regress_joints(const float* J, const float* verts, int32_t nj, int32_t nv, int32_t B, float* out, void* stream) {
    if (!J || !verts || !out || nj < 1 || nv < 1 || B < 1) return fail(THMR_ERR_INVALID, "bad argument");
    LAUNCH_OK(launch_regress_joints(J, verts, nj, nv, out, B, static_cast<hipStream_t>(stream)));
    return 0;
}

}  // extern "C"
