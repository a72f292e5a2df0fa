// fp32 GEMM on the bf16 matrix pipe:  C[M,N] = epilogue(A[M,K] . W[N,K]^T)  with every fp32 operand carried as THREE bf16 pieces.
//
// Why: exact-fp32 MFMA (v_mfma_f32_32x32x2_f32, gemm_f32.hip) runs at 1/16 of the bf16 rate on gfx950 (157 vs 2500 TFLOP/s) and the
// ViT GEMMs of the reference (tokenhmr/lib/models/backbones/vit.py:82-87,104-126) already sit at 0.93 of that peak.  An fp32 number
// is the exact sum of three bf16 numbers, x = h + m + l (8 + 8 + 8 significand bits, each piece the round-to-nearest bf16 of what
// the pieces before it left), a product of two bf16 is exact in fp32, and
//     a.b = hh + (hm + mh) + (mm + hl + lh) + [ml + lm + ll]
// where the bracket is below 2^-23 of |a.b| — the size of ONE fp32 rounding, which an fp32 dot product of length K commits K times.
// So six bf16 MFMAs (fp32 accumulate) per K step give an fp32-grade product at 16 / 6 = 2.67 times the matrix rate.
//
// Operand format ("split3"): X[R][K] fp32  ->  Xs[R][K/8][3][8] bf16: 8 consecutive k of a row as three adjacent 16-byte chunks
// (piece h, m, l).  One chunk is exactly one lane's A / B operand of a bf16 MFMA (8 consecutive k of one row), a row
// of a 32-deep K tile is 192 contiguous bytes, a row of the matrix is 6 K bytes.
//
// This file: the producers of that format from fp32 (plain conversion; LayerNorm with a split3 result).  The GEMM kernels over it are
// gemm_split16.hip, their launchers and the tile rule gemm_split3_dispatch.hip + gemm_split3_rule.h, the measured-slower 32x32x16
// kernels of the experiments build gemm_split3_exp.hip.
#include "common.h"
#include "gemm_device.h"
#include "gemm_split_device.h"

namespace {

// X[rows][lds] fp32 -> split3 (row stride ldd fp32-equivalents = 6 ldd bytes); thread = 8 consecutive k of one row
__global__ __launch_bounds__(256) void split3_kernel(const float* __restrict__ src, int64_t lds_, char* __restrict__ dst, int64_t ldd,
                                                     int64_t rows, int kg) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * kg) return;
    const int64_t r = idx / kg;
    const int g = (int)(idx - r * kg);
    const f32x4* p = reinterpret_cast<const f32x4*>(src + r * lds_ + (int64_t)g * 8);
    const f32x4 v0 = p[0], v1 = p[1];
    const float x[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    uint32_t h[8], m[8], l[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        h[e] = bf16_rne(x[e]);
        const float r1 = x[e] - __uint_as_float(h[e] << 16);          // exact: the residual of a rounding fits the format
        m[e] = bf16_rne(r1);
        const float r2 = r1 - __uint_as_float(m[e] << 16);            // exact
        l[e] = bf16_rne(r2);
    }
    u32x4* o = reinterpret_cast<u32x4*>(dst + r * ldd * 6 + (int64_t)g * 48);
    o[0] = u32x4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
    o[1] = u32x4{m[0] | (m[1] << 16), m[2] | (m[3] << 16), m[4] | (m[5] << 16), m[6] | (m[7] << 16)};
    o[2] = u32x4{l[0] | (l[1] << 16), l[2] | (l[3] << 16), l[4] | (l[5] << 16), l[6] | (l[7] << 16)};
}

// nn.LayerNorm over D = NV * 256 (vit.py:136,144; the arithmetic of rowops.hip::ln_wave_kernel, one wave per row) with the result
// written as a split3 operand: lane l holds 4 consecutive elements, so lanes 2 j and 2 j + 1 write the two 8-byte halves of the three
// chunks of k-group j — the fp32 copy of the normalised row is never written.
template <int NV>
__global__ __launch_bounds__(256) void ln_split3_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, char* __restrict__ y, int rows, float eps) {
    constexpr int D = NV * 256;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* xr = x + (int64_t)row * D;
    f32x4 v[NV];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        v[i] = *reinterpret_cast<const f32x4*>(xr + (i * 64 + lane) * 4);
        sum += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float mean = wave_sum(sum) * (1.0f / D);
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = v[i][e] - mean;
            sq += d * d;
        }
    const float var = wave_sum(sq) * (1.0f / D);
    const float rstd = 1.0f / sqrtf(var + eps);
    // The row's split3 image (6 D bytes) is assembled in a wave-private LDS buffer and then written as WHOLE lines: 1024 contiguous
    // bytes per store instruction.  Written straight from the registers a lane owns the 8-byte half of every third 16-byte chunk, and
    // such partial-line stores run at 3.8 instead of 6.2 TB/s (scripts/micro/store_patterns.hip, profiles/r4c_store_patterns.jsonl:
    // 24.8 vs 15.2 us for the 94 MB of a 64-crop operand).
    __shared__ __attribute__((aligned(16))) char rowbuf[4][D * 6];
    char* rb = rowbuf[threadIdx.x >> 6];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * 4;
        const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c);
        const f32x4 b = *reinterpret_cast<const f32x4*>(beta + c);
        uint32_t h[4], m[4], l[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float o = (v[i][e] - mean) * rstd * g[e] + b[e];
            h[e] = bf16_rne(o);
            const float r1 = o - __uint_as_float(h[e] << 16);
            m[e] = bf16_rne(r1);
            const float r2 = r1 - __uint_as_float(m[e] << 16);
            l[e] = bf16_rne(r2);
        }
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        char* o8 = rb + (c >> 3) * 48 + (lane & 1) * 8;
        *reinterpret_cast<u32x2*>(o8) = u32x2{h[0] | (h[1] << 16), h[2] | (h[3] << 16)};
        *reinterpret_cast<u32x2*>(o8 + 16) = u32x2{m[0] | (m[1] << 16), m[2] | (m[3] << 16)};
        *reinterpret_cast<u32x2*>(o8 + 32) = u32x2{l[0] | (l[1] << 16), l[2] | (l[3] << 16)};
    }
    // wave-private buffer: the wave's own LDS writes are visible to its reads in program order (no barrier)
    char* yr = y + (int64_t)row * D * 6;
    constexpr int NCH = D * 6 / 16;                      // 16-byte chunks of the row (480)
#pragma unroll
    for (int i = 0; i < (NCH + 63) / 64; ++i) {
        const int ch = i * 64 + lane;
        if (ch < NCH) *reinterpret_cast<u32x4*>(yr + ch * 16) = *reinterpret_cast<const u32x4*>(rb + ch * 16);
    }
}

}  // namespace

int launch_split3(const float* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows, int K, hipStream_t s) {
    if (rows <= 0 || K <= 0 || (K % 8) != 0 || (ld_src % 4) != 0 || (ld_dst % 8) != 0 || ld_dst < K) return -1;
    const int kg = K / 8;
    const int64_t n = rows * kg;
    hipLaunchKernelGGL(split3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, ld_src, reinterpret_cast<char*>(dst), ld_dst,
                       rows, kg);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_layernorm_split3(const float* x, const float* g, const float* b, void* y_split, int rows, int D, float eps, hipStream_t s) {
    if (rows <= 0 || D != 1280) return -1;
    hipLaunchKernelGGL(ln_split3_kernel<5>, dim3((rows + 3) / 4), dim3(256), 0, s, x, g, b, reinterpret_cast<char*>(y_split), rows, eps);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
