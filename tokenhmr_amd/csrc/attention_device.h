// The phases of the ViT attention kernels, each stated once (attention.hip: fp32 MFMA; attention_b16.hip: split3 pieces on the bf16 MFMA).
// A kernel is a SCHEDULE — copies, waits, barriers — over these: load_q, s_half, row_max + exp_tiles (softmax_rows), pv_half, store_o_f32 /
// store_o_split3; XcdShare for the kernels that walk items.  Kernels that share a phase run the same instruction sequence per query, which
// is what makes the variants of a family bit-identical.
// Lane (l15 = lane & 15, g = lane >> 4) throughout; tiles are 16 x 16 (v_mfma_f32_16x16x4_f32 operand / result layout).
#pragma once
#include "common.h"

namespace {

constexpr int NTOK = 192, HD = 80, NH = 16, DIM = 1280, QKV_LD = 3840;
constexpr float LOG2E = 1.44269504088896340736f;

inline int launch_status() { return hipGetLastError() == hipSuccess ? 0 : -2; }      // what every launcher returns after its launch

// XCD-aware walk of `nitems` work items by a grid of at most 512 workgroups: workgroup b runs on XCD b % 8 (observed placement, used for
// speed only), XCD x owns the contiguous items [x * per_xcd, (x + 1) * per_xcd) — the 16 heads of a crop stream its 15 KB token rows
// through ONE L2 — and a workgroup takes the items within, within + wpx, ... of its XCD's share.  nitems and the grid are multiples of 8.
struct XcdShare {
    int xcd, within, wpx, per_xcd;
    __device__ __forceinline__ int item(int i) const { return xcd * per_xcd + i; }
};
__device__ __forceinline__ XcdShare xcd_share(int nitems) {
    return XcdShare{(int)(blockIdx.x & 7), (int)(blockIdx.x >> 3), (int)(gridDim.x >> 3), nitems >> 3};
}

// Q fragments of a wave's QT tiles: B operand of S^T = K Q^T.  B[kslot g][j = query l15]; with the k-permutation,
// register qf[qt][j][t] = Q[q0 + 16 qt + l15][16 j + 4 g + t].  `base` = the (crop, head)'s q columns, row stride QKV_LD.
template <int QT>
__device__ __forceinline__ void load_q(f32x4 (&qf)[QT][5], const float* base, int q0, int l15, int g) {
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int j = 0; j < 5; ++j)
            qf[qt][j] = *reinterpret_cast<const f32x4*>(base + (int64_t)(q0 + qt * 16 + l15) * QKV_LD + j * 16 + g * 4);
}

template <int QT, int N>
__device__ __forceinline__ void zero_tiles(f32x4 (&t)[QT][N]) {
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int i = 0; i < N; ++i) t[qt][i] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// S^T tiles of key half hf: s[qt][kt][r] = S[q0 + 16 qt + l15][16 kt + 4 g + r], kt = 6 hf ... 6 hf + 5.  `kh` = the half's 96 K rows in
// LDS, row stride RS floats.  One K fragment read per (kt, j) step feeding 4*QT MFMAs; software-pipelined: the fragment of step i+1 is
// read BEFORE the MFMAs of step i are issued (pinned with sched_barrier; hipcc's own schedule is read -> s_waitcnt lgkmcnt(0) -> MFMAs).
// hf is a literal at every call site.  (vit_attention_kernel states this function in place — a register-allocation matter, see there.)
template <int QT, int RS>
__device__ __forceinline__ void s_half(f32x4 (&s)[QT][12], const f32x4 (&qf)[QT][5], const float* kh, int hf, int l15, int g) {
    f32x4 ka = *reinterpret_cast<const f32x4*>(&kh[l15 * RS + g * 4]);
#pragma unroll
    for (int i = 0; i < 30; ++i) {
        const int kt = hf * 6 + i / 5, j = i % 5;
        f32x4 kn = ka;
        if (i + 1 < 30)
            kn = *reinterpret_cast<const f32x4*>(&kh[(((i + 1) / 5) * 16 + l15) * RS + ((i + 1) % 5) * 16 + g * 4]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int qt = 0; qt < QT; ++qt)
                s[qt][kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[t], qf[qt][j][t], s[qt][kt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        ka = kn;
    }
}

// Maximum of a query's scores over NT tiles: 4 lanes x 4 NT registers per query = in-lane maxima + 2 xor-shuffles.
template <int NT>
__device__ __forceinline__ float row_max(const f32x4 (&s)[NT]) {
    float m = s[0][0];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) m = fmaxf(m, s[kt][r]);
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    return fmaxf(m, __shfl_xor(m, 32, 64));
}

// e_j = 2^(s_j log2e + c), c = -(row maximum) log2e, in place over NT tiles, as ONE packed fma per score PAIR (v_pk_fma_f32) +
// v_exp_f32; the rounding of the constant c is common to the whole row and cancels in e / sum.  Returns the LANE's partial row sum
// (packed adds); the caller adds the other three lanes of the query.  (Round 1: sub, mul, exp, add, mul per score = 1353 non-MFMA VALU
// instructions per wave, profiles/r1_pmc_attention.json; VALU time is matrix-pipe time on gfx950.)
template <int NT>
__device__ __forceinline__ float exp_tiles(f32x4 (&s)[NT], float c) {
    const f32x2 c2 = splat2(c), l2 = splat2(LOG2E);
    f32x2 sum2 = splat2(0.f);
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const f32x2 t = __builtin_elementwise_fma(f32x2{s[kt][2 * h], s[kt][2 * h + 1]}, l2, c2);
            const f32x2 e = f32x2{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
            s[kt][2 * h] = e.x;
            s[kt][2 * h + 1] = e.y;
            sum2 += e;
        }
    return sum2.x + sum2.y;
}

// Softmax over the 192 keys of each query, un-normalised: P.V accumulates e and the 80 outputs of a query are scaled by inv = 1 / sum
// afterwards — 20 multiplies per lane instead of 48.
template <int QT>
__device__ __forceinline__ void softmax_rows(f32x4 (&s)[QT][12], float (&inv)[QT]) {
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const float m = row_max<12>(s[qt]);
        float sum = exp_tiles<12>(s[qt], -(m * LOG2E));
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        inv[qt] = 1.0f / sum;
    }
}

// O^T += V^T P^T over key half hf: A[i = d l15][kslot g] = V[16 kt + 4 g + r][16 dt + l15], B[kslot g][j = query l15] = P register.
// `vh` = the half's 96 V rows in LDS, row stride RS floats.  The transposed product leaves each lane with 4 CONSECUTIVE d of one query
// -> 16-byte output stores.  Pipelined like s_half: the five V values of key step i+1 are read before step i's MFMAs.
template <int QT, int RS>
__device__ __forceinline__ void pv_half(f32x4 (&o)[QT][5], const f32x4 (&s)[QT][12], const float* vh, int hf, int l15, int g) {
    float vc[5], vn[5];
#pragma unroll
    for (int dt = 0; dt < 5; ++dt) vc[dt] = vh[(g * 4) * RS + l15 + dt * 16];
#pragma unroll
    for (int i = 0; i < 24; ++i) {
        const int kt = hf * 6 + i / 4, r = i % 4;
#pragma unroll
        for (int dt = 0; dt < 5; ++dt)
            vn[dt] = (i + 1 < 24) ? vh[(((i + 1) / 4) * 16 + g * 4 + (i + 1) % 4) * RS + l15 + dt * 16] : 0.f;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int dt = 0; dt < 5; ++dt)
#pragma unroll
            for (int qt = 0; qt < QT; ++qt)
                o[qt][dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vc[dt], s[qt][kt][r], o[qt][dt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int dt = 0; dt < 5; ++dt) vc[dt] = vn[dt];
    }
}

// Normalise + store, fp32 output.  D layout of 16x16: col = lane & 15 -> query (the lane that holds this query's 1 / sum),
// row = 4 * (lane >> 4) + reg -> d (one float4 per tile).  `obase` = the (crop, head)'s output columns, row stride DIM.
template <int QT>
__device__ __forceinline__ void store_o_f32(float* obase, int q0, int l15, int g, const f32x4 (&o)[QT][5], const float (&inv)[QT]) {
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int dt = 0; dt < 5; ++dt)
            *reinterpret_cast<f32x4*>(obase + (int64_t)(q0 + qt * 16 + l15) * DIM + dt * 16 + g * 4) = o[qt][dt] * inv[qt];
}

// SPLIT output of a wave's O tiles.  The MFMA leaves lane (l15, g) with 4 consecutive d of query l15 per (qt, dt) tile: columns
// h 80 + 16 dt + 4 g ... + 3 — the 8-byte LOWER half of a split3 chunk group for even g, the upper half for odd g.  Written as such that is
// three 8-byte stores per tile (45 per item; measured 137 vs 102 us per launch at 64 crops, profiles/r3ah_split3_kernel_stats.csv).  Two
// tiles X, Y at a time, v_permlane16_swap exchanges X's odd 16-lane rows with Y's even rows: afterwards an even-g lane holds all 8 columns
// of tile X's group (its own half + its neighbour's) and the odd-g lane next to it all 8 of tile Y's — three 16-byte stores of 48
// contiguous bytes each, 21 + 3 stores per item instead of 45.  The values are the same fp32 numbers, so the pieces are too.
struct SplitPair { int qa, da, qb, db; };
template <int QT>
__device__ __forceinline__ void store_o_split3(char* out, int64_t tok0, int col0, int l15, int g, f32x4 (&o)[QT][5], const float (&inv)[QT]) {
    constexpr int NPAIR = QT == 3 ? 7 : 2 * QT;
    constexpr SplitPair P3[7] = {{0, 0, 0, 1}, {0, 2, 0, 3}, {1, 0, 1, 1}, {1, 2, 1, 3}, {2, 0, 2, 1}, {2, 2, 2, 3}, {0, 4, 1, 4}};
    const bool odd = (g & 1) != 0;
#pragma unroll
    for (int p = 0; p < NPAIR; ++p) {
        const SplitPair pr = QT == 3 ? P3[p] : SplitPair{p / 2, 2 * (p % 2), p / 2, 2 * (p % 2) + 1};
        f32x4 x = o[pr.qa][pr.da] * inv[pr.qa], y = o[pr.qb][pr.db] * inv[pr.qb];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
            const u32x2_t sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(x[j]), __float_as_uint(y[j]), false, false);
            x[j] = __uint_as_float(sw.x);
            y[j] = __uint_as_float(sw.y);
        }
        const int q = odd ? pr.qb : pr.qa, dt = odd ? pr.db : pr.da;
        store_split3_oct(out + (tok0 + q * 16 + l15) * (DIM * 6), col0 + dt * 16 + (g & 2) * 4, x, y);
    }
    // the tile without a partner (QT = 3: (2, 4); otherwise every (qt, 4)): the 8-byte halves
#pragma unroll
    for (int qt = (QT == 3 ? 2 : 0); qt < QT; ++qt)
        store_split3_quad(out + (tok0 + qt * 16 + l15) * (DIM * 6), col0 + 4 * 16 + g * 4, o[qt][4] * inv[qt]);
}
constexpr int kSplitStores3 = 7 * 3 + 3;       // VMEM stores per item of store_o_split3<3> (the persistent kernel counts them: vmcnt)

}  // namespace
