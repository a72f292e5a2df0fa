// The tokenizer round trip (tokenization/models/vanilla_pose_vqvae.py:244-255 VanillaTokenizer.forward): what sits between the encoder's
// latent and the decoder's first convolution, and behind the decoder's pose.
//
//   vq_lookup       QuantizeEMAReset.dequantize (quantize_cnn.py:88-90, F.embedding) written straight as the (B*160, 3*256) conv operand
//                   of decoder.0 — what the soft path's probs @ codebook GEMM writes through its scatter epilogue (GemmArgs::cs_*): row
//                   (b, t) holds taps dk = 0..2, tap dk = the code of position t + dk - 1, zeros outside [0, 160).
//                   plain:            value = c                      (DecodeTokens on hard indices, VanillaTokenizer.decode)
//                   straight-through: value = x + (c - x), fp32, in that order   (quantize_cnn.py:124; differs from c by an ulp on ~6 % of
//                                     the elements — a reference quirk that defines parity)
//                   An index outside [0, 2048) is never read through: it is clamped and *bad_flag (may be null) is set to 1.
//   vq_stats        what QuantizeEMAReset.forward returns beside the codes (quantize_cnn.py:38-47,118-121): the code-usage histogram
//                   (integer atomics: order-independent), commit = mean((x - c[idx])^2), perplexity = exp(-sum p log(p + 1e-7)),
//                   p = count / sum(count).  Both float sums are reduced in a fixed order (per lane over its rows, across the wave by
//                   xor-shuffles, across the workgroup and then across workgroups through a partial-sum array): no float atomics, so two
//                   runs give identical bits.  The histogram is reset by a kernel and the 32 codes of a workgroup are merged before
//                   they reach memory (one atomic per distinct code per workgroup).
//   rotmat_to_aa    matrix_to_axis_angle (rotation_utils.py:428-441 = quaternion_to_axis_angle(matrix_to_quaternion)): the reference's route
//                   step for step (see the kernel), no quaternion standardisation — an angle above pi stays above pi.
#include "common.h"
#include "rotation_device.h"

namespace {

constexpr int kCode = 256, kNCode = 2048, kTok = 160;
constexpr int kStatsRowsPerBlock = 32;      // 4 waves x 8 rows

__device__ __forceinline__ int clamp_code(int c, unsigned* bad_flag) {
    if (c < 0 || c >= kNCode) {
        if (bad_flag) __hip_atomic_store(bad_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        c = c < 0 ? 0 : kNCode - 1;
    }
    return c;
}

// one workgroup per operand row (b, t): 192 lanes x float4 = 3 taps x 256 channels
__global__ __launch_bounds__(192) void vq_lookup_kernel(const int32_t* __restrict__ idx, const float* __restrict__ x,
                                                        const float* __restrict__ cb, float* __restrict__ out, unsigned* bad_flag) {
    const int row = blockIdx.x, t = row % kTok;
    const int dk = threadIdx.x >> 6, n4 = threadIdx.x & 63;
    const int tp = t + dk - 1;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tp >= 0 && tp < kTok) {
        const int64_t src = (int64_t)row + (dk - 1);
        const int c = clamp_code(idx[src], bad_flag);
        v = reinterpret_cast<const float4*>(cb + (int64_t)c * kCode)[n4];
        if (x) {
            const float4 xv = reinterpret_cast<const float4*>(x + src * kCode)[n4];
            v.x = xv.x + (v.x - xv.x); v.y = xv.y + (v.y - xv.y); v.z = xv.z + (v.z - xv.z); v.w = xv.w + (v.w - xv.w);
        }
    }
    reinterpret_cast<float4*>(out + (int64_t)row * (3 * kCode))[threadIdx.x] = v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the histogram's reset as a kernel of its own on the stream (overwrite mode): the statistics then consist of kernel launches only, which a
// captured graph replays in stream order like the eager call (a captured memset in front of the atomics did not: the replay read zeros)
__global__ __launch_bounds__(256) void vq_zero_counts_kernel(int32_t* __restrict__ count) {
    count[blockIdx.x * 256 + threadIdx.x] = 0;
}

// workgroup i: rows [32 i, 32 i + 32), wave w its rows 8 w ... 8 w + 7 one after the other; partial[i] = the workgroup's sum of squares
__global__ __launch_bounds__(256) void vq_stats_rows_kernel(const float* __restrict__ x, const float* __restrict__ cb,
                                                            const int32_t* __restrict__ idx, int rows, int32_t* __restrict__ count,
                                                            float* __restrict__ partial, unsigned* bad_flag) {
    __shared__ float ws[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r0 = (int64_t)blockIdx.x * kStatsRowsPerBlock + wave * 8;
    float acc = 0.f;
    for (int j = 0; j < 8; ++j) {
        const int64_t r = r0 + j;
        if (r >= rows) break;
        const int c = clamp_code(idx[r], nullptr);          // reported by the histogram step below
        const float4 xv = reinterpret_cast<const float4*>(x + r * kCode)[lane];
        const float4 cv = reinterpret_cast<const float4*>(cb + (int64_t)c * kCode)[lane];
        const float d0 = xv.x - cv.x, d1 = xv.y - cv.y, d2 = xv.z - cv.z, d3 = xv.w - cv.w;
        acc += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
    if (wave == 0) {
        // the workgroup's 32 codes, one per lane, merged before they reach memory: the first lane that holds a code adds its multiplicity
        // (a batch that uses few codes would otherwise serialise one atomic per row on a handful of addresses)
        const int64_t r = (int64_t)blockIdx.x * kStatsRowsPerBlock + lane;
        const bool valid = lane < kStatsRowsPerBlock && r < rows;
        const int c = valid ? clamp_code(idx[r], bad_flag) : -1;
        int mult = 0;
        bool first = true;
        for (int j = 0; j < kStatsRowsPerBlock; ++j) {
            const int cj = __shfl(c, j, 64);
            if (cj == c) { ++mult; first = first && j >= lane; }
        }
        if (valid && first) atomicAdd(count + c, mult);
    }
    acc = wave_sum(acc);
    if (lane == 0) ws[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

__device__ __forceinline__ float block_sum256(float v, float* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    const float r = sh[0];
    __syncthreads();
    return r;
}

// one workgroup: the partial sums in index order per lane, then a fixed tree; the histogram's entropy the same way
__global__ __launch_bounds__(256) void vq_stats_final_kernel(const float* __restrict__ partial, int nblk, const int32_t* __restrict__ count,
                                                             int rows, float* __restrict__ commit, float* __restrict__ perplexity) {
    __shared__ float sh[256];
    __shared__ int shi[256];
    const int t = threadIdx.x;
    if (commit) {
        float a = 0.f;
        for (int i = t; i < nblk; i += 256) a += partial[i];
        const float total = block_sum256(a, sh);
        if (t == 0) *commit = total / ((float)rows * (float)kCode);
    }
    if (perplexity) {
        int n = 0;
        for (int k = t; k < kNCode; k += 256) n += count[k];
        shi[t] = n;
        __syncthreads();
        for (int o = 128; o >= 1; o >>= 1) {
            if (t < o) shi[t] += shi[t + o];
            __syncthreads();
        }
        const float total = (float)shi[0];
        float h = 0.f;
        for (int k = t; k < kNCode; k += 256) {
            const float p = (float)count[k] / total;
            h += p * logf(p + 1e-7f);
        }
        const float H = block_sum256(h, sh);
        if (t == 0) *perplexity = expf(-H);
    }
}

// matrix_to_quaternion (rotation_utils.py:104-163) + quaternion_to_axis_angle (:478-506), one lane per matrix: the body is
// rotmat_to_aa_dev (rotation_device.h)
__global__ __launch_bounds__(256) void rotmat_to_aa_kernel(const float* __restrict__ Rm, float* __restrict__ aa, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float ax, ay, az;
    rotmat_to_aa_dev(Rm + (int64_t)i * 9, ax, ay, az);
    aa[(int64_t)i * 3 + 0] = ax;
    aa[(int64_t)i * 3 + 1] = ay;
    aa[(int64_t)i * 3 + 2] = az;
}

}  // namespace

int vq_stats_partials(int rows) { return (rows + kStatsRowsPerBlock - 1) / kStatsRowsPerBlock; }

int launch_vq_lookup(const int32_t* idx, const float* x, const float* cb, float* out, int B, unsigned* bad_flag, hipStream_t s) {
    if (!idx || !cb || !out || B < 1) return -1;
    hipLaunchKernelGGL(vq_lookup_kernel, dim3(B * kTok), dim3(192), 0, s, idx, x, cb, out, bad_flag);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_vq_stats(const float* x, const float* cb, const int32_t* idx, int rows, int32_t* count, int accumulate, float* partial,
                    float* commit, float* perplexity, unsigned* bad_flag, hipStream_t s) {
    if (!x || !cb || !idx || !count || !partial || rows < 1) return -1;
    if (!accumulate) {
        hipLaunchKernelGGL(vq_zero_counts_kernel, dim3(kNCode / 256), dim3(256), 0, s, count);
        if (hipGetLastError() != hipSuccess) return -2;
    }
    const int nblk = vq_stats_partials(rows);
    hipLaunchKernelGGL(vq_stats_rows_kernel, dim3(nblk), dim3(256), 0, s, x, cb, idx, rows, count, partial, bad_flag);
    if (hipGetLastError() != hipSuccess) return -2;
    if (commit || perplexity) {
        hipLaunchKernelGGL(vq_stats_final_kernel, dim3(1), dim3(256), 0, s, partial, nblk, count, rows, commit, perplexity);
        if (hipGetLastError() != hipSuccess) return -2;
    }
    return 0;
}

int launch_rotmat_to_aa(const float* R, float* aa, int n, hipStream_t s) {
    if (!R || !aa || n < 1) return -1;
    hipLaunchKernelGGL(rotmat_to_aa_kernel, dim3((n + 255) / 256), dim3(256), 0, s, R, aa, n);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
