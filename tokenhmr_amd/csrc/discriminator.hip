// The HMR pose and shape discriminator, forward and the gradient by its INPUTS:
//   Discriminator.forward      tokenhmr/lib/models/discriminator.py:52-99
//   its three uses             tokenhmr/lib/models/tokenhmr.py:357-362 (loss_fake, loss_real), :392-394 (loss_adv)
// All arithmetic is fp32, but for the shape branch (165 multiply-adds per item, accumulated in fp64).  Stateless: the weights are one
// caller-held device block in the layout of DiscWeights (common.h; written once at load by tokenhmr_amd/discriminator.py), so nothing
// here allocates, synchronises or keeps state between calls.
//
// Forward, four launches (five with the loss):
//   (1) disc_front_kernel      one 256-thread workgroup per item: the 9 -> 32 -> 32 per-joint chain (the two 1x1 convs, :72-75) with the
//                              207 pose values and both activation planes in LDS, the 23 per-joint heads (:77-81; one wave per head, a
//                              fixed xor-shuffle tree) and the shape branch (:84-88; one wave, the 10 / 5 / 1 values on its lanes, moved
//                              by shuffles).  Writes out[:, 0..23] and the all-joints operand h (B, 768): element j * 32 + c, and zeros in
//                              the 32 pad columns, EVERY call — the reference flattens channel-major (c * 23 + j, :91); fc1's columns are
//                              permuted to joint-major and padded to K = 768 once, at load, so that the 64-deep K step of the skinny
//                              GEMM divides it and a lane's stores are contiguous.
//   (2, 3) launch_gemm_skinny  736 (768) -> 1024 and 1024 -> 1024 with EPI_BIAS_RELU (:92-95): the weights are streamed once.
//   (4) disc_readout_kernel    one wave per item: 1024 -> 1 (:96) as 4 float4 per lane, out[:, 24], the item's sum of (out - target)^2
//                              over its 25 columns, and — for the backward — d loss / d z2 of the second wide layer.
//   (5) disc_loss_final_kernel one workgroup adds the B partial sums in fp64 in a fixed order and divides by the loss's B (:358,393).
// Backward: the forward above is run again into the workspace (so a backward needs no preceding forward), then
//   (6) launch_gemm_skinny_relu_mask   dZ1 = (dZ2 . W2) masked by a1 > 0: W2 transposed once at load, the mask is the GEMM's epilogue
//   (7) launch_gemm_skinny             dH = dZ1 . W1 (736 columns; W1 transposed at load)
//   (8) disc_front_backward_kernel     one workgroup per item: dH plus the 23 heads' terms (the same h feeds both, :79 and :91), back
//                                      through the two convs with torch's ReLU derivative (zero at z <= 0) -> grad_poses; the shape
//                                      branch's backward on one wave -> grad_betas.
// No float atomics, no arrival counters: every sum has one order, two runs are bit-equal and a captured call replays like the eager one.
// Every workspace word that is read was written by an earlier launch of the same call.
#include "common.h"

namespace {

constexpr int kJ = 23, kC = 32, kH = kJ * kC, kHp = kDiscKpad, kW = 1024, kPose = kJ * 9, kOut = 25;

// the per-joint chain of one item into LDS: P (207) must be loaded and a barrier passed; A1 is complete after the caller's next barrier
__device__ __forceinline__ void front_layer1(const float* w, const float* P, float* A1, int t) {
    for (int e = t; e < kH; e += 256) {
        const int j = e >> 5, c = e & 31;
        float z = w[DiscWeights::conv1_b + c];
#pragma unroll
        for (int i = 0; i < 9; ++i) z = fmaf(w[DiscWeights::conv1_t + i * kC + c], P[j * 9 + i], z);
        A1[e] = fmaxf(z, 0.f);
    }
}

// The shape branch on one wave (every lane runs this; lanes beyond a layer's width carry zeros): -> z1 on lanes 0..9, z2 on lanes 0..4,
// the output on every lane.  Its 165 multiply-adds per item are accumulated in fp64 from the fp32 inputs and weights: column 23 is one
// short, badly conditioned chain per item (10 -> 10 -> 5 -> 1 with cancelling terms), and the loss's gradient multiplies it by (out - 1).
__device__ __forceinline__ double shape_forward(const float* w, const float* betas, int lane, double& z1, double& z2) {
    const int i1 = lane < 10 ? lane : 0, i2 = lane < 5 ? lane : 0;
    z1 = (double)w[DiscWeights::betas_fc1_b + i1];
#pragma unroll
    for (int k = 0; k < 10; ++k) z1 = fma((double)w[DiscWeights::betas_fc1_w + i1 * 10 + k], (double)betas[k], z1);
    const double a1 = (lane < 10 && z1 > 0.0) ? z1 : 0.0;
    z2 = (double)w[DiscWeights::betas_fc2_b + i2];
#pragma unroll
    for (int k = 0; k < 10; ++k) z2 = fma((double)w[DiscWeights::betas_fc2_w + i2 * 10 + k], __shfl(a1, k, 64), z2);
    const double a2 = (lane < 5 && z2 > 0.0) ? z2 : 0.0;
    double o = (double)w[DiscWeights::betas_out_b];
#pragma unroll
    for (int k = 0; k < 5; ++k) o = fma((double)w[DiscWeights::betas_out_w + k], __shfl(a2, k, 64), o);
    return o;
}

__global__ __launch_bounds__(256) void disc_front_kernel(DiscArgs a) {
    __shared__ float P[kPose + 1], A1[kH], A2[kH];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t b = blockIdx.x;
    const float* w = a.w;
    if (t < kPose) P[t] = a.poses[b * a.pose_stride + t];
    __syncthreads();
    front_layer1(w, P, A1, t);
    __syncthreads();
    float* h = a.h + b * kHp;
    for (int e = t; e < kH; e += 256) {
        const int j = e >> 5, c = e & 31;
        float z = w[DiscWeights::conv2_b + c];
#pragma unroll
        for (int k = 0; k < kC; ++k) z = fmaf(w[DiscWeights::conv2_t + k * kC + c], A1[j * kC + k], z);
        const float v = fmaxf(z, 0.f);
        A2[e] = v;
        h[e] = v;
    }
    if (t < kHp - kH) h[kH + t] = 0.f;                  // the K pad of fc1: written every call, never assumed
    __syncthreads();
    // the 23 heads: head j reads ITS joint's 32 channels (pose_out[j], :79)
    for (int j = wave; j < kJ; j += 4) {
        float v = lane < kC ? w[DiscWeights::pose_out_w + j * kC + lane] * A2[j * kC + lane] : 0.f;
        v = wave_sum(v);
        if (lane == 0) a.out[b * kOut + j] = v + w[DiscWeights::pose_out_b + j];
    }
    if (wave == 3) {
        double z1, z2;
        const double o = shape_forward(w, a.betas + b * 10, lane, z1, z2);
        if (lane == 0) a.out[b * kOut + kJ] = (float)o;
    }
}

// one wave per item: out[:, 24], the item's squared distance to the target, dZ2 of the second wide layer
__global__ __launch_bounds__(256) void disc_readout_kernel(DiscArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.B) return;              // whole waves leave: nothing below crosses waves
    const f32x4* row = reinterpret_cast<const f32x4*>(a.a2 + b * kW);
    const f32x4* ow = reinterpret_cast<const f32x4*>(a.w + DiscWeights::out_w);
    f32x4 x[4], wv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { x[i] = row[i * 64 + lane]; wv[i] = ow[i * 64 + lane]; }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) s = fmaf(x[i][r], wv[i][r], s);
    const float o24 = wave_sum(s) + a.w[DiscWeights::out_b];
    if (lane == 0) a.out[b * kOut + kOut - 1] = o24;
    if (a.partial) {
        float d = 0.f;
        if (lane < kOut - 1) d = a.out[b * kOut + lane] - a.target;          // columns 0..23: disc_front_kernel's, an earlier launch
        if (lane == kOut - 1) d = o24 - a.target;
        d = wave_sum(d * d);
        if (lane == 0) a.partial[b] = d;
    }
    if (a.dz2) {
        const float g = a.grad_out ? a.grad_out[b * kOut + kOut - 1] : (2.f * (o24 - a.target)) / a.div;
        f32x4* dz = reinterpret_cast<f32x4*>(a.dz2 + b * kW);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f32x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = x[i][r] > 0.f ? g * wv[i][r] : 0.f;
            dz[i * 64 + lane] = v;
        }
    }
}

// one workgroup: thread t adds items t, t + 256, ... in index order in fp64, then a fixed tree; sum / B of the loss (tokenhmr.py:358,393)
__global__ __launch_bounds__(256) void disc_loss_final_kernel(DiscArgs a) {
    __shared__ double sh[256];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int i = t; i < a.B; i += 256) acc += (double)a.partial[i];
    sh[t] = acc;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    if (t == 0) a.loss[0] = (float)(sh[0] / (double)a.div);
}

__global__ __launch_bounds__(256) void disc_front_backward_kernel(DiscArgs a) {
    __shared__ float P[kPose + 1], A1[kH], D2[kH], D1[kH], G[kJ + 1];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t b = blockIdx.x;
    const float* w = a.w;
    // d loss / d out of the 23 per-joint columns: the caller's, or 2 (out - target) / B
    if (t < kJ) G[t] = a.grad_out ? a.grad_out[b * kOut + t] : (2.f * (a.out[b * kOut + t] - a.target)) / a.div;
    if (a.grad_poses) {
        if (t < kPose) P[t] = a.poses[b * a.pose_stride + t];
        __syncthreads();
        front_layer1(w, P, A1, t);
        __syncthreads();
        // dA2 = the all-joints path + the joint's own head; ReLU's derivative is torch's: zero at z <= 0, i.e. where the output is 0
        const float* h = a.h + b * kHp;
        const float* dh = a.dh + b * kHp;
        for (int e = t; e < kH; e += 256) {
            const int j = e >> 5;
            const float d = dh[e] + G[j] * w[DiscWeights::pose_out_w + e];
            D2[e] = h[e] > 0.f ? d : 0.f;
        }
        __syncthreads();
        for (int e = t; e < kH; e += 256) {
            const int j = e >> 5, k = e & 31;
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < kC; ++c) d = fmaf(D2[j * kC + c], w[DiscWeights::conv2 + c * kC + k], d);
            D1[e] = A1[e] > 0.f ? d : 0.f;
        }
        __syncthreads();
        if (t < kPose) {
            const int j = t / 9, i = t - j * 9;
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < kC; ++c) d = fmaf(D1[j * kC + c], w[DiscWeights::conv1 + c * 9 + i], d);
            a.grad_poses[b * kPose + t] = d;
        }
    } else {
        __syncthreads();               // G
    }
    if (a.grad_betas && wave == 3) {
        // in fp64 like its forward, and — for the loss's own gradient — from the forward's unrounded output
        double z1, z2;
        const double o = shape_forward(w, a.betas + b * 10, lane, z1, z2);
        const double g = a.grad_out ? (double)a.grad_out[b * kOut + kJ] : (2.0 * (o - (double)a.target)) / (double)a.div;
        const int i1 = lane < 10 ? lane : 0, i2 = lane < 5 ? lane : 0;
        const double dz2 = (lane < 5 && z2 > 0.0) ? g * (double)w[DiscWeights::betas_out_w + i2] : 0.0;
        double d1 = 0.0;
#pragma unroll
        for (int m = 0; m < 5; ++m) d1 = fma((double)w[DiscWeights::betas_fc2_w + m * 10 + i1], __shfl(dz2, m, 64), d1);
        const double dz1 = (lane < 10 && z1 > 0.0) ? d1 : 0.0;
        double d0 = 0.0;
#pragma unroll
        for (int i = 0; i < 10; ++i) d0 = fma((double)w[DiscWeights::betas_fc1_w + i * 10 + i1], __shfl(dz1, i, 64), d0);
        if (lane < 10) a.grad_betas[b * 10 + lane] = (float)d0;
    }
}

GemmArgs gemm(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, float* C, int64_t ldc, int M, int N, int K) {
    GemmArgs g{};
    g.A = A; g.W = W; g.bias = bias; g.C = C;
    g.lda = lda; g.ldw = ldw; g.ldc = ldc;
    g.M = M; g.N = N; g.K = K; g.qscale = 1.f;
    return g;
}

}  // namespace

#define DISC_LAUNCHED() do { if (hipGetLastError() != hipSuccess) return -2; } while (0)
#define DISC_OK(call) do { if (int r_ = (call)) return r_; } while (0)

// The forward chain into a.out (and a.loss); `backward`: also what the backward reads (dz2).  a.h, a.a1, a.a2 and a.partial are workspace.
static int disc_forward_chain(const DiscArgs& a, bool wide, bool backward, hipStream_t s) {
    hipLaunchKernelGGL(disc_front_kernel, dim3(a.B), dim3(256), 0, s, a);
    DISC_LAUNCHED();
    if (!wide) return 0;
    DISC_OK(launch_gemm_skinny(gemm(a.h, kHp, a.w + DiscWeights::fc1, kHp, a.w + DiscWeights::fc1_b, a.a1, kW, a.B, kW, kHp), EPI_BIAS_RELU, s));
    DISC_OK(launch_gemm_skinny(gemm(a.a1, kW, a.w + DiscWeights::fc2, kW, a.w + DiscWeights::fc2_b, a.a2, kW, a.B, kW, kW), EPI_BIAS_RELU, s));
    DiscArgs r = a;
    if (!a.loss) r.partial = nullptr;
    if (!backward) r.dz2 = nullptr;
    hipLaunchKernelGGL(disc_readout_kernel, dim3((a.B + 3) / 4), dim3(256), 0, s, r);
    DISC_LAUNCHED();
    if (a.loss) {
        hipLaunchKernelGGL(disc_loss_final_kernel, dim3(1), dim3(256), 0, s, a);
        DISC_LAUNCHED();
    }
    return 0;
}

int launch_disc_forward(const DiscArgs& a, hipStream_t s) {
    if (a.B < 1 || !a.w || !a.poses || !a.betas || !a.out || !a.h || !a.a1 || !a.a2 || (a.loss && !a.partial)) return -1;
    return disc_forward_chain(a, true, false, s);
}

int launch_disc_backward(const DiscArgs& a, hipStream_t s) {
    if (a.B < 1 || !a.w || !a.poses || !a.betas || !a.out || !a.h || !a.a1 || !a.a2 || (a.loss && !a.partial)) return -1;
    if (!a.grad_poses && !a.grad_betas) return -1;
    if (a.grad_poses && (!a.dz2 || !a.dz1 || !a.dh)) return -1;
    // without grad_poses the wide layers are only run for a caller who asked for the output or the loss
    DISC_OK(disc_forward_chain(a, a.grad_poses || a.want_out || a.loss, a.grad_poses != nullptr, s));
    if (a.grad_poses) {
        GemmArgs m = gemm(a.dz2, kW, a.w + DiscWeights::fc2_t, kW, nullptr, a.dz1, kW, a.B, kW, kW);
        m.resid = a.a1; m.ldr = kW;
        DISC_OK(launch_gemm_skinny_relu_mask(m, s));
        DISC_OK(launch_gemm_skinny(gemm(a.dz1, kW, a.w + DiscWeights::fc1_t, kW, nullptr, a.dh, kHp, a.B, kH, kW), EPI_NONE, s));
    }
    hipLaunchKernelGGL(disc_front_backward_kernel, dim3(a.B), dim3(256), 0, s, a);
    DISC_LAUNCHED();
    return 0;
}
