// The finish of the HMR2.0 regressor head (SMPLTransformerDecoderHead, tokenhmr/lib/models/heads/smpl_head.py:56-103, with
// IEF_ITERS = 1 and the zero input token): what follows the stacked read-out of token_out.
//
//   ro (B, ldro)   columns 0..143 decpose(token_out) | 144..153 decshape | 154..156 deccam, bias included (smpl_head.py:82-84)
//   + init_body_pose / init_betas / init_cam          the mean-parameter residual of the single IEF iteration (:64-66,82-84)
//   rot6d_to_rotmat over all 24 joints                geometry.py:64-84: a1 = elements 0..2, a2 = 3..5 of a joint's six values,
//                                                     b1 = F.normalize(a1), b2 = F.normalize(a2 - <b1, a2> b1) (eps 1e-12 on the norm),
//                                                     b3 = b1 x b2, stacked as ROWS; joint 0 is global_orient, 1..23 body_pose (:99-103)
//   pred_cam_t = [cam1, cam2, 2 f / (IMAGE_SIZE cam0 + 1e-9)]                                           tokenhmr.py:165-169
//
// One wave per crop: 2.5 KB in, 1 KB out — the kernel exists to be the ONE launch behind the persistent decoder kernel (and behind the
// skinny read-out GEMM of the launch chain: both forms share it, so they differ only in the read-out's summation order).
#include "common.h"

namespace {

__global__ __launch_bounds__(64) void hmr2_finish_kernel(const float* __restrict__ ro, int ldro, const float* __restrict__ init_pose,
                                                         const float* __restrict__ init_betas, const float* __restrict__ init_cam,
                                                         float* __restrict__ pose6d, float* __restrict__ rotmat, float* __restrict__ betas,
                                                         float* __restrict__ cam, float* __restrict__ cam_t, float* __restrict__ focal,
                                                         float focal_length, float img_size) {
    __shared__ float p6[144];
    const int b = blockIdx.x, t = threadIdx.x;
    const float* r = ro + (int64_t)b * ldro;
    for (int i = t; i < 144; i += 64) {
        const float v = r[i] + init_pose[i];
        p6[i] = v;
        if (pose6d) pose6d[(int64_t)b * 144 + i] = v;
    }
    __syncthreads();
    if (t < 24) {
        const float a1x = p6[t * 6 + 0], a1y = p6[t * 6 + 1], a1z = p6[t * 6 + 2];
        const float a2x = p6[t * 6 + 3], a2y = p6[t * 6 + 4], a2z = p6[t * 6 + 5];
        const float n1 = fmaxf(sqrtf(a1x * a1x + a1y * a1y + a1z * a1z), 1e-12f);   // F.normalize eps
        const float b1x = a1x / n1, b1y = a1y / n1, b1z = a1z / n1;
        const float dp = b1x * a2x + b1y * a2y + b1z * a2z;
        const float ux = a2x - dp * b1x, uy = a2y - dp * b1y, uz = a2z - dp * b1z;
        const float n2 = fmaxf(sqrtf(ux * ux + uy * uy + uz * uz), 1e-12f);
        const float b2x = ux / n2, b2y = uy / n2, b2z = uz / n2;
        const float b3x = b1y * b2z - b1z * b2y, b3y = b1z * b2x - b1x * b2z, b3z = b1x * b2y - b1y * b2x;
        float* R = rotmat + ((int64_t)b * 24 + t) * 9;
        R[0] = b1x; R[1] = b1y; R[2] = b1z;
        R[3] = b2x; R[4] = b2y; R[5] = b2z;
        R[6] = b3x; R[7] = b3y; R[8] = b3z;
    }
    if (t >= 32 && t < 42) betas[(int64_t)b * 10 + (t - 32)] = r[144 + (t - 32)] + init_betas[t - 32];
    if (t == 63) {
        const float c0 = r[154] + init_cam[0], c1 = r[155] + init_cam[1], c2 = r[156] + init_cam[2];
        cam[b * 3 + 0] = c0; cam[b * 3 + 1] = c1; cam[b * 3 + 2] = c2;
        if (cam_t) {
            cam_t[b * 3 + 0] = c1;
            cam_t[b * 3 + 1] = c2;
            cam_t[b * 3 + 2] = (2.0f * focal_length) / (img_size * c0 + 1e-9f);
        }
        if (focal) { focal[b * 2 + 0] = focal_length; focal[b * 2 + 1] = focal_length; }
    }
}

}  // namespace

int launch_hmr2_finish(const float* ro, int ldro, const float* init_pose, const float* init_betas, const float* init_cam, float* pose6d,
                       float* rotmat, float* betas, float* cam, float* cam_t, float* focal, float focal_length, float img_size, int B,
                       hipStream_t s) {
    if (B < 1 || ldro < THMR_HMR2_RO_ROWS || !ro || !rotmat || !betas || !cam) return -1;
    hipLaunchKernelGGL(hmr2_finish_kernel, dim3(B), dim3(64), 0, s, ro, ldro, init_pose, init_betas, init_cam, pose6d, rotmat, betas, cam,
                       cam_t, focal, focal_length, img_size);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
