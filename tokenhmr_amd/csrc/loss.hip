// The forward value of the reference's training / validation loss:
//   TokenHMR.compute_loss      tokenhmr/lib/models/tokenhmr.py:190-277  (plain branch :250-262 = validation; LOOSE_SUP branch :214-249)
//   its loss modules           tokenhmr/lib/models/losses.py:36-228 (Keypoint2DLoss / Keypoint3DLoss / ParameterLoss and the *PCKT forms)
//   joint_angle_error          losses.py:22-33
//   TokenLoss                  losses.py:230-252 (CrossEntropyLoss, mean, on whatever matrix it is handed)
//
// val_loss: two launches.  (1) one wave64 per item, four items per 256-thread workgroup: lanes 0..43 own a keypoint, lanes 0..23 a joint,
// lanes 0..9 a beta; the lanes' terms are added by xor-shuffles in a fixed order and lane 0 writes the item's five sums to the workspace
// (and the optional taps).  (2) one workgroup adds the B x 5 partial sums in fp64 (per thread over items t, t + 256, ... in index order,
// then a fixed tree), applies the weights and updates the running sums.  No float atomics, no arrival counter, no LDS in (1); every
// workspace word (2) reads was written by (1) of the same call, so nothing needs zeroing and a captured call replays like the eager one.
//
// The reference writes into the batch (:223, :227, :240); nothing is written into an input here — the written values are the optional
// outputs conf2d_used / conf3d_used / has_betas_used.
//
// Loads: gt_keypoints_3d rows as float4, pred_keypoints_2d rows as float2 (the entry point refuses a base pointer that is not 16- / 8-byte
// aligned); the 12-byte rows ((.,44,3) keypoints, axis-angle) and the 36-byte matrices are 4-byte aligned only and are read as 3- and 9-float
// records the compiler may merge (global_load_dwordx3).  The kernel moves ~3.3 KB per item and is bound by the latency of its dependent
// chain (loads -> cos / sin / atan2 -> shuffles), not by bandwidth.
#include "../../include/tokenhmr_hip.h"      // THMR_RECON_*
#include "common.h"
#include "rotation_device.h"

namespace {

constexpr int kKp = 44, kJoints = 24, kBetas = 10, kTerms = 5;
constexpr int kClasses = 2048;

struct __attribute__((packed, aligned(4))) F3 { float x, y, z; };
struct __attribute__((packed, aligned(4))) F9 { float m[9]; };

// The masks of the LOOSE_SUP branch, written once for the value (val_loss_items_kernel) and for the gradient (val_loss_grad_kernel): both
// evaluate these expressions in this fp32 order, so they cannot disagree about the side of a threshold an entry lies on.
struct KpMask { float err, valid, weak, conf2, conf3; };
__device__ __forceinline__ KpMask loose_kp_mask(float conf2, float conf3, float dx, float dy, float thresh, float v3) {
    KpMask m;
    m.err = conf2 * (dx * dx + dy * dy);                                   // tokenhmr.py:218-219
    m.valid = m.err > thresh ? 1.f : 0.f;                                  // :220
    m.weak = conf2 * (1.f - m.valid);                                      // :221
    m.conf2 = conf2 * m.valid;                                             // :223
    m.conf3 = conf3 * ((v3 + m.conf2) > 0.5f ? 1.f : 0.f);                 // :227
    return m;
}

struct RotMask { float angle, valid, weak; };
__device__ __forceinline__ RotMask loose_rot_mask(const float* P, const float* G, float has, float thresh, float v3) {
    // joint_angle_error (losses.py:22-33): |matrix_to_axis_angle(R_pred R_gt^T)|
    float Rr[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            Rr[i * 3 + k] = fmaf(P[i * 3 + 2], G[k * 3 + 2], fmaf(P[i * 3 + 1], G[k * 3 + 1], P[i * 3 + 0] * G[k * 3 + 0]));
    float ax, ay, az;
    rotmat_to_aa_dev(Rr, ax, ay, az);
    RotMask m;
    m.angle = sqrtf(ax * ax + ay * ay + az * az);
    const float over = m.angle > thresh ? 1.f : 0.f;                       // tokenhmr.py:244
    m.valid = (over * has + v3) != 0.f ? 1.f : 0.f;                        // :245, .bool()
    m.weak = (1.f - m.valid) * has;                                        // :246
    return m;
}

__global__ __launch_bounds__(256) void val_loss_items_kernel(ValLossArgs a) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.B) return;              // whole waves leave: nothing below crosses waves
    const bool loose = a.mode == 1;
    const float lw = a.loose_weight;
    const float v3 = loose ? a.valid_3d[b] : 0.f;

    // ---- keypoints: lane k < 44 ----
    float s2 = 0.f, w2 = 0.f, s3 = 0.f;
    {
        const int k = lane < kKp ? lane : 0;
        const int64_t r = (int64_t)b * kKp + k;
        const float2 p2 = reinterpret_cast<const float2*>(a.pred_kp2d)[r];
        const F3 g2 = reinterpret_cast<const F3*>(a.gt_kp2d)[r];
        const F3 p3 = reinterpret_cast<const F3*>(a.pred_kp3d)[r];
        const float4 g3 = reinterpret_cast<const float4*>(a.gt_kp3d)[r];
        const float dx = p2.x - g2.x, dy = p2.y - g2.y;
        const float l1 = fabsf(dx) + fabsf(dy);
        float conf2 = g2.z;                    // what the 2D loss multiplies with (Keypoint2DLoss, losses.py:61-63)
        float conf3 = g3.w;
        if (loose) {
            const KpMask m = loose_kp_mask(conf2, conf3, dx, dy, a.kp2d_thresh[k], v3);
            conf2 = m.conf2;                                               // :223
            conf3 = m.conf3;                                               // :227
            if (lane < kKp) {
                w2 = m.weak * l1;                                          // losses.py:130
                if (a.kp2d_err) a.kp2d_err[r] = m.err;
                if (a.valid2d) a.valid2d[r] = m.valid;
                if (a.weak2d) a.weak2d[r] = m.weak;
                if (a.conf2d_used) a.conf2d_used[r] = conf2;
                if (a.conf3d_used) a.conf3d_used[r] = conf3;
            }
        }
        // Keypoint3DLoss (losses.py:94-98): both sides relative to their own pelvis
        const float ppx = __shfl(p3.x, a.pelvis_id, 64), ppy = __shfl(p3.y, a.pelvis_id, 64), ppz = __shfl(p3.z, a.pelvis_id, 64);
        const float gpx = __shfl(g3.x, a.pelvis_id, 64), gpy = __shfl(g3.y, a.pelvis_id, 64), gpz = __shfl(g3.z, a.pelvis_id, 64);
        if (lane < kKp) {
            s2 = conf2 * l1;
            s3 = conf3 * ((fabsf((p3.x - ppx) - (g3.x - gpx)) + fabsf((p3.y - ppy) - (g3.y - gpy))) + fabsf((p3.z - ppz) - (g3.z - gpz)));
        }
    }

    // ---- joints: lane j < 24, joint 0 = global_orient ----
    float srot = 0.f, wrot = 0.f;
    {
        const int j = lane < kJoints ? lane : 0;
        const int64_t r = (int64_t)b * kJoints + j;
        const F9 P = reinterpret_cast<const F9*>(a.pred_rotmat)[r];
        float G[9];
        if (a.gt_pose_is_rotmat) {
            const F9 Gm = reinterpret_cast<const F9*>(a.gt_pose)[r];
#pragma unroll
            for (int i = 0; i < 9; ++i) G[i] = Gm.m[i];
        } else {
            const F3 t = reinterpret_cast<const F3*>(a.gt_pose)[r];
            aa_to_rotmat_dev(t.x, t.y, t.z, G);                            // tokenhmr.py:235,260
        }
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const float d = P.m[i] - G[i];
            sq = fmaf(d, d, sq);
        }
        const float has = j == 0 ? a.has_global_orient[b] : a.has_body_pose[b];
        float strong = has * sq, weakv = 0.f;                              // ParameterLoss (losses.py:187-192)
        if (loose) {
            const RotMask m = loose_rot_mask(P.m, G, has, a.angle_thresh[j], v3);
            strong = m.valid * sq;                                         // losses.py:214
            weakv = m.weak * sq;                                           // :218
            if (lane < kJoints) {
                if (a.angle_err) a.angle_err[r] = m.angle;
                if (a.valid_rot) a.valid_rot[r] = m.valid;
                if (a.weak_rot) a.weak_rot[r] = m.weak;
            }
        }
        if (lane < kJoints) { srot = strong; wrot = weakv; }
    }

    // ---- betas: lane i < 10 ----
    float sb = 0.f;
    float hb = a.has_betas[b];
    if (loose) hb = hb * v3;                                               // tokenhmr.py:240
    if (lane < kBetas) {
        const float d = a.pred_betas[(int64_t)b * kBetas + lane] - a.gt_betas[(int64_t)b * kBetas + lane];
        sb = hb * (d * d);
    }

    // ---- the item's five sums: xor-shuffle trees, one order for every call ----
    const float go_s = __shfl(srot, 0, 64), go_w = __shfl(wrot, 0, 64);
    if (lane == 0) { srot = 0.f; wrot = 0.f; }                             // lanes 1..23 are the body pose
    const float t2 = wave_sum(s2), t2w = wave_sum(w2), t3 = wave_sum(s3), tb = wave_sum(srot), tbw = wave_sum(wrot), tbe = wave_sum(sb);
    if (lane == 0) {
        float out[kTerms];
        out[0] = loose ? t2 + lw * t2w : t2;                               // losses.py:128-131
        out[1] = t3;
        out[2] = loose ? go_s + lw * go_w : go_s;                          // losses.py:214-220
        out[3] = loose ? tb + lw * tbw : tb;
        out[4] = tbe;
#pragma unroll
        for (int i = 0; i < kTerms; ++i) {
            a.partial[(int64_t)b * kTerms + i] = out[i];
            if (a.per_item) a.per_item[(int64_t)b * kTerms + i] = out[i];
        }
        if (loose && a.has_betas_used) a.has_betas_used[b] = hb;
    }
}

// one workgroup: thread t adds items t, t + 256, ... in index order in fp64, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void val_loss_final_kernel(ValLossArgs a) {
    __shared__ double sh[kTerms][256];
    const int t = threadIdx.x;
    double acc[kTerms] = {0, 0, 0, 0, 0};
    for (int i = t; i < a.B; i += 256)
#pragma unroll
        for (int c = 0; c < kTerms; ++c) acc[c] += (double)a.partial[(int64_t)i * kTerms + c];
#pragma unroll
    for (int c = 0; c < kTerms; ++c) sh[c][t] = acc[c];
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (t < o)
#pragma unroll
            for (int c = 0; c < kTerms; ++c) sh[c][t] += sh[c][t + o];
        __syncthreads();
    }
    if (t == 0) {
        // tokenhmr.py:264-266: 3D, 2D, then the parameter terms in the dict's order
        const double total = a.w[1] * sh[1][0] + a.w[0] * sh[0][0] + ((a.w[2] * sh[2][0] + a.w[3] * sh[3][0]) + a.w[4] * sh[4][0]);
        const float l[6] = {(float)total, (float)sh[0][0], (float)sh[1][0], (float)sh[2][0], (float)sh[3][0], (float)sh[4][0]};
        if (a.losses)
            for (int i = 0; i < 6; ++i) a.losses[i] = l[i];
        if (a.running) {          // what averaging validation_step_outputs adds up: the fp32 values of every batch
            for (int i = 0; i < 6; ++i) a.running[i] += (double)l[i];
            a.running[6] += 1.0;
        }
    }
}

// ---- the gradient of the same loss: d total / d (pred_keypoints_2d, pred_keypoints_3d, pred_rotmat, pred_betas), and
//      through the projection of forward_step (tokenhmr.py:166-168, 183-185; body_model.hip) d total / d (joints, pred_cam).  The shape of
//      val_loss_items_kernel: one wave64 per item, lanes 0..43 a keypoint, 0..23 a joint, 0..9 a beta; no LDS, no atomics, nothing crosses
//      items, so there is no workspace and no second launch.  The total is a SUM over items: nothing is divided by B.  The masks are
//      constants for the gradient (in the reference they pass through `>` and .bool()) and come from the forward's own functions above.
//      L1 terms carry torch's sign(0) = 0.  A null slot's branch is skipped; every other slot is written in full, zeros included. ----
__device__ __forceinline__ float sign0(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

__global__ __launch_bounds__(256) void val_loss_grad_kernel(ValLossGradArgs g) {
    const ValLossArgs& a = g.in;
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.B) return;              // whole waves leave: nothing below crosses waves
    const bool loose = a.mode == 1;
    const float lw = a.loose_weight;
    const float v3 = loose ? a.valid_3d[b] : 0.f;
    const bool project = g.g_joints || g.g_cam;                            // the entry point refuses either without pred_cam
    const bool want2 = g.g_kp2d || project, want3 = g.g_kp3d || g.g_joints;

    // ---- keypoints: lane k < 44 ----
    if (want2 || want3) {
        const int k = lane < kKp ? lane : 0;
        const int64_t r = (int64_t)b * kKp + k;
        const float2 p2 = reinterpret_cast<const float2*>(a.pred_kp2d)[r];
        const F3 g2 = reinterpret_cast<const F3*>(a.gt_kp2d)[r];
        const F3 p3 = reinterpret_cast<const F3*>(a.pred_kp3d)[r];
        const float4 g3 = reinterpret_cast<const float4*>(a.gt_kp3d)[r];
        const float dx = p2.x - g2.x, dy = p2.y - g2.y;
        float c2 = g2.z, conf3 = g3.w;
        if (loose) {
            const KpMask m = loose_kp_mask(g2.z, g3.w, dx, dy, a.kp2d_thresh[k], v3);
            c2 = m.conf2 + lw * m.weak;                                    // losses.py:128-131: the strong and the weak sum of one |d|
            conf3 = m.conf3;
        }
        // Keypoint2DLoss: w2d c2 sign(pred - gt)
        float gu = 0.f, gv = 0.f;
        if (want2 && lane < kKp) {
            const float s = (float)a.w[0] * c2;
            gu = s * sign0(dx);
            gv = s * sign0(dy);
            if (g.g_kp2d) { g.g_kp2d[r * 2 + 0] = gu; g.g_kp2d[r * 2 + 1] = gv; }
        }
        // Keypoint3DLoss: both sides relative to their own pelvis, so the pelvis row also collects minus every row's term
        float cx = 0.f, cy = 0.f, cz = 0.f;
        if (want3) {
            const float ppx = __shfl(p3.x, a.pelvis_id, 64), ppy = __shfl(p3.y, a.pelvis_id, 64), ppz = __shfl(p3.z, a.pelvis_id, 64);
            const float gpx = __shfl(g3.x, a.pelvis_id, 64), gpy = __shfl(g3.y, a.pelvis_id, 64), gpz = __shfl(g3.z, a.pelvis_id, 64);
            if (lane < kKp) {
                const float s = (float)a.w[1] * conf3;
                cx = s * sign0((p3.x - ppx) - (g3.x - gpx));
                cy = s * sign0((p3.y - ppy) - (g3.y - gpy));
                cz = s * sign0((p3.z - ppz) - (g3.z - gpz));
            }
            const float sx = wave_sum(cx), sy = wave_sum(cy), sz = wave_sum(cz);
            if (lane == a.pelvis_id) { cx -= sx; cy -= sy; cz -= sz; }
            if (g.g_kp3d && lane < kKp) { g.g_kp3d[r * 3 + 0] = cx; g.g_kp3d[r * 3 + 1] = cy; g.g_kp3d[r * 3 + 2] = cz; }
        }
        // the projection's adjoint: X = J + t, t = (cam1, cam2, 2F / (S cam0 + 1e-9)), (u, v) = (F / S) X_xy / X_z; u, v as the loss saw them
        if (project) {
            const float c0 = g.pred_cam[(int64_t)b * 3 + 0];
            const float den = g.img_size * c0 + 1e-9f;
            const float tz = (2.0f * g.focal_length) / den;                // head.hip's cam_t
            const float f = g.focal_length / g.img_size;
            float qx = 0.f, qy = 0.f, qz = 0.f;
            if (lane < kKp) {
                const float xz = p3.z + tz;
                qx = (f * gu) / xz;
                qy = (f * gv) / xz;
                qz = -(gu * p2.x + gv * p2.y) / xz;
                if (g.g_joints) { g.g_joints[r * 3 + 0] = cx + qx; g.g_joints[r * 3 + 1] = cy + qy; g.g_joints[r * 3 + 2] = cz + qz; }
            }
            if (g.g_cam) {
                const float tx = wave_sum(qx), ty = wave_sum(qy), tzs = wave_sum(qz);
                if (lane == 0) {
                    g.g_cam[(int64_t)b * 3 + 0] = tzs * (-(tz * g.img_size) / den);
                    g.g_cam[(int64_t)b * 3 + 1] = tx;
                    g.g_cam[(int64_t)b * 3 + 2] = ty;
                }
            }
        }
    }

    // ---- joints: lane j < 24, joint 0 = global_orient.  ParameterLoss: 2 w m (P - G) ----
    if (g.g_rotmat) {
        const int j = lane < kJoints ? lane : 0;
        const int64_t r = (int64_t)b * kJoints + j;
        const F9 P = reinterpret_cast<const F9*>(a.pred_rotmat)[r];
        float G[9];
        if (a.gt_pose_is_rotmat) {
            const F9 Gm = reinterpret_cast<const F9*>(a.gt_pose)[r];
#pragma unroll
            for (int i = 0; i < 9; ++i) G[i] = Gm.m[i];
        } else {
            const F3 t = reinterpret_cast<const F3*>(a.gt_pose)[r];
            aa_to_rotmat_dev(t.x, t.y, t.z, G);
        }
        const float has = j == 0 ? a.has_global_orient[b] : a.has_body_pose[b];
        float m = has;
        if (loose) {
            const RotMask rm = loose_rot_mask(P.m, G, has, a.angle_thresh[j], v3);
            m = rm.valid + lw * rm.weak;                                   // losses.py:214-220
        }
        const float s = (2.f * (float)(j == 0 ? a.w[2] : a.w[3])) * m;
        if (lane < kJoints) {
#pragma unroll
            for (int i = 0; i < 9; ++i) g.g_rotmat[r * 9 + i] = s * (P.m[i] - G[i]);
        }
    }

    // ---- betas: lane i < 10 ----
    if (g.g_betas && lane < kBetas) {
        float hb = a.has_betas[b];
        if (loose) hb = hb * v3;                                           // tokenhmr.py:240
        const int64_t r = (int64_t)b * kBetas + lane;
        g.g_betas[r] = (2.f * (float)a.w[4] * hb) * (a.pred_betas[r] - a.gt_betas[r]);
    }
}

// CrossEntropyLoss per row of 2048: one wave per row, the row read once as 8 float4 per lane (1 KiB per wave instruction) and kept in
// registers; max, sum of exp(x - max), log — all in one order.  A target outside [0, 2048) is not read through: the row's loss is NaN.
__global__ __launch_bounds__(256) void token_ce_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ target, int rows,
                                                            float* __restrict__ row_loss) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float4* xr = reinterpret_cast<const float4*>(x + row * kClasses);
    float4 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = xr[i * 64 + lane];
    float m = v[0].x;
#pragma unroll
    for (int i = 0; i < 8; ++i) m = fmaxf(fmaxf(fmaxf(m, v[i].x), v[i].y), fmaxf(v[i].z, v[i].w));
    m = wave_max(m);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += (expf(v[i].x - m) + expf(v[i].y - m)) + (expf(v[i].z - m) + expf(v[i].w - m));
    s = wave_sum(s);
    if (lane == 0) {
        const int tg = target[row];
        const bool ok = tg >= 0 && tg < kClasses;
        const float xt = ok ? x[row * kClasses + tg] : 0.f;
        row_loss[row] = ok ? (logf(s) + m) - xt : __builtin_nanf("");
    }
}

__global__ __launch_bounds__(256) void token_ce_final_kernel(const float* __restrict__ row_loss, int rows, float* __restrict__ out) {
    __shared__ double sh[256];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int i = t; i < rows; i += 256) acc += (double)row_loss[i];
    sh[t] = acc;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    if (t == 0) out[0] = (float)(sh[0] / (double)rows);
}

// ---- PoseReConsLoss (tokenization/utils/losses.py:65-131) with the weighted total of train_poseVQ.py:152-156, value and gradient in one
//      call: two launches.  (1) the three terms' elements as one row of workgroups — pose blocks, then mesh blocks, then joint blocks, each
//      workgroup kReconSpan consecutive elements of ONE term, four per thread, coalesced — writes each element's gradient of the TOTAL
//      (its scale w_total w_term / count is known before any sum is) and the workgroup's fp32 partial sum: per thread in element order,
//      xor-shuffles, the four waves in order.  (2) one workgroup adds the partials of each term in fp64 (thread t: partials t, t + 256, ...,
//      then a fixed tree) and writes the three means and the total.  No float atomics; every partial (2) reads was written by (1) of the
//      same call.  Kinds as torch's L1Loss / MSELoss / SmoothL1Loss (beta = 1) with mean reduction and WeightedMSE; at the kinks the
//      gradient is torch's: l1 gives 0 at d = 0, l1_smooth is d below |d| = 1 and sign(d) from it on. ----
constexpr int kReconSpan = 1024;

__device__ __forceinline__ void recon_elem(int kind, float d, float w, float& val, float& grad) {
    if (kind == THMR_RECON_L1) { val = fabsf(d); grad = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }
    else if (kind == THMR_RECON_L1_SMOOTH) {
        const float ad = fabsf(d);
        if (ad < 1.f) { val = 0.5f * d * d; grad = d; }
        else { val = ad - 0.5f; grad = d > 0.f ? 1.f : -1.f; }
    }
    else if (kind == THMR_RECON_WT_L2) { val = w * (d * d); grad = 2.f * (w * d); }
    else { val = d * d; grad = 2.f * d; }
}

__global__ __launch_bounds__(256) void recon_loss_terms_kernel(ReconLossArgs a) {
    __shared__ float ws[4];
    const int tid = threadIdx.x;
    int term = 0, lb = blockIdx.x;
    if (lb >= a.nblk[0]) { lb -= a.nblk[0]; term = 1; }
    if (term == 1 && lb >= a.nblk[1]) { lb -= a.nblk[1]; term = 2; }
    const float* pred = term == 0 ? a.pred_rot : (term == 1 ? a.pred_verts : a.pred_joints);
    const float* gt = term == 0 ? a.gt_rot : (term == 1 ? a.gt_verts : a.gt_joints);
    float* grad = term == 0 ? a.grad_rot : (term == 1 ? a.grad_verts : a.grad_joints);
    const int per_item = term == 0 ? 189 : (term == 1 ? 20670 : THMR_SMPLH_NOUT * 3);
    const int64_t total = (int64_t)a.B * per_item;
    const int kind = a.kind[term];
    const float gs = a.gscale[term];
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < kReconSpan / 256; ++k) {
        const int64_t e = (int64_t)lb * kReconSpan + k * 256 + tid;
        if (e >= total) break;
        const int r = (int)(e % per_item);
        const bool in = term != 2 || (r / 3 >= a.jlo && r / 3 < a.jhi);
        float val = 0.f, g = 0.f;
        if (in) recon_elem(kind, pred[e] - gt[e], (term == 1 && kind == THMR_RECON_WT_L2) ? a.vert_w[r] : 1.f, val, g);
        acc += val;
        if (grad) grad[e] = in ? gs * g : 0.f;
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) ws[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) a.partial[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

__global__ __launch_bounds__(256) void recon_loss_final_kernel(ReconLossArgs a) {
    __shared__ double sh[3][256];
    const int t = threadIdx.x;
    int lo = 0;
    for (int term = 0; term < 3; ++term) {
        double acc = 0.0;
        for (int i = t; i < a.nblk[term]; i += 256) acc += (double)a.partial[lo + i];
        sh[term][t] = acc;
        lo += a.nblk[term];
    }
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (t < o)
#pragma unroll
            for (int c = 0; c < 3; ++c) sh[c][t] += sh[c][t + o];
        __syncthreads();
    }
    if (t == 0) {
        const double lp = sh[0][0] / a.count[0], lm = sh[1][0] / a.count[1], lj = sh[2][0] / a.count[2];
        const double commit = a.commit ? (double)a.commit[0] : 0.0;
        a.losses[0] = (float)lp; a.losses[1] = (float)lm; a.losses[2] = (float)lj;
        a.losses[3] = (float)(a.w[4] * (((a.w[0] * lp + a.w[1] * lm) + a.w[2] * lj) + a.w[3] * commit));      // train_poseVQ.py:152-156
    }
}

}  // namespace

int launch_recon_loss(ReconLossArgs& a, hipStream_t s) {
    if (a.B < 1 || !a.partial || !a.losses) return -1;
    const int per[3] = {189, 20670, THMR_SMPLH_NOUT * 3};
    const float* present[3] = {a.pred_rot, a.pred_verts, a.pred_joints};
    int n = 0;
    for (int i = 0; i < 3; ++i) n += a.nblk[i] = present[i] ? (int)(((int64_t)a.B * per[i] + kReconSpan - 1) / kReconSpan) : 0;      // an absent term: mean 0
    if (n < 1) return -1;
    a.count[0] = (double)a.B * 189; a.count[1] = (double)a.B * 20670; a.count[2] = (double)a.B * (a.jhi - a.jlo) * 3;
    for (int i = 0; i < 3; ++i) a.gscale[i] = (float)(a.w[4] * a.w[i] / a.count[i]);
    hipLaunchKernelGGL(recon_loss_terms_kernel, dim3(n), dim3(256), 0, s, a);
    if (hipGetLastError() != hipSuccess) return -2;
    hipLaunchKernelGGL(recon_loss_final_kernel, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_val_loss(const ValLossArgs& a, hipStream_t s) {
    if (a.B < 1 || !a.partial || a.pelvis_id < 0 || a.pelvis_id >= kKp || (a.mode != 0 && a.mode != 1)) return -1;
    hipLaunchKernelGGL(val_loss_items_kernel, dim3((a.B + 3) / 4), dim3(256), 0, s, a);
    if (hipGetLastError() != hipSuccess) return -2;
    if (a.losses || a.running) {
        hipLaunchKernelGGL(val_loss_final_kernel, dim3(1), dim3(256), 0, s, a);
        if (hipGetLastError() != hipSuccess) return -2;
    }
    return 0;
}

int launch_val_loss_grad(const ValLossGradArgs& g, hipStream_t s) {
    const ValLossArgs& a = g.in;
    if (a.B < 1 || a.pelvis_id < 0 || a.pelvis_id >= kKp || (a.mode != 0 && a.mode != 1)) return -1;
    if (!g.g_kp2d && !g.g_kp3d && !g.g_joints && !g.g_cam && !g.g_rotmat && !g.g_betas) return -1;
    if ((g.g_joints || g.g_cam) && !g.pred_cam) return -1;
    hipLaunchKernelGGL(val_loss_grad_kernel, dim3((a.B + 3) / 4), dim3(256), 0, s, g);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_token_ce(const float* x, const int32_t* target, int rows, float* out, float* row_loss, hipStream_t s) {
    if (!x || !target || !out || !row_loss || rows < 1) return -1;
    hipLaunchKernelGGL(token_ce_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, target, rows, row_loss);
    if (hipGetLastError() != hipSuccess) return -2;
    hipLaunchKernelGGL(token_ce_final_kernel, dim3(1), dim3(256), 0, s, row_loss, rows, out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
