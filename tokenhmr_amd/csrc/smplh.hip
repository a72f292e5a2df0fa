// SMPL-H forward as the tokenizer uses it: linear blend skinning over 6890 vertices with a 52-joint chain (22 body joints + 2 x 15 hand
// joints), 459 pose features, and 73 output joints = the 52 posed chain joints + 21 picked vertices (no regressor, no remap).
//
// Replaces the un-vendored smplx `SMPLHLayer.forward` (rotation matrices; tokenization/models/vanilla_pose_vqvae.py:10-17,182-191, the
// decoder's module-level body model) and `SMPLH.forward` (axis-angle; tokenization/dataset/dataset_poseVQ.py:81,111-113, the ground truth), both
// -> `lbs.lbs` + `VertexJointSelector`, restated from their published algorithm (unpinned, smplx is installed nowhere).
//
// Same three launches as lbs.hip (prep, blend GEMM, skin) with what differs for SMPL-H:
//   * J_template (52x3) / J_shapedirs (52x3x10) once in fp64; dirs^T (20670 x 480) = [shapedirs | posedirs | 0]: 10 + 459 = 469 columns,
//     zero-padded to a multiple of the GEMM's 32-deep K tile.
//   * prep, one workgroup per pose: rest joints from the betas, the chain in smplx's formulation (relative transforms in array order,
//     A_j = G_j - [0 | G_j J_j]), the GEMM operand row [betas | (R[1:] - I) | 0], and the 52 posed chain joints written straight into
//     joints 0..51 of the output (nothing is regressed from the vertices, so nothing crosses workgroups and no arrival counter exists).
//   * skin: one thread per vertex, its skinning weights in registers for the whole pass, the pose's bone matrices staged in LDS one pose
//     ahead; the thread that owns one of the 21 selected vertices also writes it to joints 52..72, so those equal the vertex bit for bit.
//   * the FOLDED body-only path (the tokenizer's call: identity hands).  A joint whose local rotation is the identity has its parent's
//     bone matrix — G_i [I | -J_i] = G_p [I | J_i - J_p] [I | -J_i] = G_p [I | -J_p] — so each hand's 15 weight columns are added into
//     its wrist's once at creation (22 columns, padded to 24) and the pose correctives keep only the 21 body joints' 189 features
//     (K = 199 -> 224).  The skin loop reads 66 broadcast float4 per pose instead of 156: the LDS return traffic that lbs.hip's header
//     names as that kernel's bound.  The posed HAND joints come from the wrist's transform applied to their rest position.
#include "common.h"

namespace {

constexpr int NV = 6890, NB = 10;
constexpr int NJH = THMR_SMPLH_NJ, NBODY = THMR_SMPLH_NBODY, NOUT = THMR_SMPLH_NOUT;

// ---- one-time: J_template[j][i], J_shapedirs[j][i][l] in fp64 -> fp32 (as lbs_jreg_kernel) ----
__global__ __launch_bounds__(256) void smplh_jreg_kernel(const float* __restrict__ Jreg, const float* __restrict__ vt,
                                                         const float* __restrict__ sd, float* __restrict__ Jt,
                                                         float* __restrict__ Jsd) {
    __shared__ double red[256];
    const int j = blockIdx.x, q = blockIdx.y;   // q in [0,33): 0..2 template coords, 3.. = 3 + i*10 + l
    double acc = 0.0;
    for (int v = threadIdx.x; v < NV; v += 256) {
        const double w = Jreg[(int64_t)j * NV + v];
        const double val = (q < 3) ? (double)vt[v * 3 + q] : (double)sd[(int64_t)v * 30 + (q - 3)];
        acc += w * val;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (unsigned s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (q < 3) Jt[j * 3 + q] = (float)red[0];
        else Jsd[j * 30 + (q - 3)] = (float)red[0];
    }
}

// ---- one-time: dirs^T[n][k], n = 3*vertex + coordinate: k < 10 shapedirs, 10 <= k < 10 + npf the first npf rows of posedirs, rest 0 ----
__global__ __launch_bounds__(256) void smplh_build_dirs_kernel(const float* __restrict__ sd, const float* __restrict__ pd,
                                                               float* __restrict__ dirsT, int npf, int kx) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)NV * 3 * kx) return;
    const int n = (int)(idx / kx), k = (int)(idx % kx);
    float v = 0.f;
    if (k < NB) v = sd[(int64_t)n * NB + k];                            // shapedirs (6890,3,10) == [n][10]
    else if (k < NB + npf) v = pd[(int64_t)(k - NB) * (NV * 3) + n];    // posedirs (459, 20670)
    dirsT[idx] = v;
}

// ---- one-time: the folded weight table Wf[v][a], a < 24: the columns j with fold[j] == a added in ascending j; columns 22, 23 are 0 ----
__global__ __launch_bounds__(256) void smplh_fold_weights_kernel(const float* __restrict__ W, const int32_t* __restrict__ fold,
                                                                 float* __restrict__ Wf) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= NV * THMR_SMPLH_NBODY_PAD) return;
    const int v = idx / THMR_SMPLH_NBODY_PAD, a = idx % THMR_SMPLH_NBODY_PAD;
    float acc = 0.f;
    for (int j = 0; j < NJH; ++j)
        if (fold[j] == a) acc += W[(int64_t)v * NJH + j];
    Wf[idx] = acc;
}

// ---- per pose: rest joints, kinematic chain over the NC joints of the pose input, bone matrices A (B,NC,12), operand row, joints 0..51.
//      NC = 52: the full path.  NC = 22: the folded path — root + 21 body joints, the hands at rest relative to their wrists. ----
template <int NC, int KX>
__global__ __launch_bounds__(128) void smplh_prep_kernel(const float* __restrict__ rotmat, const float* __restrict__ betas,
                                                         const float* __restrict__ transl, const float* __restrict__ Jt,
                                                         const float* __restrict__ Jsd, const int32_t* __restrict__ parents,
                                                         const int32_t* __restrict__ fold, float* __restrict__ A,
                                                         float* __restrict__ xf, float* __restrict__ joints) {
    __shared__ float J[NJH][3];
    __shared__ float G[NC][12];
    __shared__ float R[NC][9];
    __shared__ float bs[NB];
    const int b = blockIdx.x, t = threadIdx.x;
    for (int i = t; i < NC * 9; i += 128) R[i / 9][i % 9] = rotmat[(int64_t)b * NC * 9 + i];
    if (t < NB) bs[t] = betas ? betas[(int64_t)b * NB + t] : 0.f;
    __syncthreads();
    for (int i = t; i < NJH * 3; i += 128) {
        float v = 0.f;
#pragma unroll
        for (int l = 0; l < NB; ++l) v = fmaf(bs[l], Jsd[i * NB + l], v);
        J[i / 3][i % 3] = Jt[i] + v;
    }
    // blend-shape GEMM operand row: [betas (10) | pose_feature = (R[1:] - I).view((NC - 1) * 9) (smplx lbs.py) | 0 ...]
    for (int i = t; i < KX; i += 128) {
        float v = 0.f;
        if (i < NB) v = bs[i];
        else if (i < NB + (NC - 1) * 9) {
            const int q = i - NB, j = 1 + q / 9, e = q % 9;
            v = R[j][e] - ((e == 0 || e == 4 || e == 8) ? 1.0f : 0.0f);
        }
        xf[(int64_t)b * KX + i] = v;
    }
    __syncthreads();
    // kinematic chain (smplx batch_rigid_transform): G_0 = T_0, G_i = G_parent(i) . T_i,  T_i = [R_i | J_i - J_parent]
    const int r = t / 4, c = t % 4;
    if (t < 12) G[0][t] = (c < 3) ? R[0][r * 3 + c] : J[0][r];
    __syncthreads();
    for (int i = 1; i < NC; ++i) {
        const int p = parents[i];
        if (t < 12) {
            float v;
            if (c < 3) {
                v = G[p][r * 4 + 0] * R[i][0 * 3 + c] + G[p][r * 4 + 1] * R[i][1 * 3 + c] + G[p][r * 4 + 2] * R[i][2 * 3 + c];
            } else {
                const float rx = J[i][0] - J[p][0], ry = J[i][1] - J[p][1], rz = J[i][2] - J[p][2];
                v = G[p][r * 4 + 0] * rx + G[p][r * 4 + 1] * ry + G[p][r * 4 + 2] * rz + G[p][r * 4 + 3];
            }
            G[i][t] = v;
        }
        __syncthreads();
    }
    // A_i = G_i with the rest-pose joint removed: A[:, :3, 3] = G[:, :3, 3] - G[:, :3, :3] . J_i
    for (int i = t; i < NC * 12; i += 128) {
        const int j = i / 12, e = i % 12, rr = e / 4, cc = e % 4;
        float v = G[j][e];
        if (cc == 3) v = v - (G[j][rr * 4 + 0] * J[j][0] + G[j][rr * 4 + 1] * J[j][1] + G[j][rr * 4 + 2] * J[j][2]);
        A[(int64_t)b * NC * 12 + i] = v;
    }
    if (!joints) return;
    // posed chain joints = the translation column of G; a joint outside the chain (folded path: a hand joint, local rotation I) is its
    // wrist's transform applied to the rest offset, G_w . [J_j - J_w; 1]
    for (int i = t; i < NJH * 3; i += 128) {
        const int j = i / 3, k = i % 3;
        float v;
        if (j < NC) v = G[j][k * 4 + 3];
        else {
            const int w = fold[j];
            const float rx = J[j][0] - J[w][0], ry = J[j][1] - J[w][1], rz = J[j][2] - J[w][2];
            v = G[w][k * 4 + 0] * rx + G[w][k * 4 + 1] * ry + G[w][k * 4 + 2] * rz + G[w][k * 4 + 3];
        }
        joints[((int64_t)b * NOUT + j) * 3 + k] = v + (transl ? transl[b * 3 + k] : 0.f);
    }
}

// ---- skinning: T = sum_j W[v][j] * A[b][j] (3x4), out = T . [v_posed; 1] (+ transl) — one thread per vertex, a workgroup owns 256 vertices
//      and walks CG poses, so the NS weights of its vertex stay in registers for the whole pass (NSP = the table's row length, a multiple of
//      4).  The pose's NS bone matrices are staged in LDS (double-buffered, requested one pose ahead) and read as broadcast ds_read_b128. ----
constexpr int SKB = (NV + 255) / 256;     // skin workgroups per pose = 27
template <int NS, int NSP>
__global__ __launch_bounds__(256) void smplh_skin_kernel(const float* __restrict__ vposed, const float* __restrict__ W,
                                                         const float* __restrict__ A, const int32_t* __restrict__ extra,
                                                         const float* __restrict__ transl, float* __restrict__ verts,
                                                         float* __restrict__ joints, int B, int CG) {
    static_assert(NS * 3 <= 256 && NSP % 4 == 0 && NS <= NSP, "one float4 of the bone matrices per thread");
    __shared__ f32x4 AS[2][NS * 3];          // bone matrices of the current / next pose
    const int tid = threadIdx.x, v = blockIdx.x * 256 + tid;
    const bool vok = v < NV;
    const int vv = vok ? v : NV - 1;
    f32x4 wv[NSP / 4];
#pragma unroll
    for (int q = 0; q < NSP / 4; ++q) wv[q] = reinterpret_cast<const f32x4*>(W + (int64_t)vv * NSP)[q];
    unsigned slots = 0;                   // which of the 21 selected-vertex slots pick this thread's vertex (bit k; an id may repeat)
#pragma unroll
    for (int k = 0; k < 21; ++k) slots |= (extra[k] == v && vok) ? 1u << k : 0u;
    const int b0 = blockIdx.y * CG;
    float xn = 0.f, yn = 0.f, zn = 0.f;
    f32x4 an = {0.f, 0.f, 0.f, 0.f};
    if (b0 < B) {
        const float* p = vposed + ((int64_t)b0 * NV + vv) * 3;
        xn = p[0]; yn = p[1]; zn = p[2];
        if (tid < NS * 3) AS[0][tid] = reinterpret_cast<const f32x4*>(A + (int64_t)b0 * NS * 12)[tid];
    }
    for (int c = 0; c < CG; ++c) {
        const int b = b0 + c;             // workgroup-uniform
        if (b >= B) break;
        __syncthreads();                  // AS[c & 1] is complete, and nobody still reads the buffer that is rewritten below
        const float x = xn, y = yn, z = zn;
        const bool more = c + 1 < CG && b + 1 < B;
        if (more) {
            const float* p = vposed + ((int64_t)(b + 1) * NV + vv) * 3;
            xn = p[0]; yn = p[1]; zn = p[2];
            if (tid < NS * 3) an = reinterpret_cast<const f32x4*>(A + (int64_t)(b + 1) * NS * 12)[tid];
        }
        const f32x4* ASc = AS[c & 1];
        f32x4 T0 = {0.f, 0.f, 0.f, 0.f}, T1 = T0, T2 = T0;
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const float w = wv[j >> 2][j & 3];
            T0 += w * ASc[j * 3 + 0];
            T1 += w * ASc[j * 3 + 1];
            T2 += w * ASc[j * 3 + 2];
        }
        float ox = T0[0] * x + T0[1] * y + T0[2] * z + T0[3];
        float oy = T1[0] * x + T1[1] * y + T1[2] * z + T1[3];
        float oz = T2[0] * x + T2[1] * y + T2[2] * z + T2[3];
        if (transl) { ox += transl[b * 3 + 0]; oy += transl[b * 3 + 1]; oz += transl[b * 3 + 2]; }
        if (vok) {
            float* o = verts + ((int64_t)b * NV + v) * 3;
            o[0] = ox; o[1] = oy; o[2] = oz;
        }
        if (joints)
            for (unsigned m = slots; m; m &= m - 1) {
                float* xo = joints + ((int64_t)b * NOUT + NJH + __builtin_ctz(m)) * 3;
                xo[0] = ox; xo[1] = oy; xo[2] = oz;
            }
        if (more && tid < NS * 3) AS[(c + 1) & 1][tid] = an;          // next pose's bone matrices (landed during the skinning)
    }
}

}  // namespace

int launch_smplh_jreg(const float* Jreg, const float* vt, const float* sd, float* Jt, float* Jsd, hipStream_t s) {
    hipLaunchKernelGGL(smplh_jreg_kernel, dim3(NJH, 33), dim3(256), 0, s, Jreg, vt, sd, Jt, Jsd);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_smplh_build_dirs(const float* sd, const float* pd, float* dirsT, int body_only, hipStream_t s) {
    const int kx = body_only ? THMR_SMPLH_KXB : THMR_SMPLH_KX, npf = ((body_only ? NBODY : NJH) - 1) * 9;
    const int64_t total = (int64_t)NV * 3 * kx;
    hipLaunchKernelGGL(smplh_build_dirs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, sd, pd, dirsT, npf, kx);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_smplh_fold_weights(const float* W, const int32_t* fold, float* Wf, hipStream_t s) {
    hipLaunchKernelGGL(smplh_fold_weights_kernel, dim3((NV * THMR_SMPLH_NBODY_PAD + 255) / 256), dim3(256), 0, s, W, fold, Wf);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// poses per skin workgroup: reuse of the per-vertex weights only pays once the grid already fills the chip several times (27 workgroups per
// pose on 256 CUs).  1 below 64 poses, 2 from 64, 4 from 128, 8 from 256: an UNMEASURED adaptation of lbs.hip's rule (B / 32 capped at 8,
// measured for 24 weights per thread) to powers of two; at 52 weights per thread the trade-off may sit elsewhere
int smplh_poses_per_workgroup(int B) { return B >= 256 ? 8 : (B >= 128 ? 4 : (B >= 64 ? 2 : 1)); }

int launch_smplh(const SmplhArgs& a, hipStream_t s) {
    if (!a.rotmat || !a.verts || a.B < 1) return -1;
    const int B = a.B, kx = a.body_only ? THMR_SMPLH_KXB : THMR_SMPLH_KX;
    if (a.body_only)
        hipLaunchKernelGGL((smplh_prep_kernel<NBODY, THMR_SMPLH_KXB>), dim3(B), dim3(128), 0, s, a.rotmat, a.betas, a.transl, a.Jt, a.Jsd,
                           a.parents, a.fold, a.A, a.xf, a.joints);
    else
        hipLaunchKernelGGL((smplh_prep_kernel<NJH, THMR_SMPLH_KX>), dim3(B), dim3(128), 0, s, a.rotmat, a.betas, a.transl, a.Jt, a.Jsd,
                           a.parents, a.fold, a.A, a.xf, a.joints);
    if (hipGetLastError() != hipSuccess) return -2;
    GemmArgs g{};
    g.A = a.xf; g.lda = kx; g.W = a.body_only ? a.dirsT_body : a.dirsT; g.ldw = kx; g.bias = a.vt; g.resid = nullptr; g.ldr = 0;
    g.C = a.vposed; g.ldc = NV * 3; g.M = B; g.N = NV * 3; g.K = kx; g.qscale = 1.f; g.qcols = 0;
    if (int r = launch_gemm(g, EPI_BIAS, -1, s)) return r;
    const int cg = smplh_poses_per_workgroup(B);
    const dim3 grid(SKB, (B + cg - 1) / cg);
    if (a.body_only)
        hipLaunchKernelGGL((smplh_skin_kernel<NBODY, THMR_SMPLH_NBODY_PAD>), grid, dim3(256), 0, s, a.vposed, a.W_body, a.A, a.extra, a.transl,
                           a.verts, a.joints, B, cg);
    else
        hipLaunchKernelGGL((smplh_skin_kernel<NJH, NJH>), grid, dim3(256), 0, s, a.vposed, a.W, a.A, a.extra, a.transl, a.verts, a.joints, B,
                           cg);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
