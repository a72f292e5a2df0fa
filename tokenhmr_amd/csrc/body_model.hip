// The two body models, SMPL and SMPL-H: linear blend skinning over 6890 vertices from rotation matrices + betas, in three launches each
// (prep, blend GEMM, skin) that share one set of kernels.
//
// SMPL as TokenHMR uses it: a 24-joint chain, 207 pose features, 44 output joints and their weak-perspective projection.  Replaces
// tokenhmr/lib/models/smpl_wrapper.py:27-41 (SMPL.forward: joint_map remap + J19 regressor) over the un-vendored smplx==0.1.28
// `SMPLLayer.forward(pose2rot=False)` -> `lbs.lbs` (restated from its published algorithm), and
// tokenhmr/lib/utils/geometry.py:86-124 perspective_projection as called at tokenhmr/lib/models/tokenhmr.py:183-187.
// SMPL-H as the tokenizer uses it: a 52-joint chain (22 body joints + 2 x 15 hand joints), 459 pose features, and 73 output joints = the 52
// posed chain joints + 21 picked vertices (no regressor, no remap).  Replaces the un-vendored smplx `SMPLHLayer.forward` (rotation matrices;
// tokenization/models/vanilla_pose_vqvae.py:10-17,182-191) and `SMPLH.forward` (axis-angle; tokenization/dataset/dataset_poseVQ.py:81,
// 111-113, the ground truth), both -> `lbs.lbs` + `VertexJointSelector` (unpinned, smplx is installed nowhere).
//
// SURVEY classes the SMPL stage as HBM-bound (83 KB written per crop; 19.8 MB of constants per batch).  Measured it is NOT: 25 MB in 55 us
// at 64 crops = 0.057 of the HBM peak — three dependent launches (9 + 13 + 29 us) whose time is per-workgroup set-up, the 72 broadcast LDS
// reads of bone matrices per thread and crop, and the serial joint finish (five restructurings measured and not kept,
// HISTORY.md 10.4, 11.8).  Layout decisions:
//   * J = J_regressor . v_shaped is linear in betas, so J_template (NR x 3) and J_shapedirs (NR x 3 x 10) are precomputed once in fp64 at
//     load time: no per-crop reduction over 6890 vertices before the chain.
//   * blend shapes + pose correctives are ONE matrix product: v_posed (B x 20670) = [betas | pose_feature | 0] (B x KX, zero-padded to a
//     multiple of the GEMM's 32-deep K tile: 217 -> 224 for SMPL, 469 -> 480 for SMPL-H) . dirs^T + v_template, with dirs^T (20670 x KX,
//     K-contiguous) built once at load from shapedirs and posedirs.  It runs on the MFMA GEMM (gemm_f32.hip) with the template as the
//     bias epilogue, so the dirs stream is read once per 64-row tile of crops at matrix-core speed (the first version did these 6890*621
//     FMAs per crop on the VALU out of LDS and took 107 us at B = 64).
//   * prep, one workgroup per crop: rest joints from the betas, the chain in smplx's formulation (relative transforms in array order,
//     A_j = G_j - [0 | G_j J_j]) and the GEMM operand row.  SMPL also stores the posed joints for the joint finish and zeroes the crop's
//     arrival counter; SMPL-H writes its 52 posed chain joints straight into joints 0..51 of the output (nothing is regressed from the
//     vertices, so nothing crosses workgroups and no arrival counter exists).
//   * skin: one thread per vertex, several crops per workgroup pass: the vertex's weights (registers) x the crop's bone matrices (LDS,
//     staged one crop ahead) -> 3x4 transform.  SMPL's kernel goes on to regress J19 and its crop group's last workgroup finishes the
//     joints; SMPL-H's thread that owns one of the 21 selected vertices writes it to joints 52..72, so those equal the vertex bit for bit.
//   * every global access is coalesced: consecutive lanes = consecutive vertices (12 B each) on loads and stores.
//   * the FOLDED body-only SMPL-H path (the tokenizer's call: identity hands).  A joint whose local rotation is the identity has its
//     parent's bone matrix — G_i [I | -J_i] = G_p [I | J_i - J_p] [I | -J_i] = G_p [I | -J_p] — so each hand's 15 weight columns are added
//     into its wrist's once at creation (22 columns, padded to 24) and the pose correctives keep only the 21 body joints' 189 features
//     (K = 199 -> 224).  The skin loop reads 66 broadcast float4 per pose instead of 156: the LDS return traffic that is this kernel's
//     bound.  The posed HAND joints come from the wrist's transform applied to their rest position.
//   * the backward of both models (thmr_smpl_backward, thmr_smplh_backward for either path), further down: the forward's prep and blend GEMM
//     recomputed, then skin-backward on SkinLane, the blend GEMM reversed and chain-backward, the mirror of prep — one pair of kernel
//     templates, the model's joint finish under `if constexpr`.
#include "common.h"

namespace {

constexpr int NV = 6890, NB = 10;
constexpr int NJ = 24;                                                                                 // SMPL's chain
constexpr int NJH = THMR_SMPLH_NJ, NBODY = THMR_SMPLH_NBODY, NOUT = THMR_SMPLH_NOUT;                   // SMPL-H's
enum Model { SMPL, SMPLH };

// ---- one-time: J_template[j][i], J_shapedirs[j][i][l] in fp64 -> fp32; one workgroup column per joint ----
__global__ __launch_bounds__(256) void jreg_kernel(const float* __restrict__ Jreg, const float* __restrict__ vt,
                                                   const float* __restrict__ sd, float* __restrict__ Jt, float* __restrict__ Jsd) {
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
__global__ __launch_bounds__(256) void build_dirs_kernel(const float* __restrict__ sd, const float* __restrict__ pd,
                                                         float* __restrict__ dirsT, int npf, int kx) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)NV * 3 * kx) return;
    const int n = (int)(idx / kx), k = (int)(idx % kx);
    float v = 0.f;
    if (k < NB) v = sd[(int64_t)n * NB + k];                            // shapedirs (6890,3,10) == [n][10]
    else if (k < NB + npf) v = pd[(int64_t)(k - NB) * (NV * 3) + n];    // posedirs (npf or more, 20670)
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

// ---- per crop: NR rest joints, kinematic chain over the NC joints of the pose input, bone matrices A (B,NC,12), operand row (B,KX).
//      SMPL (24, 24, 224): also Jtr (B,24,3) and the zeroed arrival counter (transl, fold unused).  SMPL-H: joints 0..51 of the (B,73,3)
//      output (Jtr, cnt unused); NC = 52 the full path, NC = 22 the folded one — root + 21 body joints, the hands at rest relative to
//      their wrists. ----
template <int NR, int NC, int KX, Model M>
__global__ __launch_bounds__(128) void prep_kernel(const float* __restrict__ rotmat, const float* __restrict__ betas,
                                                   const float* __restrict__ transl, const float* __restrict__ Jt,
                                                   const float* __restrict__ Jsd, const int32_t* __restrict__ parents,
                                                   const int32_t* __restrict__ fold, float* __restrict__ A, float* __restrict__ xf,
                                                   float* __restrict__ Jtr, unsigned* __restrict__ cnt, float* __restrict__ joints) {
    __shared__ float J[NR][3];
    __shared__ float G[NC][12];
    __shared__ float R[NC][9];
    __shared__ float bs[NB];
    const int b = blockIdx.x, t = threadIdx.x;
    // arrival counter of this crop's 27 skin workgroups (lbs_skin_joints_kernel): zeroed HERE, by the launch that always precedes
    // them on the stream, so an aborted launch cannot leave a count behind for the next call (round 2: the last arriver re-zeroed it)
    if constexpr (M == SMPL)
        if (t == 0) cnt[b] = 0u;
    for (int i = t; i < NC * 9; i += 128) R[i / 9][i % 9] = rotmat[(int64_t)b * NC * 9 + i];
    if (t < NB) bs[t] = (M == SMPL || betas) ? betas[(int64_t)b * NB + t] : 0.f;      // only SMPL-H takes null betas (= zeros)
    __syncthreads();
    for (int i = t; i < NR * 3; i += 128) {
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
    if constexpr (M == SMPL) {
        if (t < NC * 3) Jtr[(int64_t)b * NC * 3 + t] = G[t / 3][(t % 3) * 4 + 3];
    } else {
        if (!joints) return;
        // posed chain joints = the translation column of G; a joint outside the chain (folded path: a hand joint, local rotation I) is
        // its wrist's transform applied to the rest offset, G_w . [J_j - J_w; 1]
        for (int i = t; i < NR * 3; i += 128) {
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
}

// ---- skinning, the part both models share: T = sum_j W[v][j] * A[b][j] (3x4), out = T . [v_posed; 1] — one thread per vertex, a
//      workgroup owns 256 vertices and walks CG crops, so the NS weights of its vertex stay in registers for the whole pass (NSP = the
//      table's row length, a multiple of 4).  The crop's NS bone matrices are staged in LDS (double-buffered, requested one crop ahead)
//      and read as broadcast ds_read_b128.  A kernel calls begin() once, then per crop: __syncthreads(), skin(), its own tail,
//      publish(). ----
constexpr int SKB = (NV + 255) / 256;     // skin workgroups per crop = 27
template <int NS, int NSP>
struct SkinLane {
    static_assert(NS * 3 <= 256 && NSP % 4 == 0 && NS <= NSP, "one float4 of the bone matrices per thread");
    int tid, v, vv;
    bool vok, more;
    f32x4 wv[NSP / 4];
    unsigned slots;                       // which of the 21 selected-vertex slots pick this thread's vertex (bit k; an id may repeat)
    float xn, yn, zn;                     // the posed vertex of crop c + 1 is requested before crop c is skinned
    f32x4 an;

    __device__ __forceinline__ void begin(f32x4 (*AS)[NS * 3], const float* __restrict__ vposed, const float* __restrict__ W,
                                          const float* __restrict__ A, const int32_t* __restrict__ extra, int b0, int B) {
        tid = threadIdx.x, v = blockIdx.x * 256 + tid;
        vok = v < NV;
        vv = vok ? v : NV - 1;
#pragma unroll
        for (int q = 0; q < NSP / 4; ++q) wv[q] = reinterpret_cast<const f32x4*>(W + (int64_t)vv * NSP)[q];
        slots = 0;
#pragma unroll
        for (int k = 0; k < 21; ++k) slots |= (extra[k] == v && vok) ? 1u << k : 0u;      // 21 scalar loads in one batch, no branches
        xn = 0.f, yn = 0.f, zn = 0.f;
        an = f32x4{0.f, 0.f, 0.f, 0.f};
        if (b0 < B) {
            const float* p = vposed + ((int64_t)b0 * NV + vv) * 3;
            xn = p[0]; yn = p[1]; zn = p[2];
            if (tid < NS * 3) AS[0][tid] = reinterpret_cast<const f32x4*>(A + (int64_t)b0 * NS * 12)[tid];
        }
    }
    // hands out the posed vertex of crop b and requests crop b + 1's vertex and bone matrices
    __device__ __forceinline__ void advance(const float* __restrict__ vposed, const float* __restrict__ A, int c, int b, int B, int CG,
                                            float& x, float& y, float& z) {
        x = xn, y = yn, z = zn;
        more = c + 1 < CG && b + 1 < B;
        if (more) {
            const float* p = vposed + ((int64_t)(b + 1) * NV + vv) * 3;
            xn = p[0]; yn = p[1]; zn = p[2];
            if (tid < NS * 3) an = reinterpret_cast<const f32x4*>(A + (int64_t)(b + 1) * NS * 12)[tid];
        }
    }
    // crop b, the c-th of this pass; the caller's __syncthreads() came first: AS[c & 1] is complete.  The vertex's blended 3x4 transform
    // (rows T0, T1, T2) and its posed rest position: what the forward applies (skin) and the backward transposes (lbs_skin_backward_kernel)
    __device__ __forceinline__ void transform(const f32x4 (*AS)[NS * 3], const float* __restrict__ vposed, const float* __restrict__ A,
                                              int c, int b, int B, int CG, f32x4& T0, f32x4& T1, f32x4& T2, float& x, float& y, float& z) {
        advance(vposed, A, c, b, B, CG, x, y, z);
        // (Round 3 also tried the bone matrices as SCALAR loads — 288 floats into SGPRs, one SGPR operand per FMA, no LDS return
        // traffic: each new crop misses the scalar cache and the 12 dependent s_load round trips per crop made the kernel slower,
        // 161 vs 142 us at 512 crops, profiles/r3b_lbs_scalar_loads.log.)
        const f32x4* ASc = AS[c & 1];
        T0 = f32x4{0.f, 0.f, 0.f, 0.f}, T1 = T0, T2 = T0;
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const float w = wv[j >> 2][j & 3];
            T0 += w * ASc[j * 3 + 0];
            T1 += w * ASc[j * 3 + 1];
            T2 += w * ASc[j * 3 + 2];
        }
    }
    // the same transform with the joint loop rolled, four joints per trip, the weights read again from the table: for a kernel that has no
    // registers left for NS weights and the NS * 3 rows the unrolled loop keeps in flight (the 52-joint skin-backward)
    __device__ __forceinline__ void transform_rolled(const f32x4 (*AS)[NS * 3], const float* __restrict__ vposed, const float* __restrict__ W,
                                                     const float* __restrict__ A, int c, int b, int B, int CG, f32x4& T0, f32x4& T1, f32x4& T2,
                                                     float& x, float& y, float& z) {
        advance(vposed, A, c, b, B, CG, x, y, z);
        const f32x4* ASc = AS[c & 1];
        const f32x4* wr = reinterpret_cast<const f32x4*>(W + (int64_t)vv * NSP);
        T0 = f32x4{0.f, 0.f, 0.f, 0.f}, T1 = T0, T2 = T0;
#pragma unroll 1
        for (int q = 0; q < NS / 4; ++q) {
            const f32x4 w4 = wr[q];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = q * 4 + k;
                T0 += w4[k] * ASc[j * 3 + 0];
                T1 += w4[k] * ASc[j * 3 + 1];
                T2 += w4[k] * ASc[j * 3 + 2];
            }
        }
    }
    __device__ __forceinline__ void skin(const f32x4 (*AS)[NS * 3], const float* __restrict__ vposed, const float* __restrict__ A, int c,
                                         int b, int B, int CG, float& ox, float& oy, float& oz) {
        f32x4 T0, T1, T2;
        float x, y, z;
        transform(AS, vposed, A, c, b, B, CG, T0, T1, T2, x, y, z);
        ox = T0[0] * x + T0[1] * y + T0[2] * z + T0[3];
        oy = T1[0] * x + T1[1] * y + T1[2] * z + T1[3];
        oz = T2[0] * x + T2[1] * y + T2[2] * z + T2[3];
    }
    __device__ __forceinline__ void store(float* __restrict__ verts, int b, float ox, float oy, float oz) const {
        if (vok) {
            float* o = verts + ((int64_t)b * NV + v) * 3;
            o[0] = ox; o[1] = oy; o[2] = oz;
        }
    }
    // next crop's bone matrices (they landed while this crop was worked on)
    __device__ __forceinline__ void publish(f32x4 (*AS)[NS * 3], int c) const {
        if (more && tid < NS * 3) AS[(c + 1) & 1][tid] = an;
    }
};

// ---- SMPL-H: the skinned vertex (+ transl), and the picked vertices straight into joints 52..72 ----
template <int NS, int NSP>
__global__ __launch_bounds__(256) void smplh_skin_kernel(const float* __restrict__ vposed, const float* __restrict__ W,
                                                         const float* __restrict__ A, const int32_t* __restrict__ extra,
                                                         const float* __restrict__ transl, float* __restrict__ verts,
                                                         float* __restrict__ joints, int B, int CG) {
    __shared__ f32x4 AS[2][NS * 3];          // bone matrices of the current / next pose
    SkinLane<NS, NSP> t;
    const int b0 = blockIdx.y * CG;
    t.begin(AS, vposed, W, A, extra, b0, B);
    for (int c = 0; c < CG; ++c) {
        const int b = b0 + c;             // workgroup-uniform
        if (b >= B) break;
        __syncthreads();                  // AS[c & 1] is complete, and nobody still reads the buffer that is rewritten below
        float ox, oy, oz;
        t.skin(AS, vposed, A, c, b, B, CG, ox, oy, oz);
        if (transl) { ox += transl[b * 3 + 0]; oy += transl[b * 3 + 1]; oz += transl[b * 3 + 2]; }
        t.store(verts, b, ox, oy, oz);
        if (joints)
            for (unsigned m = t.slots; m; m &= m - 1) {
                float* xo = joints + ((int64_t)b * NOUT + NJH + __builtin_ctz(m)) * 3;
                xo[0] = ox; xo[1] = oy; xo[2] = oz;
            }
        t.publish(AS, c);
    }
}

// ---- SMPL: skinning + joints in ONE kernel.
//   J19:    (smpl_wrapper.py:38-39 vertices2joints) thread (joint j, vertex group g) of 19 x 12 adds its 22 vertices' products
//           for all three coordinates — the regressor entries come from registers, the skinned vertex is ONE broadcast
//           ds_read_b128 — then 57 threads add the 12 group sums in a fixed order.
//   joints: the LAST of a crop group's 27 workgroups to finish (ONE device-scope arrival per pass) adds the 27 partial sums in
//           block order for each crop of the group, picks the 21 extra vertices (vertex_joint_selector), applies joint_map
//           (smpl_wrapper.py:19-20,32), update_hips (:33-36), appends the 19 regressed joints and projects (geometry.py:86-124).
//           What crosses workgroups (partials, the 21 picked vertices) moves with device-scope stores / loads.
// Round 3 (PMC at 512 crops, profiles/r3a_pmc_lbs_b512.json): the round-2 kernel was LDS-bound, not HBM- or latency-bound —
// every thread re-read the 72 float4 of the bone matrices from LDS per crop and the regression did two ds_read_b32 per FMA:
// ~3700 LDS cycles per workgroup and crop = 83 of its 142 us; it also drained its stores and took one device-scope atomic round
// trip PER CROP.  Here: 22 ds_read_b128 per thread for the regression instead of 128 ds_read_b32, one arrival per pass; the 72
// broadcast reads of the bone matrices stay (their 73 KB of LDS return traffic per wave and crop is what is left of the bound). ----
constexpr int CG_MAX = 8;                 // most crops per workgroup pass (chosen per call: enough workgroups first)
constexpr int RG = 12, RV = 22;           // regression: 12 vertex groups of 22 (the last one: 14) x 19 joints = 228 threads
__global__ __launch_bounds__(256) void lbs_skin_joints_kernel(const float* __restrict__ vposed, const float* __restrict__ W,
                                                              const float* __restrict__ A, const float* __restrict__ J19,
                                                              const float* __restrict__ Jtr, const int32_t* __restrict__ extra,
                                                              const int32_t* __restrict__ jmap, const int32_t* __restrict__ update_hips,
                                                              const float* __restrict__ cam_t, float* __restrict__ verts,
                                                              float* jpart, float* xv, unsigned* cnt, float* __restrict__ joints,
                                                              float* __restrict__ kp2d, float focal_over_size, int B, int CG) {
    __shared__ f32x4 AS[2][NJ * 3];          // bone matrices of the current / next crop
    __shared__ __attribute__((aligned(16))) float outs[256 * 4];     // the crop's skinned vertices of this workgroup (x, y, z, -)
    __shared__ float part[RG][57];
    __shared__ float jo[44][3];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    // regression thread (rj, rg): joint rj, vertices rg*22 .. rg*22+21 of this workgroup's 256; its regressor entries, once
    const int rj = tid % 19, rg = tid / 19;
    float jw[RV];
#pragma unroll
    for (int u = 0; u < RV; ++u) {
        const int lv = rg * RV + u, gv = blockIdx.x * 256 + lv;
        jw[u] = (rg < RG && lv < 256 && gv < NV) ? J19[(int64_t)rj * NV + gv] : 0.f;
    }
    SkinLane<NJ, NJ> t;
    const int b0 = blockIdx.y * CG;
    t.begin(AS, vposed, W, A, extra, b0, B);
    for (int c = 0; c < CG; ++c) {
        const int b = b0 + c;             // wave-uniform
        if (b >= B) break;
        __syncthreads();                  // AS[c & 1] is complete; outs / part of the previous crop are no longer read
        float ox, oy, oz;
        t.skin(AS, vposed, A, c, b, B, CG, ox, oy, oz);
        t.store(verts, b, ox, oy, oz);
        for (unsigned m = t.slots; m; m &= m - 1) {
            float* xo = xv + ((int64_t)b * 21 + __builtin_ctz(m)) * 3;
            st_dev(xo + 0, ox); st_dev(xo + 1, oy); st_dev(xo + 2, oz);
        }
        *reinterpret_cast<f32x4*>(outs + tid * 4) = f32x4{t.vok ? ox : 0.f, t.vok ? oy : 0.f, t.vok ? oz : 0.f, 0.f};
        __syncthreads();
        if (tid < 19 * RG) {
            float sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll
            for (int u = 0; u < RV; ++u) {
                const int lv = min(rg * RV + u, 255);                 // past the end: weight 0
                const f32x4 o = *reinterpret_cast<const f32x4*>(outs + lv * 4);
                sx = fmaf(jw[u], o[0], sx); sy = fmaf(jw[u], o[1], sy); sz = fmaf(jw[u], o[2], sz);
            }
            part[rg][rj * 3 + 0] = sx; part[rg][rj * 3 + 1] = sy; part[rg][rj * 3 + 2] = sz;
        }
        __syncthreads();
        if (tid < 57) {
            float sacc = part[0][tid];
#pragma unroll
            for (int g = 1; g < RG; ++g) sacc += part[g][tid];
            st_dev(jpart + ((int64_t)b * SKB + blockIdx.x) * 57 + tid, sacc);
        }
        t.publish(AS, c);
    }
    // ONE arrival per pass: this workgroup's device-scope stores for all its crops have completed before it counts itself in
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) s_last = __hip_atomic_fetch_add(&cnt[blockIdx.y], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(SKB - 1);
    __syncthreads();
    if (!s_last) return;
    for (int c = 0; c < CG; ++c) {        // all 27 workgroups of this crop group have arrived: finish its crops
        const int b = b0 + c;
        if (b >= B) break;
        if (tid < 57) {                   // J19 regressor: the partial sums of workgroups 0 .. 26 in order
            float sacc = 0.f;
            for (int k = 0; k < SKB; ++k) sacc += ld_dev(jpart + ((int64_t)b * SKB + k) * 57 + tid);
            jo[25 + tid / 3][tid % 3] = sacc;
        }
        if (tid >= 64 && tid < 64 + 75) {
            const int u = tid - 64, j = u / 3, i = u % 3;
            const int src = jmap[j];
            jo[j][i] = (src < NJ) ? Jtr[((int64_t)b * NJ + src) * 3 + i] : ld_dev(xv + ((int64_t)b * 21 + (src - NJ)) * 3 + i);
        }
        __syncthreads();
        // SMPL(update_hips=True), smpl_wrapper.py:33-36, on the 25 mapped joints (before the extra joints are appended):
        //   j[9,12] = (j[9,12] + 0.25*(j[9,12] - j[12,9])) + 0.5*(j[8] - 0.5*(j[9,12] + j[12,9]))
        if (*update_hips && tid < 3) {
            const float a = jo[9][tid], cc = jo[12][tid], m = jo[8][tid];
            jo[9][tid] = (a + 0.25f * (a - cc)) + 0.5f * (m - 0.5f * (a + cc));
            jo[12][tid] = (cc + 0.25f * (cc - a)) + 0.5f * (m - 0.5f * (cc + a));
        }
        __syncthreads();
        if (tid < 132 && joints) joints[(int64_t)b * 132 + tid] = jo[tid / 3][tid % 3];
        if (tid < 44 && kp2d && cam_t) {
            const float px = jo[tid][0] + cam_t[b * 3 + 0], py = jo[tid][1] + cam_t[b * 3 + 1], pz = jo[tid][2] + cam_t[b * 3 + 2];
            kp2d[((int64_t)b * 44 + tid) * 2 + 0] = (px / pz) * focal_over_size;
            kp2d[((int64_t)b * 44 + tid) * 2 + 1] = (py / pz) * focal_over_size;
        }
        __syncthreads();                  // jo is rewritten by the next crop
    }
}

// smplx.lbs.batch_rodrigues (smplx==0.1.28, pose2rot=True path used for GT meshes, image_dataset.py:254-270):
//   angle = ||r + 1e-8||, dir = r / angle, R = I + sin(angle) K + (1 - cos(angle)) K^2,  K = [dir]_x
__global__ void rodrigues_kernel(const float* __restrict__ aa, float* __restrict__ R, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = aa[i * 3 + 0], y = aa[i * 3 + 1], z = aa[i * 3 + 2];
    const float ex = x + 1e-8f, ey = y + 1e-8f, ez = z + 1e-8f;
    const float angle = sqrtf(ex * ex + ey * ey + ez * ez);
    const float rx = x / angle, ry = y / angle, rz = z / angle;
    const float s = sinf(angle), c = cosf(angle), oc = 1.0f - c;
    // K^2 = dir dir^T - I (|dir| = 1 up to the epsilon), written out as smplx's bmm(K, K)
    const float k2[9] = {-(rz * rz) - ry * ry, rx * ry, rx * rz,
                         rx * ry, -(rz * rz) - rx * rx, ry * rz,
                         rx * rz, ry * rz, -(ry * ry) - rx * rx};
    const float k1[9] = {0.f, -rz, ry, rz, 0.f, -rx, -ry, rx, 0.f};
    float* o = R + (int64_t)i * 9;
#pragma unroll
    for (int e = 0; e < 9; ++e) o[e] = ((e == 0 || e == 4 || e == 8) ? 1.0f : 0.0f) + s * k1[e] + oc * k2[e];
}

// ================================================================================================================================
// The vector-Jacobian product of both models (thmr_smpl_backward, thmr_smplh_backward), stated for SMPL; what SMPL-H
// exchanges stands at the two kernels.  Given gV (B,6890,3) and gJ (B,44,3), with the forward's A and
// v_posed recomputed by prep_kernel and the blend GEMM:
//   skin-backward   per vertex  g = gV + sum_k J19[k][v] g19_k + (the mapped joints that pick this vertex),  g_vposed = T[:, :3]^T g,
//                   gT = g (x) [v_posed; 1];  per workgroup  gA_j = sum_v W[v][j] gT_v  (24 x 12, stored per workgroup)
//   blend reverse   gx (B x 224) = g_vposed (B x 20672) . dirs   on the fp32 split-K GEMM, THMR_LBS_GKSPLIT planes
//   chain-backward  per crop: the 27 gA partials in block order, the planes in plane order, the reverse kinematic chain
// Nothing crosses workgroups inside a launch and no floating-point atomic is used: every sum has one fixed order, so a crop's gradient
// is the same bits whatever else is in the batch and however many crops a workgroup pass walks.
// ================================================================================================================================

// ---- one-time: dirsK[k][n] = dirsT[n][k], n < 20670; columns 20670, 20671 (the pad to the GEMM's K tile) zero ----
__global__ __launch_bounds__(256) void build_dirs_k_kernel(const float* __restrict__ dirsT, float* __restrict__ dirsK, int kx) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)kx * THMR_LBS_GK) return;
    const int k = (int)(idx / THMR_LBS_GK), n = (int)(idx % THMR_LBS_GK);
    dirsK[idx] = n < NV * 3 ? dirsT[(int64_t)n * kx + k] : 0.f;
}

// rows of a workgroup's gA partial: the NS bone matrices, and for SMPL-H a row of ones behind them (grad_transl)
constexpr int skin_backward_rows(int ns, Model m) { return ns + (m == SMPLH ? 1 : 0); }

// ---- skin-backward: the forward's grid (27 workgroups of 256 vertices x crop groups, one thread per vertex, SkinLane's registers and
//      LDS staging).  The in-workgroup reduction gA (24 x 12) = W^T (24 x 256) . gT (256 x 12) runs on v_mfma_f32_16x16x4_f32 (exact
//      fp32): each wave owns its 64 vertices as K = 16 steps of 4, two 16-row blocks of joints (24 -> 32), 12 -> 16 columns.  The W^T
//      fragments are constant over the crops of a pass and sit in registers in the MFMA's operand layout (lane l: joint l & 15,
//      vertex 4 step + (l >> 4)), loaded once from global; gT goes through LDS once per crop ([256][12], read conflict-free: the 64 lanes
//      of a step read 48 consecutive floats) — 16 ds_read_b32 and 32 MFMAs per wave and crop, where a VALU reduction out of LDS would read
//      two operands per FMA (288 x 256 FMAs per crop) and wave reductions would take 288 x 6 cross-lane steps per thread.  The four waves'
//      tiles are added in wave order.
//      SMPL-H (M == SMPLH): g = gV + the picked joints 52..72 that are this vertex, nothing else (no regressor, no remap); NSP is the weight
//      table's row length (24 for the folded path's 22 joints).  WREG = false, the 52-joint path's four joint blocks: the W^T fragments do not
//      stay in registers, and the bone-matrix loop is rolled (SkinLane::transform_rolled). ----
template <int NS, int NSP, Model M, bool WREG>
__global__ __launch_bounds__(256) void lbs_skin_backward_kernel(const float* __restrict__ vposed, const float* __restrict__ W,
                                                                const float* __restrict__ A, const float* __restrict__ J19,
                                                                const int32_t* __restrict__ extra, const int32_t* __restrict__ jmap,
                                                                const int32_t* __restrict__ update_hips, const float* __restrict__ gV,
                                                                const float* __restrict__ gJ, float* __restrict__ gvp,
                                                                float* __restrict__ gApart, int B, int CG) {
    // SMPL-H adds one row of ones behind the NS joints: its translation column is sum_v g_v, the vertices' share of grad_transl
    constexpr int NA = skin_backward_rows(NS, M), NBLK = (NA + 15) / 16;
    static_assert(NA <= NBLK * 16 && (WREG ? NBLK == 2 : NS % 4 == 0), "16-row MFMA blocks of joints; two of them fit in registers");
    // SMPL: the 44 output joints, the 25 mapped ones in front of the 19 regressed.  SMPL-H: the 21 picked vertices, joints 52..72
    constexpr int NOJ = M == SMPL ? 44 : 21, NMAP = 25, NREG = M == SMPL ? 19 : 1;
    __shared__ f32x4 AS[2][NS * 3];                   // bone matrices of the current / next crop
    __shared__ float gjs[NOJ * 3];                    // the crop's joint gradients (SMPL: update_hips' adjoint applied)
    __shared__ __attribute__((aligned(16))) float gTs[256 * 12];
    __shared__ float red[4][NA * 12];
    __shared__ float jws[NREG][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    SkinLane<NS, NSP> t;
    const int b0 = blockIdx.y * CG;
    t.begin(AS, vposed, W, A, extra, b0, B);
    // the mapped joints that are this thread's vertex (bit s: joint_map[s] names a picked slot whose vertex id is v; an id may repeat)
    unsigned jslots = 0;
    bool hips = false;
    if constexpr (M == SMPL) {
#pragma unroll
        for (int s = 0; s < NMAP; ++s) {
            const int src = jmap[s];
            jslots |= (src >= NS && ((t.slots >> (src - NS)) & 1u)) ? 1u << s : 0u;
        }
        // the vertex's 19 regressor entries: LDS, not registers (the 24 skin weights and the 32 MFMA fragments already live there across
        // the bone-matrix loop); [k][tid], read conflict-free
        for (int k = 0; k < 19; ++k) jws[k][tid] = t.vok ? J19[(int64_t)k * NV + t.vv] : 0.f;
    } else {
        jslots = t.slots;             // no remap: slot k is joint 52 + k
    }
    // W^T as the MFMA's A operand: step u, lane (i = lane & 15, k = lane >> 4): W[first vertex of the wave + 4 u + k][i (+ 16 ...)]
    float wm[WREG ? 16 : 1][2];
    if constexpr (WREG) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int gv = blockIdx.x * 256 + wave * 64 + u * 4 + (lane >> 4), i = lane & 15;
            wm[u][0] = gv < NV ? W[(int64_t)gv * NSP + i] : 0.f;
            wm[u][1] = (gv < NV && 16 + i < NS) ? W[(int64_t)gv * NSP + 16 + i] : 0.f;
            if constexpr (M == SMPLH)
                if (gv < NV && 16 + i == NS) wm[u][1] = 1.f;
        }
    }
    if constexpr (M == SMPL) hips = *update_hips != 0;
    for (int c = 0; c < CG; ++c) {
        const int b = b0 + c;             // workgroup-uniform
        if (b >= B) break;
        // this thread's element of the crop's joint gradient; the forward is j9' = j9 - j12 / 2 + j8 / 2 (and 12 <-> 9), so
        // (g9, g12, g8) <- (g9 - g12 / 2, g12 - g9 / 2, g8 + (g9 + g12) / 2)
        float gjv = 0.f;
        if (gJ && tid < NOJ * 3) {
            if constexpr (M == SMPL) {
                const float* q = gJ + (int64_t)b * NOJ * 3;
                const int j = tid / 3, i = tid % 3;
                gjv = q[tid];
                if (hips && j == 9) gjv = gjv - 0.5f * q[12 * 3 + i];
                if (hips && j == 12) gjv = gjv - 0.5f * q[9 * 3 + i];
                if (hips && j == 8) gjv = gjv + 0.5f * (q[9 * 3 + i] + q[12 * 3 + i]);
            } else {
                gjv = gJ[((int64_t)b * NOUT + NJH) * 3 + tid];
            }
        }
        __syncthreads();                  // AS[c & 1] is complete; gjs, gTs and red of the previous crop are no longer read
        if (tid < NOJ * 3) gjs[tid] = gjv;
        f32x4 T0, T1, T2;
        float x, y, z;
        if constexpr (WREG) t.transform(AS, vposed, A, c, b, B, CG, T0, T1, T2, x, y, z);
        else t.transform_rolled(AS, vposed, W, A, c, b, B, CG, T0, T1, T2, x, y, z);
        __syncthreads();
        float g0 = 0.f, g1 = 0.f, g2 = 0.f;
        if (gV && t.vok) {
            const float* p = gV + ((int64_t)b * NV + t.v) * 3;
            g0 = p[0]; g1 = p[1]; g2 = p[2];
        }
        if (gJ) {
            if constexpr (M == SMPL) {
#pragma unroll
                for (int k = 0; k < 19; ++k) {
                    const float jw = jws[k][tid];
                    g0 = fmaf(jw, gjs[(NMAP + k) * 3 + 0], g0);
                    g1 = fmaf(jw, gjs[(NMAP + k) * 3 + 1], g1);
                    g2 = fmaf(jw, gjs[(NMAP + k) * 3 + 2], g2);
                }
            }
            for (unsigned m = jslots; m; m &= m - 1) {        // ascending slot order; a vertex named by two slots receives both
                const int s = __builtin_ctz(m);
                g0 += gjs[s * 3 + 0]; g1 += gjs[s * 3 + 1]; g2 += gjs[s * 3 + 2];
            }
        }
        if (!t.vok) g0 = g1 = g2 = 0.f;
        // g_vposed = T[:, :3]^T g, the row padded to THMR_LBS_GK: the thread behind the last vertex writes the two pad columns
        if (t.vok) {
            float* o = gvp + (int64_t)b * THMR_LBS_GK + t.v * 3;
            o[0] = T0[0] * g0 + T1[0] * g1 + T2[0] * g2;
            o[1] = T0[1] * g0 + T1[1] * g1 + T2[1] * g2;
            o[2] = T0[2] * g0 + T1[2] * g1 + T2[2] * g2;
        } else if (t.v == NV) {
            float* o = gvp + (int64_t)b * THMR_LBS_GK + NV * 3;
            o[0] = 0.f; o[1] = 0.f;
        }
        // gT = g (x) [x y z 1], in the bone matrix's own order (row r of 3, column of 4)
        f32x4* gq = reinterpret_cast<f32x4*>(gTs + tid * 12);
        gq[0] = f32x4{g0 * x, g0 * y, g0 * z, g0};
        gq[1] = f32x4{g1 * x, g1 * y, g1 * z, g1};
        gq[2] = f32x4{g2 * x, g2 * y, g2 * z, g2};
        __syncthreads();
        const int n = lane & 15, kq = lane >> 4;
        if constexpr (WREG) {
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const float bv = n < 12 ? gTs[(wave * 64 + u * 4 + kq) * 12 + n] : 0.f;
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wm[u][0], bv, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wm[u][1], bv, acc1, 0, 0, 0);
            }
            // result layout: register r of lane l is row 4 (l >> 4) + r, column l & 15
            if (n < 12) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = kq * 4 + r;
                    red[wave][j * 12 + n] = acc0[r];
                    if (16 + j < NA) red[wave][(16 + j) * 12 + n] = acc1[r];
                }
            }
        } else {
            // more joint blocks than registers hold fragments for: one 16-row block per pass over the gT tile in LDS, its W^T fragments
            // straight from global (the workgroup's 256 rows of W stay in the cache across the crops of a pass)
#pragma unroll 1
            for (int blk = 0; blk < NBLK; ++blk) {
                const float* Wl = W;
                asm volatile("" : "+s"(Wl));      // loads that are the same in every crop are not to be hoisted into 64 registers
                const int row = blk * 16 + n;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int gv = blockIdx.x * 256 + wave * 64 + u * 4 + kq;
                    const float bv = n < 12 ? gTs[(wave * 64 + u * 4 + kq) * 12 + n] : 0.f;
                    float av = (gv < NV && row < NS) ? Wl[(int64_t)gv * NSP + row] : 0.f;
                    if (M == SMPLH && gv < NV && row == NS) av = 1.f;
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
                }
                if (n < 12) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = blk * 16 + kq * 4 + r;
                        if (j < NA) red[wave][j * 12 + n] = acc[r];
                    }
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < NA * 12; i += 256)
            gApart[((int64_t)b * SKB + blockIdx.x) * (NA * 12) + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
        t.publish(AS, c);
    }
}

// ---- chain-backward: one workgroup per crop, the mirror of prep_kernel.  Adds the 27 gA partials in block order and the split-K planes
//      of the blend GEMM's reverse in plane order, recomputes J, R and G as prep_kernel does, and walks the chain from the leaves:
//        gGr_j = gA_j[:, :3] - gA_j[:, 3] (x) J_j,  gGt_j = gA_j[:, 3] + gJtr_j,  gJ_j = -Gr_j^T gA_j[:, 3]
//        i = NC-1 .. 1, p = parent(i), rel = J_i - J_p:  gR_i += Gr_p^T gGr_i;  gGr_p += gGr_i R_i^T + gGt_i (x) rel;
//                                                         gGt_p += gGt_i;  grel = Gr_p^T gGt_i;  gJ_i += grel;  gJ_p -= grel
//        gR_0 += gGr_0,  gJ_0 += gGt_0,  gbeta += sum_{j,i} Jsd[j][i][.] gJ_j[i]
//      (parents[i] < i, as the forward assumes: every child of i has been folded into i before i is read).
//      SMPL (24, 24): the posed joints' gradient arrives through joint_map with update_hips' adjoint.  SMPL-H (NR = 52 rest joints, NC = 52
//      or 22 chain joints): output joint j < 52 IS chain joint j, so gJtr_j = gJo_j.  On the folded path (NC = 22) the forward writes hand
//      joint j >= 22 as Gr_w (J_j - J_w) + Gt_w, w = fold[j] its wrist, whose adjoint, before the chain is walked and in ascending j, is
//        gGr_w += gJo_j (x) (J_j - J_w);  gGt_w += gJo_j;  grel = Gr_w^T gJo_j;  gJ_j += grel;  gJ_w -= grel
//      and reaches the betas through gJ.  grad_transl = the ones row of gA (sum_v g_v, lbs_skin_backward_kernel) + sum_j gJo_j, j ascending. ----
template <int NR, int NC, int KX, int KS, Model M>
__global__ __launch_bounds__(128) void lbs_chain_backward_kernel(const float* __restrict__ rotmat, const float* __restrict__ betas,
                                                                 const float* __restrict__ Jt, const float* __restrict__ Jsd,
                                                                 const int32_t* __restrict__ parents, const int32_t* __restrict__ jmap,
                                                                 const int32_t* __restrict__ update_hips, const int32_t* __restrict__ fold,
                                                                 const float* __restrict__ gJo,
                                                                 const float* __restrict__ gApart, const float* __restrict__ planes,
                                                                 float* __restrict__ grad_rotmat, float* __restrict__ grad_betas,
                                                                 float* __restrict__ grad_transl, int B) {
    constexpr int NMAP = M == SMPL ? 25 : NR, NA = skin_backward_rows(NC, M);      // gm: SMPL the mapped joints', SMPL-H all 52 chain joints'
    static_assert(NC <= NR && (M == SMPLH || NC == NR), "SMPL has no joints outside its chain");
    __shared__ float J[NR][3], R[NC][9], Gr[NC][9], Gt[NC][3], bs[NB];
    __shared__ float gA[NA][12], gx[KX], gm[NMAP][3];
    __shared__ float gGr[NC][9], gGt[NC][3], gJ[NR][3], gR[NC][9];
    const int b = blockIdx.x, t = threadIdx.x;
    for (int i = t; i < NC * 9; i += 128) R[i / 9][i % 9] = rotmat[(int64_t)b * NC * 9 + i];
    if (t < NB) bs[t] = (M == SMPL || betas) ? betas[(int64_t)b * NB + t] : 0.f;      // only SMPL-H takes null betas (= zeros)
    for (int i = t; i < NA * 12; i += 128) {
        float acc = 0.f;      // the loads of a sum are independent and issued together (compile-time counts); the adds keep their order
#pragma unroll
        for (int k = 0; k < SKB; ++k) acc += gApart[((int64_t)b * SKB + k) * (NA * 12) + i];
        gA[i / 12][i % 12] = acc;
    }
    for (int i = t; i < KX; i += 128) {
        float acc = 0.f;
#pragma unroll
        for (int sp = 0; sp < KS; ++sp) acc += planes[((int64_t)sp * B + b) * KX + i];
        gx[i] = acc;
    }
    if constexpr (M == SMPLH) {
        for (int i = t; i < NR * 3; i += 128) gm[i / 3][i % 3] = gJo ? gJo[(int64_t)b * NOUT * 3 + i] : 0.f;
    } else if (t < NMAP * 3) {           // the mapped joints' gradient, update_hips' adjoint applied (as lbs_skin_backward_kernel)
        float v = 0.f;
        if (gJo) {
            const float* q = gJo + (int64_t)b * 132;
            const int j = t / 3, i = t % 3;
            const bool hips = *update_hips != 0;
            v = q[t];
            if (hips && j == 9) v = v - 0.5f * q[12 * 3 + i];
            if (hips && j == 12) v = v - 0.5f * q[9 * 3 + i];
            if (hips && j == 8) v = v + 0.5f * (q[9 * 3 + i] + q[12 * 3 + i]);
        }
        gm[t / 3][t % 3] = v;
    }
    __syncthreads();
    for (int i = t; i < NR * 3; i += 128) {
        float v = 0.f;
#pragma unroll
        for (int l = 0; l < NB; ++l) v = fmaf(bs[l], Jsd[i * NB + l], v);
        J[i / 3][i % 3] = Jt[i] + v;
    }
    __syncthreads();
    // the forward chain, rotation and translation parts apart: Gr_i = Gr_p R_i, Gt_i = Gr_p (J_i - J_p) + Gt_p
    if (t < 9) Gr[0][t] = R[0][t];
    if (t >= 9 && t < 12) Gt[0][t - 9] = J[0][t - 9];
    __syncthreads();
    for (int i = 1; i < NC; ++i) {
        const int p = parents[i];
        if (t < 9) {
            const int r = t / 3, c = t % 3;
            Gr[i][t] = Gr[p][r * 3 + 0] * R[i][0 * 3 + c] + Gr[p][r * 3 + 1] * R[i][1 * 3 + c] + Gr[p][r * 3 + 2] * R[i][2 * 3 + c];
        } else if (t < 12) {
            const int r = t - 9;
            const float rx = J[i][0] - J[p][0], ry = J[i][1] - J[p][1], rz = J[i][2] - J[p][2];
            Gt[i][r] = Gr[p][r * 3 + 0] * rx + Gr[p][r * 3 + 1] * ry + Gr[p][r * 3 + 2] * rz + Gt[p][r];
        }
        __syncthreads();
    }
    // the adjoints of A_j = [Gr_j | Gt_j - Gr_j J_j] and of the posed joints (joint_map slots below NC, in slot order)
    for (int i = t; i < NC * 9; i += 128) {
        const int j = i / 9, r = (i % 9) / 3, c = i % 3;
        gGr[j][i % 9] = gA[j][r * 4 + c] - gA[j][r * 4 + 3] * J[j][c];
        gR[j][i % 9] = (j >= 1 && 10 + (j - 1) * 9 + i % 9 < KX) ? gx[10 + (j - 1) * 9 + i % 9] : 0.f;
    }
    for (int i = t; i < NC * 3; i += 128) {
        const int j = i / 3, r = i % 3;
        float v = gA[j][r * 4 + 3];
        if constexpr (M == SMPLH) v += gm[j][r];
        else
            for (int s = 0; s < NMAP; ++s)
                if (jmap[s] == j) v += gm[s][r];
        gGt[j][r] = v;
        gJ[j][r] = -(Gr[j][0 * 3 + r] * gA[j][0 * 4 + 3] + Gr[j][1 * 3 + r] * gA[j][1 * 4 + 3] + Gr[j][2 * 3 + r] * gA[j][2 * 4 + 3]);
    }
    __syncthreads();
    if constexpr (NC < NR) {                 // the folded path's hand joints: each thread owns one element index of every wrist, no barrier
        for (int j = NC; j < NR; ++j) {
            const int w = fold[j];
            if (t < 9) {
                const int r = t / 3, c = t % 3;
                gGr[w][t] += gm[j][r] * (J[j][c] - J[w][c]);
            } else if (t < 12) {
                gGt[w][t - 9] += gm[j][t - 9];
            } else if (t >= 32 && t < 32 + 3) {
                const int r = t - 32;
                const float grel = Gr[w][0 * 3 + r] * gm[j][0] + Gr[w][1 * 3 + r] * gm[j][1] + Gr[w][2 * 3 + r] * gm[j][2];
                gJ[j][r] = grel;                 // a hand joint's rest position enters nowhere else
                gJ[w][r] -= grel;
            }
        }
        __syncthreads();
    }
    for (int i = NC - 1; i >= 1; --i) {
        const int p = parents[i];
        if (t < 9) {                         // gR_i += Gr_p^T gGr_i
            const int r = t / 3, c = t % 3;
            gR[i][t] += Gr[p][0 * 3 + r] * gGr[i][0 * 3 + c] + Gr[p][1 * 3 + r] * gGr[i][1 * 3 + c] + Gr[p][2 * 3 + r] * gGr[i][2 * 3 + c];
        } else if (t < 18) {                 // gGr_p += gGr_i R_i^T + gGt_i (x) rel
            const int e = t - 9, r = e / 3, c = e % 3;
            gGr[p][e] += (gGr[i][r * 3 + 0] * R[i][c * 3 + 0] + gGr[i][r * 3 + 1] * R[i][c * 3 + 1] + gGr[i][r * 3 + 2] * R[i][c * 3 + 2]) +
                         gGt[i][r] * (J[i][c] - J[p][c]);
        } else if (t < 21) {                 // gGt_p += gGt_i
            gGt[p][t - 18] += gGt[i][t - 18];
        } else if (t < 24) {                 // grel = Gr_p^T gGt_i;  gJ_i += grel;  gJ_p -= grel
            const int r = t - 21;
            const float grel = Gr[p][0 * 3 + r] * gGt[i][0] + Gr[p][1 * 3 + r] * gGt[i][1] + Gr[p][2 * 3 + r] * gGt[i][2];
            gJ[i][r] += grel;
            gJ[p][r] -= grel;
        }
        __syncthreads();
    }
    if (t < 9) gR[0][t] += gGr[0][t];
    if (t >= 9 && t < 12) gJ[0][t - 9] += gGt[0][t - 9];
    __syncthreads();
    if (grad_rotmat)
        for (int i = t; i < NC * 9; i += 128) grad_rotmat[(int64_t)b * NC * 9 + i] = gR[i / 9][i % 9];
    if (grad_betas && t < NB) {
        float v = gx[t];
#pragma unroll
        for (int i = 0; i < NR * 3; ++i) v = fmaf(Jsd[i * NB + t], gJ[i / 3][i % 3], v);
        grad_betas[(int64_t)b * NB + t] = v;
    }
    if constexpr (M == SMPLH) {
        if (grad_transl && t >= 64 && t < 64 + 3) {
            // 6890 + 73 terms of one sign-free sum: the 27 workgroups' fp32 partials and the joints' rows are added in fp64, in order
            // (added in fp32 the 27 partials alone put it at 2.5 times the fp32 reference's distance to float64)
            const int r = t - 64;
            double v = 0.0;
            for (int k = 0; k < SKB; ++k) v += (double)gApart[((int64_t)b * SKB + k) * (NA * 12) + NC * 12 + r * 4 + 3];
            for (int j = 0; j < NR; ++j) v += (double)gm[j][r];
            grad_transl[(int64_t)b * 3 + r] = (float)v;
        }
    }
}

// the adjoint of rodrigues_kernel's own formula: e = r + 1e-8, a = |e|, d = r / a, R = I + sin a K(d) + (1 - cos a) (d d^T - |d|^2 I).
// 1 - cos a is evaluated as 2 sin^2(a / 2): in fp32 the plain form has lost every digit below a ~ 3e-4 rad
__global__ void rodrigues_backward_kernel(const float* __restrict__ aa, const float* __restrict__ gR, float* __restrict__ gaa, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = aa[i * 3 + 0], y = aa[i * 3 + 1], z = aa[i * 3 + 2];
    const float ex = x + 1e-8f, ey = y + 1e-8f, ez = z + 1e-8f;
    const float a = sqrtf(ex * ex + ey * ey + ez * ez);
    const float dx = x / a, dy = y / a, dz = z / a;
    const float s = sinf(a), c = cosf(a), sh = sinf(0.5f * a), oc = 2.0f * sh * sh;
    const float* G = gR + (int64_t)i * 9;
    const float g00 = G[0], g01 = G[1], g02 = G[2], g10 = G[3], g11 = G[4], g12 = G[5], g20 = G[6], g21 = G[7], g22 = G[8];
    const float wx = g21 - g12, wy = g02 - g20, wz = g10 - g01;         // sum(G o K(d)) = w . d
    const float tr = g00 + g11 + g22;
    const float sx = (g00 + g00) * dx + (g01 + g10) * dy + (g02 + g20) * dz;   // (G + G^T) d
    const float sy = (g10 + g01) * dx + (g11 + g11) * dy + (g12 + g21) * dz;
    const float sz = (g20 + g02) * dx + (g21 + g12) * dy + (g22 + g22) * dz;
    const float dd = dx * dx + dy * dy + dz * dz;
    const float gs = wx * dx + wy * dy + wz * dz;
    const float goc = 0.5f * (sx * dx + sy * dy + sz * dz) - dd * tr;    // d^T G d - |d|^2 tr G
    const float gdx = s * wx + oc * (sx - 2.0f * tr * dx), gdy = s * wy + oc * (sy - 2.0f * tr * dy), gdz = s * wz + oc * (sz - 2.0f * tr * dz);
    const float ga = (gs * c + goc * s) - (gdx * x + gdy * y + gdz * z) / (a * a);
    gaa[i * 3 + 0] = gdx / a + ga * (ex / a);
    gaa[i * 3 + 1] = gdy / a + ga * (ey / a);
    gaa[i * 3 + 2] = gdz / a + ga * (ez / a);
}

// v_posed (B x 20670) = xf (B x kx) . dirs^T + v_template
int launch_blend(const float* xf, const float* dirsT, const float* vt, float* vposed, int B, int kx, hipStream_t s) {
    GemmArgs g{};
    g.A = xf; g.lda = kx; g.W = dirsT; g.ldw = kx; g.bias = vt; g.resid = nullptr; g.ldr = 0;
    g.C = vposed; g.ldc = NV * 3; g.M = B; g.N = NV * 3; g.K = kx; g.qscale = 1.f; g.qcols = 0;
    return launch_gemm(g, EPI_BIAS, -1, s);
}

// poses per SMPL-H skin workgroup: reuse of the per-vertex weights only pays once the grid already fills the chip several times (27
// workgroups per pose on 256 CUs).  1 below 64 poses, 2 from 64, 4 from 128, 8 from 256: an UNMEASURED adaptation of SMPL's rule in
// launch_lbs (B / 32 capped at 8, measured for 24 weights per thread) to powers of two; at 52 weights per thread the trade-off may sit
// elsewhere
int smplh_poses_per_workgroup(int B) { return B >= 256 ? 8 : (B >= 128 ? 4 : (B >= 64 ? 2 : 1)); }

// crops per SMPL skin workgroup pass, forward and backward: reuse of the per-vertex constants only pays once the grid already fills the
// chip several times (64 crops: 2 -> 864 workgroups; 256 crops and up: 8)
int lbs_crops_per_pass(int B) { return B >= 32 * CG_MAX ? CG_MAX : (B >= 32 ? B / 32 : 1); }

void launch_lbs_prep(const LbsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((prep_kernel<NJ, NJ, THMR_LBS_KX, SMPL>), dim3(a.B), dim3(128), 0, s, a.rotmat, a.betas, nullptr, a.Jt, a.Jsd, a.parents,
                       nullptr, a.A, a.xf, a.Jtr, a.cnt, nullptr);
}

// prep -> blend GEMM (the forward's, recomputed) -> skin-backward -> blend GEMM reversed -> chain-backward: five launches, SMPL's and either
// SMPL-H path's alike.  `a` is LbsArgs or SmplhArgs; what only one model or path has comes as an argument, null for the other.  cg: crops per
// skin workgroup, the forward's rule
template <int NR, int NC, int NSP, int KX, Model M, bool WREG, class Args>
int launch_body_backward(const Args& a, const BodyGradArgs& g, const float* W, const float* dirsT, const float* J19, const int32_t* jmap,
                         const int32_t* update_hips, const int32_t* fold, float* Jtr, unsigned* cnt, const float* transl, int cg, hipStream_t s) {
    const int B = a.B;
    hipLaunchKernelGGL((prep_kernel<NR, NC, KX, M>), dim3(B), dim3(128), 0, s, a.rotmat, a.betas, transl, a.Jt, a.Jsd, a.parents, fold, a.A, a.xf,
                       Jtr, cnt, nullptr);
    if (hipGetLastError() != hipSuccess) return -2;
    if (int r = launch_blend(a.xf, dirsT, a.vt, a.vposed, B, KX, s)) return r;
    hipLaunchKernelGGL((lbs_skin_backward_kernel<NC, NSP, M, WREG>), dim3(SKB, (B + cg - 1) / cg), dim3(256), 0, s, a.vposed, W, a.A, J19, a.extra,
                       jmap, update_hips, g.gV, g.gJ, g.gvp, g.gApart, B, cg);
    if (hipGetLastError() != hipSuccess) return -2;
    // gx (B x KX) = g_vposed (B x 20672) . dirsK^T: M = B is skinny and N = 224 / 480 is two / four tiles, so K is split THMR_LBS_GKSPLIT = 38
    // ways (544 = 17 K tiles per slice) to put 76 / 152 workgroups per 64 crops on the chip; ONE tile shape (64 x 128) at every batch size,
    // so no dispatch switch exists between sizes (every shape sums a slice's K in the same order anyway, gemm_f32.hip)
    GemmArgs ga{};
    ga.A = g.gvp; ga.lda = THMR_LBS_GK; ga.W = g.dirsK; ga.ldw = THMR_LBS_GK; ga.M = B; ga.N = KX; ga.K = THMR_LBS_GK;
    ga.qscale = 1.f;
    if (int r = launch_gemm_splitk(ga, 12, THMR_LBS_GKSPLIT, g.planes, s)) return r;
    hipLaunchKernelGGL((lbs_chain_backward_kernel<NR, NC, KX, THMR_LBS_GKSPLIT, M>), dim3(B), dim3(128), 0, s, a.rotmat, a.betas, a.Jt, a.Jsd,
                       a.parents, jmap, update_hips, fold, g.gJ, g.gApart, g.planes, g.grad_rotmat, g.grad_betas, g.grad_transl, B);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

int launch_body_build_dirs_k(const float* dirsT, float* dirsK, int kx, hipStream_t s) {
    const int64_t total = (int64_t)kx * THMR_LBS_GK;
    hipLaunchKernelGGL(build_dirs_k_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, dirsT, dirsK, kx);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_rodrigues_backward(const float* aa, const float* gR, float* gaa, int n, hipStream_t s) {
    hipLaunchKernelGGL(rodrigues_backward_kernel, dim3((n + 255) / 256), dim3(256), 0, s, aa, gR, gaa, n);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_lbs_backward(const LbsArgs& a, const BodyGradArgs& g, hipStream_t s) {
    if (a.B < 1 || (!g.gV && !g.gJ) || (!g.grad_rotmat && !g.grad_betas)) return -1;
    return launch_body_backward<NJ, NJ, NJ, THMR_LBS_KX, SMPL, true>(a, g, a.W, a.dirsT, a.J19, a.jmap, a.update_hips, nullptr, a.Jtr, a.cnt, nullptr,
                                                                     lbs_crops_per_pass(a.B), s);
}

int launch_smplh_backward(const SmplhArgs& a, const BodyGradArgs& g, hipStream_t s) {
    if (!a.rotmat || a.B < 1 || (!g.gV && !g.gJ) || (!g.grad_rotmat && !g.grad_betas && !g.grad_transl)) return -1;
    const int cg = smplh_poses_per_workgroup(a.B);
    if (a.body_only)
        return launch_body_backward<NJH, NBODY, THMR_SMPLH_NBODY_PAD, THMR_SMPLH_KXB, SMPLH, true>(a, g, a.W_body, a.dirsT_body, nullptr, nullptr, nullptr,
                                                                                                   a.fold, nullptr, nullptr, a.transl, cg, s);
    return launch_body_backward<NJH, NJH, NJH, THMR_SMPLH_KX, SMPLH, false>(a, g, a.W, a.dirsT, nullptr, nullptr, nullptr, a.fold, nullptr, nullptr,
                                                                            a.transl, cg, s);
}

int launch_rodrigues(const float* aa, float* R, int n, hipStream_t s) {
    hipLaunchKernelGGL(rodrigues_kernel, dim3((n + 255) / 256), dim3(256), 0, s, aa, R, n);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_body_jreg(const float* Jreg, const float* vt, const float* sd, float* Jt, float* Jsd, int nj, hipStream_t s) {
    hipLaunchKernelGGL(jreg_kernel, dim3(nj, 33), dim3(256), 0, s, Jreg, vt, sd, Jt, Jsd);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_body_build_dirs(const float* sd, const float* pd, float* dirsT, int npf, int kx, hipStream_t s) {
    const int64_t total = (int64_t)NV * 3 * kx;
    hipLaunchKernelGGL(build_dirs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, sd, pd, dirsT, npf, kx);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_smplh_fold_weights(const float* W, const int32_t* fold, float* Wf, hipStream_t s) {
    hipLaunchKernelGGL(smplh_fold_weights_kernel, dim3((NV * THMR_SMPLH_NBODY_PAD + 255) / 256), dim3(256), 0, s, W, fold, Wf);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_lbs(const LbsArgs& a, hipStream_t s) {
    const int B = a.B;
    launch_lbs_prep(a, s);
    if (int r = launch_blend(a.xf, a.dirsT, a.vt, a.vposed, B, THMR_LBS_KX, s)) return r;
    // the J19 partial sums live behind the (B,224) operand rows in the xf scratch: B * 27 * 57 floats
    float* jpart = a.xf + (size_t)B * THMR_LBS_KX;
    const int cg = lbs_crops_per_pass(B);
    hipLaunchKernelGGL(lbs_skin_joints_kernel, dim3(SKB, (B + cg - 1) / cg), dim3(256), 0, s, a.vposed, a.W, a.A, a.J19, a.Jtr, a.extra,
                       a.jmap, a.update_hips, a.cam_t, a.verts, jpart, a.xv, a.cnt, a.joints, a.kp2d, a.focal_over_size, B, cg);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_smplh(const SmplhArgs& a, hipStream_t s) {
    if (!a.rotmat || !a.verts || a.B < 1) return -1;
    const int B = a.B, kx = a.body_only ? THMR_SMPLH_KXB : THMR_SMPLH_KX;
    if (a.body_only)
        hipLaunchKernelGGL((prep_kernel<NJH, NBODY, THMR_SMPLH_KXB, SMPLH>), dim3(B), dim3(128), 0, s, a.rotmat, a.betas, a.transl, a.Jt, a.Jsd,
                           a.parents, a.fold, a.A, a.xf, nullptr, nullptr, a.joints);
    else
        hipLaunchKernelGGL((prep_kernel<NJH, NJH, THMR_SMPLH_KX, SMPLH>), dim3(B), dim3(128), 0, s, a.rotmat, a.betas, a.transl, a.Jt, a.Jsd,
                           a.parents, a.fold, a.A, a.xf, nullptr, nullptr, a.joints);
    if (hipGetLastError() != hipSuccess) return -2;
    if (int r = launch_blend(a.xf, a.body_only ? a.dirsT_body : a.dirsT, a.vt, a.vposed, B, kx, s)) return r;
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
