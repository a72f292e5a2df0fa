// The stand-alone body models of include/tokenhmr_hip.h: the thmr_smpl and thmr_smplh handles.  Each owns one allocation of constants and
// per-batch scratch (SmplConsts / SmplhConsts, abi_util.h) and, once reserved, the backward's workspaces (BodyGradWorkspace); every call
// validates its arguments before any HIP call and then launches what the engine launches, through body_model.hip's launch_* (common.h).
#include <hip/hip_runtime.h>

#include "abi_util.h"

#define THMR_FAIL(code, msg) fail(code, msg)      // HIP_OK / LAUNCH_OK (abi_util.h)

// pose as rotation matrices: itself, or (pose2rot) its n axis-angle vectors converted into rot_scratch.  nullptr: the launch failed, error recorded
static const float* resolve_pose(const float* pose, int pose2rot, float* rot_scratch, int n, hipStream_t st) {
    if (!pose2rot) return pose;
    if (launch_rodrigues(pose, rot_scratch, n, st) == 0) return rot_scratch;
    fail(THMR_ERR_HIP, std::string("launch_rodrigues failed: ") + hipGetErrorString(hipGetLastError()));
    return nullptr;
}

// the reverse: the matrices' gradient the backward left in the workspace (BodyGradWorkspace::fill) becomes the axis-angle vectors'
static int finish_pose_grad(const float* pose, int pose2rot, const BodyGradWorkspace& ws, float* grad_pose, int n, hipStream_t st) {
    if (pose2rot && grad_pose) LAUNCH_OK(launch_rodrigues_backward(pose, ws.mem + ws.rot, grad_pose, n, st));
    return 0;
}

extern "C" {

// ---- stand-alone SMPL model ----
struct thmr_smpl {
    float* mem = nullptr;
    int max_batch = 0;
    SmplConsts c;
    size_t o_A, o_pf, o_Jtr, o_vposed, o_rot, o_joints, o_xv, o_cnt;
    BodyGradWorkspace grad;           // thmr_smpl_grad_reserve
    int device = 0;

    // constants, scratch and inputs of a forward or backward launch; an axis-angle pose goes through the rot scratch first
    int fill(LbsArgs& a, const float* pose, int pose2rot, const float* betas, int B, hipStream_t st) const {
        if (!(a.rotmat = resolve_pose(pose, pose2rot, mem + o_rot, B * NJ, st))) return THMR_ERR_HIP;
        c.fill(a, mem);
        a.betas = betas; a.B = B;
        a.A = mem + o_A; a.xf = mem + o_pf; a.Jtr = mem + o_Jtr; a.vposed = mem + o_vposed;
        a.cnt = reinterpret_cast<unsigned*>(mem + o_cnt);
        return 0;
    }
};

int thmr_smpl_create(const thmr_smpl_desc* d, int32_t max_batch, int32_t device, thmr_smpl** out) {
    if (!d || !out || max_batch < 1) return fail(THMR_ERR_INVALID, "bad argument");
    *out = nullptr;
    if (!d->v_template || !d->shapedirs || !d->posedirs || !d->J_regressor || !d->lbs_weights || !d->J19_regressor ||
        !d->parents || !d->extra_verts || !d->joint_map)
        return fail(THMR_ERR_INVALID, "thmr_smpl_desc has a null field");
    HIP_OK(hipSetDevice(device));
    thmr_smpl* m = new thmr_smpl();
    m->max_batch = max_batch; m->device = device;
    size_t off = m->c.lay(0);
    auto take = [&](size_t n) { size_t o = off; off = align64(off + n); return o; };
    const size_t B = (size_t)max_batch;
    m->o_A = take(B * NJ * 12); m->o_pf = take(B * THMR_LBS_XF); m->o_Jtr = take(B * NJ * 3); m->o_rot = take(B * NJ * 9);
    m->o_vposed = take(B * NV * 3); m->o_joints = take(B * 132);
    m->o_xv = take(B * 63); m->o_cnt = take(B);
    if (hipMalloc(&m->mem, off * sizeof(float)) != hipSuccess) { delete m; return fail(THMR_ERR_NOMEM, "hipMalloc(smpl) failed"); }
    if (hipMemset(m->mem + m->o_cnt, 0, B * sizeof(float)) != hipSuccess) { thmr_smpl_destroy(m); return fail(THMR_ERR_HIP, "hipMemset(lbs counters) failed"); }
    // upload() only enqueues its copies: d's arrays and m->c.hips_host are read until the hipDeviceSynchronize() below
    if (m->c.upload(m->mem, d, d->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, nullptr) != hipSuccess ||
        m->c.derive(m->mem, nullptr) != 0 || hipDeviceSynchronize() != hipSuccess) {
        thmr_smpl_destroy(m);
        return fail(THMR_ERR_HIP, "SMPL constant upload failed");
    }
    *out = m;
    return 0;
}

void thmr_smpl_destroy(thmr_smpl* m) {
    if (!m) return;
    if (m->mem) (void)hipFree(m->mem);
    m->grad.release();
    delete m;
}

int thmr_smpl_forward(thmr_smpl* m, const float* pose, int32_t pose2rot, const float* betas, int32_t B, float* verts,
                      float* joints, void* stream) {
    if (!m || !pose || !betas || !verts) return fail(THMR_ERR_INVALID, "null argument");
    if (B < 1 || B > m->max_batch) return fail(THMR_ERR_INVALID, "batch outside [1, max_batch]");
    hipStream_t st = static_cast<hipStream_t>(stream);
    LbsArgs a{};
    if (int rc = m->fill(a, pose, pose2rot, betas, B, st)) return rc;
    a.xv = m->mem + m->o_xv;
    a.verts = verts; a.joints = joints ? joints : m->mem + m->o_joints;
    a.focal_over_size = FOCAL / IMG;
    LAUNCH_OK(launch_lbs(a, st));
    return 0;
}

int thmr_smpl_grad_reserve(thmr_smpl* m) {
    if (!m) return fail(THMR_ERR_INVALID, "smpl_grad_reserve: null handle");
    if (m->grad.mem) return 0;
    HIP_OK(hipSetDevice(m->device));
    if (int rc = m->grad.reserve(m->mem + m->c.dirs, THMR_LBS_KX, THMR_LBS_GA, NJ, (size_t)m->max_batch))
        return fail(rc, rc == THMR_ERR_NOMEM ? "hipMalloc(smpl backward workspace) failed"
                                             : "smpl_grad_reserve: building the transposed blend-shape matrix failed");
    return 0;
}

int thmr_smpl_backward(thmr_smpl* m, const float* pose, int32_t pose2rot, const float* betas, int32_t B, const float* grad_verts,
                       const float* grad_joints, float* grad_pose, float* grad_betas, void* stream) {
    if (!m || !pose || !betas) return fail(THMR_ERR_INVALID, "smpl_backward: null handle, pose or betas");
    if (!grad_verts && !grad_joints) return fail(THMR_ERR_INVALID, "smpl_backward: grad_verts and grad_joints are both null");
    if (!grad_pose && !grad_betas) return fail(THMR_ERR_INVALID, "smpl_backward: grad_pose and grad_betas are both null");
    if (B < 1 || B > m->max_batch) return fail(THMR_ERR_INVALID, "smpl_backward: batch outside [1, max_batch]");
    if (pose2rot != 0 && pose2rot != 1) return fail(THMR_ERR_INVALID, "smpl_backward: pose2rot is 0 or 1");
    if (!m->grad.mem) return fail(THMR_ERR_INVALID, "smpl_backward: call thmr_smpl_grad_reserve on this handle first");
    hipStream_t st = static_cast<hipStream_t>(stream);
    LbsArgs a{};
    if (int rc = m->fill(a, pose, pose2rot, betas, B, st)) return rc;
    BodyGradArgs g{};
    m->grad.fill(g, grad_verts, grad_joints, pose2rot, grad_pose, grad_betas, nullptr);
    LAUNCH_OK(launch_lbs_backward(a, g, st));
    return finish_pose_grad(pose, pose2rot, m->grad, grad_pose, B * NJ, st);
}

// ---- stand-alone SMPL-H model ----
struct thmr_smplh {
    float* mem = nullptr;
    int max_batch = 0;
    SmplhConsts c;
    BodyGradWorkspace grad[2];        // thmr_smplh_grad_reserve, one per path: [0] full, [1] folded
    int device = 0;

    int fill(SmplhArgs& a, const float* pose, int pose2rot, const float* betas, const float* transl, int body_only, int B, hipStream_t st) const {
        if (!(a.rotmat = resolve_pose(pose, pose2rot, mem + c.rot, B * (body_only ? THMR_SMPLH_NBODY : THMR_SMPLH_NJ), st))) return THMR_ERR_HIP;
        c.fill(a, mem);
        a.betas = betas; a.transl = transl; a.B = B; a.body_only = body_only;
        return 0;
    }
};

int thmr_smplh_create(const thmr_smplh_desc* d, int32_t max_batch, int32_t device, thmr_smplh** out) {
    constexpr int HJ = THMR_SMPLH_NJ, HB = THMR_SMPLH_NBODY;
    if (!d || !out || max_batch < 1) return fail(THMR_ERR_INVALID, "bad argument");
    *out = nullptr;
    if (!d->v_template || !d->shapedirs || !d->posedirs || !d->J_regressor || !d->lbs_weights || !d->parents || !d->extra_verts)
        return fail(THMR_ERR_INVALID, "thmr_smplh_desc has a null field");
    HIP_OK(hipSetDevice(device));
    int32_t par[HJ], ext[21], fold[HJ];
    const hipMemcpyKind to_host = d->on_device ? hipMemcpyDeviceToHost : hipMemcpyHostToHost;
    HIP_OK(hipMemcpy(par, d->parents, sizeof(par), to_host));
    HIP_OK(hipMemcpy(ext, d->extra_verts, sizeof(ext), to_host));
    if (par[0] != -1) return fail(THMR_ERR_INVALID, "thmr_smplh_desc.parents[0] must be -1 (the root)");
    for (int i = 1; i < HJ; ++i)
        if (par[i] < 0 || par[i] >= i)
            return fail(THMR_ERR_INVALID, "thmr_smplh_desc.parents[" + std::to_string(i) + "] = " + std::to_string(par[i]) + " is outside [0, " + std::to_string(i) + ")");
    for (int k = 0; k < 21; ++k)
        if (ext[k] < 0 || ext[k] >= NV)
            return fail(THMR_ERR_INVALID, "thmr_smplh_desc.extra_verts[" + std::to_string(k) + "] = " + std::to_string(ext[k]) + " is outside [0, 6890)");
    // fold[j]: the body joint whose bone matrix joint j has when every hand rotation is the identity.  parents[i] < i keeps the 22 body
    // joints a chain of their own and gives fold[j] < 22 by induction (one ascending pass)
    for (int j = 0; j < HJ; ++j) fold[j] = j < HB ? j : fold[par[j]];
    thmr_smplh* m = new thmr_smplh();
    m->max_batch = max_batch; m->device = device;
    if (hipMalloc(&m->mem, m->c.lay(0, (size_t)max_batch) * sizeof(float)) != hipSuccess) { delete m; return fail(THMR_ERR_NOMEM, "hipMalloc(smplh) failed"); }
    if (!m->c.upload(m->mem, d, d->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, par, ext, fold) ||
        m->c.derive(m->mem, nullptr) != 0 || hipDeviceSynchronize() != hipSuccess) {
        thmr_smplh_destroy(m);
        return fail(THMR_ERR_HIP, "SMPL-H constant upload failed");
    }
    *out = m;
    return 0;
}

void thmr_smplh_destroy(thmr_smplh* m) {
    if (!m) return;
    if (m->mem) (void)hipFree(m->mem);
    for (auto& g : m->grad) g.release();
    delete m;
}

int thmr_smplh_forward(thmr_smplh* m, const float* pose, int32_t pose2rot, const float* betas, const float* transl, int32_t body_only,
                       int32_t B, float* verts, float* joints, void* stream) {
    if (!m || !pose || !verts) return fail(THMR_ERR_INVALID, "smplh_forward: null argument");
    if (B < 1 || B > m->max_batch) return fail(THMR_ERR_INVALID, "smplh_forward: batch outside [1, max_batch]");
    if ((pose2rot != 0 && pose2rot != 1) || (body_only != 0 && body_only != 1))
        return fail(THMR_ERR_INVALID, "smplh_forward: pose2rot and body_only are 0 or 1");
    hipStream_t st = static_cast<hipStream_t>(stream);
    SmplhArgs a{};
    if (int rc = m->fill(a, pose, pose2rot, betas, transl, body_only, B, st)) return rc;
    a.verts = verts; a.joints = joints;
    LAUNCH_OK(launch_smplh(a, st));
    return 0;
}

int thmr_smplh_grad_reserve(thmr_smplh* m, int32_t paths) {
    if (!m) return fail(THMR_ERR_INVALID, "smplh_grad_reserve: null handle");
    if (paths < 1 || paths > (THMR_SMPLH_GRAD_FOLDED | THMR_SMPLH_GRAD_FULL))
        return fail(THMR_ERR_INVALID, "smplh_grad_reserve: paths is THMR_SMPLH_GRAD_FOLDED (1), THMR_SMPLH_GRAD_FULL (2) or both (3)");
    HIP_OK(hipSetDevice(m->device));
    for (int folded = 0; folded < 2; ++folded) {
        if (!(paths & (folded ? THMR_SMPLH_GRAD_FOLDED : THMR_SMPLH_GRAD_FULL)) || m->grad[folded].mem) continue;
        if (int rc = folded ? m->grad[1].reserve(m->mem + m->c.dirsb, THMR_SMPLH_KXB, THMR_SMPLH_GA_BODY, THMR_SMPLH_NBODY, (size_t)m->max_batch)
                            : m->grad[0].reserve(m->mem + m->c.dirs, THMR_SMPLH_KX, THMR_SMPLH_GA, THMR_SMPLH_NJ, (size_t)m->max_batch))
            return fail(rc, rc == THMR_ERR_NOMEM ? "hipMalloc(smplh backward workspace) failed"
                                                 : "smplh_grad_reserve: building the transposed blend-shape matrix failed");
    }
    return 0;
}

int thmr_smplh_backward(thmr_smplh* m, const float* pose, int32_t pose2rot, const float* betas, const float* transl, int32_t body_only,
                        int32_t B, const float* grad_verts, const float* grad_joints, float* grad_pose, float* grad_betas,
                        float* grad_transl, void* stream) {
    if (!m || !pose) return fail(THMR_ERR_INVALID, "smplh_backward: null handle or pose");
    if (!grad_verts && !grad_joints) return fail(THMR_ERR_INVALID, "smplh_backward: grad_verts and grad_joints are both null");
    if (!grad_pose && !grad_betas && !grad_transl) return fail(THMR_ERR_INVALID, "smplh_backward: grad_pose, grad_betas and grad_transl are all null");
    if (B < 1 || B > m->max_batch) return fail(THMR_ERR_INVALID, "smplh_backward: batch outside [1, max_batch]");
    if ((pose2rot != 0 && pose2rot != 1) || (body_only != 0 && body_only != 1))
        return fail(THMR_ERR_INVALID, "smplh_backward: pose2rot and body_only are 0 or 1");
    const BodyGradWorkspace& ws = m->grad[body_only];
    if (!ws.mem)
        return fail(THMR_ERR_INVALID, body_only ? "smplh_backward: the folded path was not reserved (thmr_smplh_grad_reserve with THMR_SMPLH_GRAD_FOLDED)"
                                                : "smplh_backward: the full path was not reserved (thmr_smplh_grad_reserve with THMR_SMPLH_GRAD_FULL)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    SmplhArgs a{};
    if (int rc = m->fill(a, pose, pose2rot, betas, transl, body_only, B, st)) return rc;
    BodyGradArgs g{};
    ws.fill(g, grad_verts, grad_joints, pose2rot, grad_pose, grad_betas, grad_transl);
    LAUNCH_OK(launch_smplh_backward(a, g, st));
    return finish_pose_grad(pose, pose2rot, ws, grad_pose, B * (body_only ? THMR_SMPLH_NBODY : THMR_SMPLH_NJ), st);
}

}  // extern "C"
