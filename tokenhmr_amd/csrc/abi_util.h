// Host-side plumbing shared by the files that own C entry points of include/tokenhmr_hip.h: the engine units (engine.hip,
// engine_weights.hip, engine_paths.hip: every call that takes a thmr_engine), ops_abi.hip (the stateless operators) and body_model_abi.hip
// (the thmr_smpl / thmr_smplh handles).  Host only: no kernel includes this (the body-model structs call launchers of body_model.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/tokenhmr_hip.h"
#include "common.h"

// body-model and camera constants of the release configuration (smpl_wrapper.py:27-41, tokenhmr.py:165-187)
constexpr int NV = 6890, NJ = 24, NB = 10, NP = 207;
constexpr float FOCAL = 5000.0f, IMG = 256.0f;

// One thread-local last-error string (in engine.hip): thmr_last_error(nullptr) reads what either form wrote, from whichever file.  The
// engine form also keeps the message in the engine (thmr_last_error(e)); e may be null.
int fail(thmr_engine* e, int code, const std::string& msg);
int fail(int code, const std::string& msg);

// HIP_OK (a HIP call) / LAUNCH_OK (a launch_* helper: 0, -1 = it refused the arguments, else the launch failed) return from the calling
// function through THMR_FAIL(code, msg), which the including file defines: engine_state.h as fail(e, code, msg), ops_abi.hip and body_model_abi.hip as fail(code, msg).
#define HIP_OK(call)                                                                          \
    do {                                                                                      \
        hipError_t _e = (call);                                                               \
        if (_e != hipSuccess)                                                                 \
            return THMR_FAIL(THMR_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_e)); \
    } while (0)

#define LAUNCH_OK(call)                                                                       \
    do {                                                                                      \
        int _r = (call);                                                                      \
        if (_r != 0) {                                                                        \
            hipError_t _e = hipGetLastError();                                                \
            return THMR_FAIL(_r == -1 ? THMR_ERR_INVALID : THMR_ERR_HIP,                      \
                             std::string(#call) + " failed: " + hipGetErrorString(_e));       \
        }                                                                                     \
    } while (0)

inline size_t align64(size_t f) { return (f + 63) & ~size_t(63); }   // 256-byte alignment in floats

// The SMPL constant block (thmr_smpl_desc + what is derived from it once) as float offsets from a base pointer: the engine lays it into
// its weight arena (whose byte layout is broadcast between ranks), thmr_smpl into its own allocation.
struct SmplConsts {
    size_t vt = 0, sd = 0, pd = 0, jr = 0, w = 0, j19 = 0, ints = 0, jt = 0, jsd = 0, dirs = 0;
    // the int32 block (128 words): parents (24) | extra_verts (21) | joint_map (25) | update_hips (1)
    static constexpr int kParents = 0, kExtra = 24, kJmap = 48, kUpdateHips = 80;
    int32_t hips_host = 0;            // SMPL(update_hips=...), smpl_wrapper.py:11,33-36: the stable source of its asynchronous copy

    size_t lay(size_t off) {          // returns the next free offset
        auto take = [&](size_t& o, size_t n) { o = off; off = align64(off + n); };
        take(vt, (size_t)NV * 3); take(sd, (size_t)NV * 30); take(pd, (size_t)NP * NV * 3); take(jr, (size_t)NJ * NV);
        take(w, (size_t)NV * NJ); take(j19, (size_t)19 * NV); take(ints, 128); take(jt, NJ * 3); take(jsd, NJ * 30);
        take(dirs, (size_t)NV * 3 * THMR_LBS_KX);       // [shapedirs | posedirs | 0]^T, derived
        return off;
    }
    hipError_t upload(float* base, const thmr_smpl_desc* d, hipMemcpyKind k, hipStream_t st) {
        int32_t* iv = reinterpret_cast<int32_t*>(base + ints);
        hips_host = d->update_hips ? 1 : 0;
        const struct { void* dst; const void* src; size_t bytes; hipMemcpyKind kind; } copies[] = {
            {base + vt, d->v_template, sizeof(float) * NV * 3, k},      {base + sd, d->shapedirs, sizeof(float) * NV * 30, k},
            {base + pd, d->posedirs, sizeof(float) * NP * NV * 3, k},   {base + jr, d->J_regressor, sizeof(float) * NJ * NV, k},
            {base + w, d->lbs_weights, sizeof(float) * NV * NJ, k},     {base + j19, d->J19_regressor, sizeof(float) * 19 * NV, k},
            {iv + kParents, d->parents, sizeof(int32_t) * 24, k},       {iv + kExtra, d->extra_verts, sizeof(int32_t) * 21, k},
            {iv + kJmap, d->joint_map, sizeof(int32_t) * 25, k},        {iv + kUpdateHips, &hips_host, sizeof(int32_t), hipMemcpyHostToDevice}};
        for (const auto& c : copies)
            if (hipError_t e = hipMemcpyAsync(c.dst, c.src, c.bytes, c.kind, st)) return e;
        return hipSuccess;
    }
    int derive(float* base, hipStream_t st) const {     // Jt / Jsd and dirs^T from what upload() copied
        if (int r = launch_body_jreg(base + jr, base + vt, base + sd, base + jt, base + jsd, NJ, st)) return r;
        return launch_body_build_dirs(base + sd, base + pd, base + dirs, NP, THMR_LBS_KX, st);
    }
    void fill(LbsArgs& a, const float* base) const {    // the constant pointers of one launch_lbs call
        const int32_t* iv = reinterpret_cast<const int32_t*>(base + ints);
        a.Jt = base + jt; a.Jsd = base + jsd; a.vt = base + vt; a.dirsT = base + dirs; a.W = base + w; a.J19 = base + j19;
        a.parents = iv + kParents; a.extra = iv + kExtra; a.jmap = iv + kJmap; a.update_hips = iv + kUpdateHips;
    }
};

// thmr_smplh's constant block, the same way (thmr_smplh_desc + what is derived from it once), and the per-batch scratch behind it
struct SmplhConsts {
    size_t vt = 0, sd = 0, pd = 0, jr = 0, w = 0, wb = 0, ints = 0, jt = 0, jsd = 0, dirs = 0, dirsb = 0;
    size_t A = 0, xf = 0, rot = 0, vposed = 0;      // scratch: (B,52,12), (B,480), (B,52,9) for pose2rot, (B,20670)
    // the int32 block (192 words): parents [0, 52) | extra_verts [64, 85) | fold [128, 180)
    static constexpr int kParents = 0, kExtra = 64, kFold = 128;
    static constexpr int HJ = THMR_SMPLH_NJ, HB = THMR_SMPLH_NBODY, HP = THMR_SMPLH_NP;

    size_t lay(size_t off, size_t B) {          // returns the next free offset
        auto take = [&](size_t& o, size_t n) { o = off; off = align64(off + n); };
        take(vt, (size_t)NV * 3); take(sd, (size_t)NV * 30); take(pd, (size_t)HP * NV * 3); take(jr, (size_t)HJ * NV);
        take(w, (size_t)NV * HJ); take(wb, (size_t)NV * THMR_SMPLH_NBODY_PAD);      // wb: the folded path's weights, derived
        take(ints, 192); take(jt, HJ * 3); take(jsd, HJ * 30);
        take(dirs, (size_t)NV * 3 * THMR_SMPLH_KX); take(dirsb, (size_t)NV * 3 * THMR_SMPLH_KXB);      // both derived
        take(A, B * HJ * 12); take(xf, B * THMR_SMPLH_KX); take(rot, B * HJ * 9); take(vposed, B * NV * 3);
        return off;
    }
    // par (52), ext (21) and fold (52) are the caller's validated host copies; the float arrays come from d as it says (k)
    bool upload(float* base, const thmr_smplh_desc* d, hipMemcpyKind k, const int32_t* par, const int32_t* ext, const int32_t* fold) const {
        int32_t* iv = reinterpret_cast<int32_t*>(base + ints);
        auto cp = [](void* dst, const void* src, size_t bytes, hipMemcpyKind kind) { return hipMemcpy(dst, src, bytes, kind) == hipSuccess; };
        return cp(base + vt, d->v_template, sizeof(float) * NV * 3, k) && cp(base + sd, d->shapedirs, sizeof(float) * NV * 30, k) &&
               cp(base + pd, d->posedirs, sizeof(float) * HP * NV * 3, k) && cp(base + jr, d->J_regressor, sizeof(float) * HJ * NV, k) &&
               cp(base + w, d->lbs_weights, sizeof(float) * NV * HJ, k) && cp(iv + kParents, par, sizeof(int32_t) * HJ, hipMemcpyHostToDevice) &&
               cp(iv + kExtra, ext, sizeof(int32_t) * 21, hipMemcpyHostToDevice) && cp(iv + kFold, fold, sizeof(int32_t) * HJ, hipMemcpyHostToDevice);
    }
    int derive(float* base, hipStream_t st) const {     // Jt / Jsd, both dirs^T and the folded weights from what upload() copied
        if (int r = launch_body_jreg(base + jr, base + vt, base + sd, base + jt, base + jsd, HJ, st)) return r;
        if (int r = launch_body_build_dirs(base + sd, base + pd, base + dirs, (HJ - 1) * 9, THMR_SMPLH_KX, st)) return r;
        if (int r = launch_body_build_dirs(base + sd, base + pd, base + dirsb, (HB - 1) * 9, THMR_SMPLH_KXB, st)) return r;
        return launch_smplh_fold_weights(base + w, reinterpret_cast<const int32_t*>(base + ints) + kFold, base + wb, st);
    }
    void fill(SmplhArgs& a, float* base) const {        // the constant and scratch pointers of one launch_smplh call
        const int32_t* iv = reinterpret_cast<const int32_t*>(base + ints);
        a.Jt = base + jt; a.Jsd = base + jsd; a.vt = base + vt; a.dirsT = base + dirs; a.dirsT_body = base + dirsb; a.W = base + w; a.W_body = base + wb;
        a.parents = iv + kParents; a.extra = iv + kExtra; a.fold = iv + kFold;
        a.A = base + A; a.xf = base + xf; a.vposed = base + vposed;
    }
};

// The backward's own allocation of a body-model handle (thmr_smpl: one; thmr_smplh: one per path): dirsT transposed (kx, 20672), g_vposed
// (B, 20672), the bone-matrix partials (B, ga_per_item), the split-K planes (38, B, kx) and, for pose2rot, the rotation matrices' gradient
// (B, nj, 9).  mem is null until reserve() has succeeded.
struct BodyGradWorkspace {
    float* mem = nullptr;
    size_t dirs = 0, vp = 0, part = 0, planes = 0, rot = 0;

    // 0, THMR_ERR_NOMEM (the allocation) or THMR_ERR_HIP (building dirsK); synchronises the device once.  The current device is the handle's.
    int reserve(const float* dirsT, size_t kx, size_t ga_per_item, size_t nj, size_t max_batch) {
        size_t off = 0;
        auto take = [&](size_t& o, size_t n) { o = off; off = align64(off + n); };
        take(dirs, kx * THMR_LBS_GK); take(vp, max_batch * THMR_LBS_GK); take(part, max_batch * ga_per_item);
        take(planes, (size_t)THMR_LBS_GKSPLIT * max_batch * kx); take(rot, max_batch * nj * 9);
        float* g = nullptr;
        if (hipMalloc(&g, off * sizeof(float)) != hipSuccess) return THMR_ERR_NOMEM;
        if (launch_body_build_dirs_k(dirsT, g + dirs, (int)kx, nullptr) != 0 || hipDeviceSynchronize() != hipSuccess) {
            (void)hipFree(g);
            return THMR_ERR_HIP;
        }
        mem = g;
        return 0;
    }
    void fill(BodyGradArgs& g, const float* gV, const float* gJ, bool pose2rot, float* grad_pose, float* grad_betas, float* grad_transl) const {
        g.gV = gV; g.gJ = gJ; g.dirsK = mem + dirs; g.gvp = mem + vp; g.gApart = mem + part; g.planes = mem + planes;
        g.grad_rotmat = !grad_pose ? nullptr : (pose2rot ? mem + rot : grad_pose);      // axis-angle: finished from `rot` (finish_pose_grad)
        g.grad_betas = grad_betas; g.grad_transl = grad_transl;
    }
    void release() { if (mem) (void)hipFree(mem); mem = nullptr; }
};

inline GemmArgs mk(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, const float* resid, int64_t ldr,
                   float* C, int64_t ldc, int M, int N, int K) {
    GemmArgs a{};
    a.A = A; a.W = W; a.bias = bias; a.resid = resid; a.C = C;
    a.lda = lda; a.ldw = ldw; a.ldc = ldc; a.ldr = ldr;
    a.M = M; a.N = N; a.K = K; a.qscale = 1.f; a.qcols = 0;
    return a;
}

// the persistent split3 GEMM's decomposition is 8 XCDs x 32 CUs: only offered on a 256-CU device (cached per device; engine.hip)
bool device_has_256_cus();
