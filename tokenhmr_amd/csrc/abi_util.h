// Host-side plumbing shared by the files that own C entry points of include/tokenhmr_hip.h: the engine units (engine.hip,
// engine_weights.hip, engine_paths.hip: every call that takes a thmr_engine) and ops_abi.hip (the stateless operators).  Host only: no kernel includes this (SmplConsts::derive calls two launchers).
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
// function through THMR_FAIL(code, msg), which the including file defines: engine_state.h as fail(e, code, msg), ops_abi.hip as fail(code, msg).
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
