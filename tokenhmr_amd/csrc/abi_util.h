// Host-side plumbing shared by the files that own C entry points of include/tokenhmr_hip.h: engine.hip (every call that takes a
// thmr_engine) and ops_abi.hip (the stateless operators).  Host only: no kernel includes this.
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
// function through THMR_FAIL(code, msg), which the including file defines: engine.hip as fail(e, code, msg), ops_abi.hip as fail(code, msg).
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
