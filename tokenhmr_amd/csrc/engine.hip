// TokenHMR inference engine + C ABI (include/tokenhmr_hip.h).
//
// One engine per GPU: owns a packed weight arena (reference checkpoint tensors at fixed offsets, so a
// single RCCL broadcast of the arena replicates the model) and a static activation arena sized for
// max_batch crops; thmr_forward launches the whole path on the caller's stream with no allocation
// and no host synchronisation.
//
// This file: create / destroy, the per-device turnstile, the timeout recoveries, status, debug, profiler and the forward-type entry points
// (the file map is in engine_state.h).
#include <cstdlib>
#include <map>
#include <mutex>

#include "engine_state.h"

static thread_local std::string g_last_error;

// the one last-error string behind both forms of fail() (abi_util.h); thmr_last_error(nullptr) reads it
int fail(thmr_engine* e, int code, const std::string& msg) {
    if (e) e->err = msg;
    g_last_error = msg;
    return code;
}
int fail(int code, const std::string& msg) { return fail(nullptr, code, msg); }

bool device_has_256_cus() {
    static std::mutex mu;
    static std::map<int, bool> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(dev);
    if (it != cache.end()) return it->second;
    hipDeviceProp_t prop;
    const bool ok = hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount == 256;
    cache[dev] = ok;
    return ok;
}

namespace {

// The persistent kernels need ALL their workgroups resident at once: the decoder kernel has a grid barrier and, from 49 crops on, asks
// for every CU; the persistent split3 GEMM's consumers wait for slabs their producers publish, one 147 KB workgroup per CU.  Two such
// launches issued concurrently by two engines on two streams could each grab part of the chip and wait for the rest until the bounded
// waits run out.  So when a process has more than one engine on a device, their forward-type calls are chained through one event per
// device (struct Turn below: one wait + one record per CALL since round 6, not per launch): each call waits for the previous one (of any
// engine) to finish.  One engine (the normal case) never touches the event, and a capturing stream does not either (an event from outside
// a capture cannot be waited on).  ANOTHER PROCESS on the same GPU is outside this protection: see THMR_CFG_NO_PERSISTENT (header).  (Engines of the shipped and of the experiments
// library in one process each have their own copy of this object: do not run them concurrently on one device — tests do not.)
struct DecoderTurnstile {
    std::mutex mu;
    std::map<int, int> engines;          // device -> live engines
    std::map<int, hipEvent_t> last;      // device -> event recorded at the end of the most recent forward-type call of any engine
};
DecoderTurnstile& turnstile() {
    static DecoderTurnstile t;
    return t;
}

// One TURN per forward-type call (round 6, ADVICE r5: round 5 took the mutex and waited / recorded the event around EVERY persistent launch,
// 33 and more per forward).  With more than one engine of this library on the device and no capture in progress, the call's stream first
// waits for the event the previous call (of any engine) recorded at its end, and records it again at its own end; the mutex is held for the
// host-side enqueue of the whole call (~0.3 ms), so two threads cannot both wait on the same earlier record and then overlap.  Whole
// forwards of different engines therefore run one after the other on the device — which is what kernels that need all 256 CUs resident
// amount to anyway.  One engine per device (the normal case): no lock held, no event touched.
struct Turn {
    std::unique_lock<std::mutex> lk;
    hipStream_t st = nullptr;
    hipEvent_t ev = nullptr;
    int rc = 0;
    Turn(thmr_engine* e, hipStream_t s) : lk(turnstile().mu), st(s) {
        DecoderTurnstile& t = turnstile();
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (t.engines[e->cfg.device] <= 1 || hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
            lk.unlock();
            return;
        }
        auto it = t.last.find(e->cfg.device);
        if (it == t.last.end()) {
            hipEvent_t nev;
            if (hipEventCreateWithFlags(&nev, hipEventDisableTiming) != hipSuccess) { rc = -2; lk.unlock(); return; }
            it = t.last.emplace(e->cfg.device, nev).first;
        } else if (hipStreamWaitEvent(st, it->second, 0) != hipSuccess) { rc = -2; lk.unlock(); return; }
        ev = it->second;
    }
    // records the end of the turn; returns -2 if the record failed (the launches themselves were fine)
    int end() {
        int r = 0;
        if (ev) {
            if (hipEventRecord(ev, st) != hipSuccess) r = -2;
            ev = nullptr;
        }
        if (lk.owns_lock()) lk.unlock();
        return r;
    }
    ~Turn() { (void)end(); }
};

// The persistent decoder kernel's bounded grid barrier timed out in an earlier call (its workgroups were not resident together:
// another process on the GPU, a partition with fewer CUs than reported ...).  That call's outputs are garbage and its barrier
// words are in an undefined state.  Recover instead of staying poisoned: drain the device, zero the barrier words and the
// sticky error, and run this engine's head as the launch chain from now on (it needs no co-residency), so the caller can
// simply re-submit.  Returns the error ONCE.
int recover_decoder_timeout(thmr_engine* e, hipStream_t st = nullptr) {
    // hipDeviceSynchronize / hipMemset are illegal while a stream of this thread is being captured into a hipGraph (they would also
    // invalidate the capture): report, leave the device alone, and let the caller recover outside the capture
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (st != nullptr && hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return fail(e, THMR_ERR_HIP, "persistent decoder kernel: grid barrier timed out in a previous forward, and this call is inside a "
                                     "stream capture: end the capture, call thmr_engine_status() (it resets the engine), then re-capture");
    (void)hipDeviceSynchronize();
    (void)hipMemset(e->sarena + e->so.sync, 0, 512 * sizeof(float));
    if (e->host_err) *e->host_err = 0;
    e->legacy_head = true;
    return fail(e, THMR_ERR_HIP, "persistent decoder kernel: grid barrier timed out in a previous forward (its workgroups could not be "
                                 "resident together); that call's outputs are invalid.  The engine has reset its barrier and switched to "
                                 "the launch-chain head: re-submit the batch");
}

// A consumer of the persistent split3 GEMM gave up waiting for its producer's slab in an earlier call (the launch's workgroups were not
// resident together for ~0.5 s: another kernel held the device).  That call's outputs are invalid.  The epochs in the flags make later
// launches safe by themselves (a late producer cannot be mistaken for a later launch's), but the cause is likely to persist: report ONCE,
// reset the workspace and fall back to the one-workgroup-per-tile kernel (same results), so the caller can simply re-submit.
int recover_split3_timeout(thmr_engine* e, hipStream_t st = nullptr) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (st != nullptr && hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return fail(e, THMR_ERR_HIP, "persistent split3 GEMM: a hand-over wait timed out in a previous forward, and this call is inside a "
                                     "stream capture: end the capture, call thmr_engine_status() (it resets the engine), then re-capture");
    (void)hipDeviceSynchronize();
    if (e->s3_host_err) *e->s3_host_err = 0;
    e->s3_persist = 0;
    if (e->s3_ws) {
        if (int r = reset_s3_workspace(e, nullptr)) return r;
        (void)hipDeviceSynchronize();
    }
    return fail(e, THMR_ERR_HIP, "persistent split3 GEMM: a hand-over wait timed out in a previous forward; that call's outputs are invalid. "
                                 "The engine has reset the workspace and switched to the per-tile kernel: re-submit the batch");
}

int check_ready(thmr_engine* e, int B, hipStream_t st = nullptr) {
    if (!e) return fail(nullptr, THMR_ERR_INVALID, "null engine");
    if (e->host_err && *static_cast<volatile unsigned*>(e->host_err) != 0) return recover_decoder_timeout(e, st);
    if (e->s3_host_err && *static_cast<volatile unsigned*>(e->s3_host_err) != 0) return recover_split3_timeout(e, st);
    if (!e->finalized) return fail(e, THMR_ERR_STATE, "weights not finalized: call thmr_finalize_weights first");
    if (B < 1 || B > e->max_batch) return fail(e, THMR_ERR_INVALID, "batch " + std::to_string(B) + " outside [1, max_batch=" + std::to_string(e->max_batch) + "]");
    return 0;
}

}  // namespace

int validate_cfg(const thmr_config* cfg) {
    if (!cfg) return fail(nullptr, THMR_ERR_INVALID, "null config");
    if (cfg->abi_version != THMR_ABI_VERSION) return fail(nullptr, THMR_ERR_INVALID, "abi_version mismatch");
    if (cfg->vit_depth < 1 || cfg->vit_depth > 64 || cfg->dec_depth < 1 || cfg->dec_depth > 6 || cfg->max_batch < 1 ||
        cfg->max_batch > 4096)
        return fail(nullptr, THMR_ERR_INVALID, "config out of range (vit_depth 1..64, dec_depth 1..6, max_batch 1..4096)");
    if ((cfg->flags & ~(THMR_CFG_VIT_GEMM_F32 | THMR_CFG_NO_PERSISTENT | THMR_CFG_HEAD_HMR2)) != 0 || cfg->reserved[0] != 0 || cfg->reserved[1] != 0)
        return fail(nullptr, THMR_ERR_INVALID, "unknown config flag / non-zero reserved field");
    return 0;
}

// =============================================================================================== C ABI
extern "C" {

int thmr_abi_version(void) { return THMR_ABI_VERSION; }
#ifndef THMR_SRC_HASH
#define THMR_SRC_HASH "unhashed"      // __graft_entry__.build() passes the content hash of csrc/ + include/ + flags
#endif
#ifdef THMR_EXPERIMENTS
#define THMR_BUILD_KIND " experiments"      // environment knobs, debug hooks and the kernels that lost their A/B (csrc/common.h)
#else
#define THMR_BUILD_KIND ""
#endif
const char* thmr_build_info(void) { return "tokenhmr_hip gfx950 fp32-mfma src:" THMR_SRC_HASH THMR_BUILD_KIND " " __DATE__ " " __TIME__; }

const char* thmr_last_error(const thmr_engine* e) { return e ? e->err.c_str() : g_last_error.c_str(); }

// the plan's knobs: their defaults in the shipped library (thmr_knob is a constant nullptr there), THMR_* environment variables in the
// experiments build
static VitKnobs read_knobs() {
    VitKnobs k;
#ifdef THMR_EXPERIMENTS
    auto off = [](const char* name) { const char* v = thmr_knob(name); return v && v[0] == '0'; };
    auto on = [](const char* name) { const char* v = thmr_knob(name); return v && v[0] == '1'; };
    auto num = [](const char* name, int& dst) { if (const char* v = thmr_knob(name)) dst = atoi(v); };
    auto digit = [](const char* name, char hi, int& dst) { const char* v = thmr_knob(name); if (v && v[0] >= '0' && v[0] <= hi) dst = v[0] - '0'; };
    k.qkv_ring16 = !off("THMR_QKV_RING16");
    k.attn_keysplit = !off("THMR_ATTN_KEYSPLIT");
    if (on("THMR_ATTN_B16") || off("THMR_ATTN_B16")) k.attn_b16 = on("THMR_ATTN_B16");
    k.split3_small = on("THMR_SPLIT3_SMALL");
    if (on("THMR_SPLIT3_FC2_SPLIT")) k.split3_fc2_split = 1;
    num("THMR_SPLIT3_MIN_B", k.split3_min_b);
    k.tile_opts = split3_tile_knobs().opts;
    num("THMR_SPLIT3_PN_MASK", k.pn_mask);
    num("THMR_SPLIT3_PN_MAX", k.pn_max);
    num("THMR_SPLIT3_PN_FILL", k.pn_fill);
    num("THMR_SPLIT3_PK_MAX", k.pk_max);
    num("THMR_SPLIT3_PN_FILL_PROJ", k.pn_fill_proj);
    num("THMR_SPLIT3_PW_FILL", k.pw_fill);
    if (off("THMR_SPLIT3_PW_FC1")) k.pw_fc1 = 0;
    digit("THMR_SPLIT3_PERSIST", '1', k.persist);
    digit("THMR_SPLIT3_FC1_MODE", '2', k.fc1_mode);
    num("THMR_SPLIT3_PERSIST_MASK", k.persist_mask);
    k.bs_blk = !off("THMR_SPLIT3_BS_BLK");
    if (const char* ms = thmr_knob("THMR_MID_SPLIT")) {
        if (ms[0] && ms[1]) { k.mid_split_force[0] = ms[0] - '0'; k.mid_split_force[1] = ms[1] - '0'; }
    }
#endif
    return k;
}

int thmr_create(const thmr_config* cfg, void* weight_arena_dev, void* scratch_arena_dev, thmr_engine** out) {
    if (!out) return fail(nullptr, THMR_ERR_INVALID, "null out");
    *out = nullptr;
    if (int r = validate_cfg(cfg)) return r;
    thmr_engine* e = new thmr_engine();
    e->cfg = *cfg;
    e->vit_depth = cfg->vit_depth; e->dec_depth = cfg->dec_depth; e->max_batch = cfg->max_batch;
    e->hmr2 = (cfg->flags & THMR_CFG_HEAD_HMR2) != 0;
    layout_weights(*e, e->vit_depth, e->dec_depth, e->hmr2);
    e->so = layout_scratch(e->max_batch, e->hmr2);
    e->sfloats = e->so.total;
    auto bail = [&](int code, const std::string& m) { fail(nullptr, code, m); thmr_destroy(e); return code; };
    if (hipSetDevice(cfg->device) != hipSuccess) return bail(THMR_ERR_HIP, "hipSetDevice failed");
    if (weight_arena_dev) e->warena = static_cast<float*>(weight_arena_dev);
    else {
        if (hipMalloc(&e->warena, e->wfloats * sizeof(float)) != hipSuccess) return bail(THMR_ERR_NOMEM, "hipMalloc(weights) failed");
        e->own_w = true;
    }
    if (scratch_arena_dev) e->sarena = static_cast<float*>(scratch_arena_dev);
    else {
        if (hipMalloc(&e->sarena, e->sfloats * sizeof(float)) != hipSuccess) return bail(THMR_ERR_NOMEM, "hipMalloc(scratch) failed");
        e->own_s = true;
    }
    // grid-barrier words of the persistent decoder kernel (the scratch arena is private to this engine; a caller-provided
    // one may hold garbage)
    if (hipMemset(e->sarena + e->so.sync, 0, 512 * sizeof(float)) != hipSuccess) return bail(THMR_ERR_HIP, "hipMemset(sync words) failed");
    // arrival counters of the fused skin + joints kernel (self-resetting; zero before the first call)
    if (hipMemset(e->sarena + e->so.lcnt, 0, (size_t)e->max_batch * sizeof(float)) != hipSuccess) return bail(THMR_ERR_HIP, "hipMemset(lbs counters) failed");
    // sticky error word of the persistent decoder kernel, host-mapped so that the next call sees a timeout without a D2H copy
    if (hipHostMalloc(reinterpret_cast<void**>(&e->host_err), 64, hipHostMallocMapped) != hipSuccess) return bail(THMR_ERR_NOMEM, "hipHostMalloc(error word) failed");
    e->host_err[0] = e->host_err[1] = e->host_err[2] = 0;
    e->s3_host_err = e->host_err + 1;
    { const char* lg = thmr_knob("THMR_LEGACY_HEAD"); e->legacy_head = lg && lg[0] == '1'; }
    { const char* mc = thmr_knob("THMR_MIXER_CLUSTER"); e->mixer_cluster = !(mc && mc[0] == '0'); }
    { const char* tg = thmr_knob("THMR_TINY_GEMM"); e->tiny_gemm = !(tg && tg[0] == '0'); }
    e->knobs = read_knobs();
    e->s3_persist = e->knobs.persist;
    if (cfg->flags & THMR_CFG_VIT_GEMM_F32) e->vit_gemm_mode = 0;      // created in the opt-out mode: finalize builds nothing for split3
    if (cfg->flags & THMR_CFG_NO_PERSISTENT) {                         // no kernel that needs all its workgroups resident at once
        e->s3_persist = 0;
        e->legacy_head = true;
        e->no_persistent = true;
    }
    { DecoderTurnstile& t = turnstile(); std::lock_guard<std::mutex> lk(t.mu); t.engines[cfg->device] += 1; e->counted = true; }
    *out = e;
    return 0;
}

void thmr_destroy(thmr_engine* e) {
    if (!e) return;
    if (e->counted) {
        DecoderTurnstile& t = turnstile();
        std::lock_guard<std::mutex> lk(t.mu);
        if (--t.engines[e->cfg.device] <= 0) {              // the device's last engine: its turnstile event goes with it
            auto it = t.last.find(e->cfg.device);
            if (it != t.last.end()) { (void)hipEventDestroy(it->second); t.last.erase(it); }
        }
    }
    for (auto ev : e->ev_pool) (void)hipEventDestroy(ev);
    if (e->host_err) (void)hipHostFree(e->host_err);
    release_split_weights(e);
    if (e->split_act) (void)hipFree(e->split_act);
    if (e->s3_ws) (void)hipFree(e->s3_ws);
    if (e->own_w && e->warena) (void)hipFree(e->warena);
    if (e->own_s && e->sarena) (void)hipFree(e->sarena);
    delete e;
}

// an engine created with THMR_CFG_HEAD_HMR2 has no tokenizer: its entry points and the token outputs are refused by name
static int refuse_hmr2(thmr_engine* e, const char* what) {
    return fail(e, THMR_ERR_INVALID, std::string(what) + " does not exist on an engine created with THMR_CFG_HEAD_HMR2 (the HMR2 head has no pose tokens and no tokenizer)");
}
static int refuse_hmr2_outputs(thmr_engine* e, const thmr_outputs* out) {
    if (!e->hmr2 || !out) return 0;
    if (out->cls_logits_softmax) return refuse_hmr2(e, "thmr_outputs.cls_logits_softmax");
    if (out->cls_logits) return refuse_hmr2(e, "thmr_outputs.cls_logits");
    if (out->token_idx) return refuse_hmr2(e, "thmr_outputs.token_idx");
    return 0;
}

int thmr_vq_decode(thmr_engine* e, const float* probs_dev, int32_t B, float* pose6d_dev, void* stream) {
    if (int r = check_ready(e, B)) return r;
    if (e->hmr2) return refuse_hmr2(e, "thmr_vq_decode");
    if (!probs_dev || !pose6d_dev) return fail(e, THMR_ERR_INVALID, "null buffer");
    return vq_decode(e, probs_dev, B, pose6d_dev, static_cast<hipStream_t>(stream));
}

int thmr_encode_tokens(thmr_engine* e, const float* pose_dev, int32_t B, int32_t* idx_dev, float* latent_dev, void* stream) {
    if (int r = check_ready(e, B)) return r;
    if (e->hmr2) return refuse_hmr2(e, "thmr_encode_tokens");
    if (!e->enc_ready) return fail(e, THMR_ERR_STATE, "tokenizer encoder weights ('encoder.encoder.*') were not loaded");
    if (!pose_dev || !idx_dev) return fail(e, THMR_ERR_INVALID, "null buffer");
    return encode_tokens_call(e, pose_dev, B, idx_dev, latent_dev, nullptr, static_cast<hipStream_t>(stream));
}

// A code index outside [0, 2048) reached a lookup / statistics kernel of this engine (clamped there, never read through): the kernels set
// the host-mapped flag word [2], and the next status read or tokenizer call reports it ONCE.  The work that carried it is invalid.
static int report_bad_code_index(thmr_engine* e) {
    if (!e->host_err || *static_cast<volatile unsigned*>(e->host_err + 2) == 0) return 0;
    e->host_err[2] = 0;
    return fail(e, THMR_ERR_INVALID, "a code index outside [0, 2048) was passed to thmr_vq_decode_idx / thmr_tokenizer_roundtrip in an earlier "
                                     "call (clamped on the device, nothing was read out of bounds); that call's outputs are invalid");
}

int thmr_vq_decode_idx(thmr_engine* e, const int32_t* idx_dev, int32_t B, float* pose6d_dev, void* stream) {
    if (int r = check_ready(e, B)) return r;
    if (e->hmr2) return refuse_hmr2(e, "thmr_vq_decode_idx");
    if (int r = report_bad_code_index(e)) return r;
    if (!idx_dev || !pose6d_dev) return fail(e, THMR_ERR_INVALID, "null buffer");
    return vq_decode_idx(e, idx_dev, nullptr, B, pose6d_dev, static_cast<hipStream_t>(stream));
}

int thmr_tokenizer_roundtrip(thmr_engine* e, const float* pose6d_dev, int32_t B, const thmr_tokenizer_out* out, void* stream) {
    if (int r = check_ready(e, B, static_cast<hipStream_t>(stream))) return r;
    if (e->hmr2) return refuse_hmr2(e, "thmr_tokenizer_roundtrip");
    if (!e->enc_ready) return fail(e, THMR_ERR_STATE, "tokenizer encoder weights ('encoder.encoder.*') were not loaded");
    if (int r = report_bad_code_index(e)) return r;
    if (!pose6d_dev || !out) return fail(e, THMR_ERR_INVALID, "null buffer");
    if (out->accumulate_counts && !out->code_count) return fail(e, THMR_ERR_INVALID, "accumulate_counts needs a code_count buffer");
    return tokenizer_roundtrip_call(e, pose6d_dev, B, out, static_cast<hipStream_t>(stream));
}

int thmr_engine_status(thmr_engine* e, void* stream) {
    if (!e) return fail(e, THMR_ERR_INVALID, "null engine");
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned words[4] = {0, 0, 0, 0};
    HIP_OK(hipMemcpyAsync(words, e->sarena + e->so.sync, sizeof(words), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (words[3] != 0 || (e->host_err && *static_cast<volatile unsigned*>(e->host_err) != 0)) return recover_decoder_timeout(e);
    if (int r = report_bad_code_index(e)) return r;
    if (e->s3_ws) {
        // persistent split3 GEMM: a consumer's bounded wait for a hand-over slab ran out (see recover_split3_timeout; the next forward-type
        // call reports it too, through the host-mapped copy of this word).  Reported once.
        unsigned err = 0;
        if (gemm_split3_persist_error(e->s3_ws, st, &err) != 0) return fail(e, THMR_ERR_HIP, "reading the split3 hand-over error word failed");
        if (e->s3_host_err && *static_cast<volatile unsigned*>(e->s3_host_err) != 0) err = 1;
#ifdef THMR_EXPERIMENTS
        // tests only: report a hand-over timeout that did not happen, once per engine, to exercise the recovery
        if (e->s3_persist && e->vit_gemm_mode == 1 && !e->s3_forced_once) {
            const char* f = thmr_knob("THMR_SPLIT3_FORCE_TIMEOUT");
            if (f && f[0] == '1') { err = 1; e->s3_forced_once = true; }
        }
#endif
        if (err != 0) return recover_split3_timeout(e);
    }
    return 0;
}

int thmr_debug_decoder_timeline(thmr_engine* e, uint64_t* stamps_host, int32_t max_stamps, void* stream) {
    if (!e || !stamps_host || max_stamps < 1 || max_stamps > 240) return fail(e, THMR_ERR_INVALID, "bad argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_OK(hipMemcpyAsync(stamps_host, e->sarena + e->so.sync + 16, sizeof(uint64_t) * max_stamps, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}

int thmr_debug_vit_plan(const thmr_config* cfg, int32_t vit_gemm_mode, int32_t B, int32_t streams_available, thmr_vit_plan_desc* out) {
    if (int r = validate_cfg(cfg)) return r;
    if (vit_gemm_mode != 0 && vit_gemm_mode != 1) return fail(nullptr, THMR_ERR_INVALID, "vit gemm mode must be 0 or 1");
    if (!out || B < 1 || B > cfg->max_batch) return fail(nullptr, THMR_ERR_INVALID, "null out / batch outside [1, max_batch]");
    VitPlanIn in{};
    in.mode = vit_gemm_mode; in.B = B; in.dec_depth = cfg->dec_depth;
    in.split_ready = vit_gemm_mode == 1 && cfg->max_batch >= kSplit3LowMinB;      // what thmr_finalize_weights builds (build_split_weights)
    in.streams = streams_available != 0 && !(cfg->flags & THMR_CFG_NO_PERSISTENT);
    in.part_floats = layout_scratch(cfg->max_batch, false).part_floats;
    *out = plan_vit(read_knobs(), in);
    return 0;
}

// a forward-type call = one turn of the per-device turnstile (struct Turn): r = the call's own result, then the turn's end
static int end_turn(thmr_engine* e, Turn& turn, int r) {
    const int t = turn.end();
    if (r) return r;
    return t ? fail(e, THMR_ERR_HIP, "hipEventRecord failed at the end of the call (per-device engine turnstile)") : 0;
}
#define THMR_TURN(turn, e, st)                                                                                         \
    Turn turn(e, st);                                                                                                  \
    if (turn.rc) return fail(e, THMR_ERR_HIP, "the per-device engine turnstile could not create / wait for its event")

int thmr_vit_forward(thmr_engine* e, const float* img_dev, int32_t B, float* feats_dev, void* stream) {
    if (int r = check_ready(e, B, static_cast<hipStream_t>(stream))) return r;
    if (!img_dev || !feats_dev) return fail(e, THMR_ERR_INVALID, "null buffer");
    THMR_TURN(turn, e, static_cast<hipStream_t>(stream));
    return end_turn(e, turn, vit_forward(e, img_dev, B, feats_dev, static_cast<hipStream_t>(stream)));
}

int thmr_head_forward(thmr_engine* e, const float* ctx_dev, int32_t B, const thmr_outputs* out, void* stream) {
    if (int r = check_ready(e, B, static_cast<hipStream_t>(stream))) return r;
    if (!ctx_dev) return fail(e, THMR_ERR_INVALID, "null buffer");
    if (int r = refuse_hmr2_outputs(e, out)) return r;
    hipStream_t st = static_cast<hipStream_t>(stream);
    THMR_TURN(turn, e, st);
    return end_turn(e, turn, head_forward_call(e, ctx_dev, B, out, st));
}

int thmr_forward(thmr_engine* e, const float* img_dev, int32_t B, const thmr_outputs* out, void* stream) {
    if (int r = check_ready(e, B, static_cast<hipStream_t>(stream))) return r;
    if (!img_dev || !out) return fail(e, THMR_ERR_INVALID, "null buffer");
    if (int r = refuse_hmr2_outputs(e, out)) return r;
    hipStream_t st = static_cast<hipStream_t>(stream);
    THMR_TURN(turn, e, st);
    return end_turn(e, turn, forward_call(e, img_dev, B, out, st));
}

int thmr_lbs_forward(thmr_engine* e, const float* rotmat_dev, const float* betas_dev, const float* cam_dev, int32_t B,
                     float* verts_dev, float* joints_dev, float* cam_t_dev, float* kp2d_dev, void* stream) {
    if (int r = check_ready(e, B)) return r;
    if (!rotmat_dev || !betas_dev) return fail(e, THMR_ERR_INVALID, "null buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float* camt = nullptr;
    if (cam_dev) {
        float* ct = cam_t_dev ? cam_t_dev : e->S(e->so.camt);
        LAUNCH_OK(launch_cam_t(cam_dev, ct, FOCAL, IMG, B, st));
        camt = ct;
    }
    return lbs(e, rotmat_dev, betas_dev, camt, B, verts_dev, joints_dev, camt ? kp2d_dev : nullptr, st);
}

int thmr_vq_argmin(thmr_engine* e, const float* x_dev, int32_t rows, int32_t* idx_dev, float* dist_dev, void* stream) {
    if (!e) return fail(e, THMR_ERR_INVALID, "null engine");
    if (!e->finalized) return fail(e, THMR_ERR_STATE, "weights not finalized");
    if (e->hmr2) return refuse_hmr2(e, "thmr_vq_argmin");
    if (!x_dev || !idx_dev || rows < 1) return fail(e, THMR_ERR_INVALID, "bad argument");
    if ((size_t)rows * NCLS > (size_t)e->max_batch * TOK * 6144) return fail(e, THMR_ERR_INVALID, "rows exceed scratch capacity");
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* dot = e->S(e->so.big);
    GemmArgs a = mk(x_dev, CODE, e->hot.codebook, CODE, nullptr, nullptr, 0, dot, NCLS, rows, NCLS, CODE);
    LAUNCH_OK(launch_gemm(a, EPI_NONE, -1, st));
    LAUNCH_OK(launch_vq_argmin_rows(x_dev, dot, e->warena + e->o_cnorm, idx_dev, dist_dev, rows, st));
    return 0;
}

// ---- profiler ----
int thmr_prof_enable(thmr_engine* e, int32_t on) {
    if (!e) return fail(e, THMR_ERR_INVALID, "null engine");
    e->prof_on = on < 0 ? 0 : (on > 3 ? 1 : on);
    return 0;
}

int thmr_prof_collect(thmr_engine* e, thmr_prof_entry* entries, int32_t reset) {
    if (!e || !entries) return fail(e, THMR_ERR_INVALID, "null argument");
    for (int i = 0; i < THMR_PROF_NUM; ++i) entries[i] = thmr_prof_entry{0, 0, 0, 0};
    for (auto& r : e->prof) {
        HIP_OK(hipEventSynchronize(r.e1));
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, r.e0, r.e1));
        entries[r.cls].ms += ms;
        entries[r.cls].flops += r.flops;
        entries[r.cls].bytes += r.bytes;
        entries[r.cls].launches += 1;
    }
    if (reset) { e->prof.clear(); e->ev_next = 0; }
    return 0;
}

}  // extern "C"
