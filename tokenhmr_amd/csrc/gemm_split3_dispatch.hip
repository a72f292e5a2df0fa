// Host side of the split3 GEMM (no kernel here): the entry points the engine and the operators call, their argument checks, the tile
// stream's workspace, and the execution of the tile rule (gemm_split3_rule.h — a pure function, tested without a GPU).  The kernels are
// gemm_split16.hip (what ships) and gemm_split3_exp.hip (experiments build); the operand format is described in split3_convert.hip.
#include <cstdlib>
#include <map>
#include <mutex>

#include "common.h"
#include "gemm_split_device.h"
#include "gemm_split3_rule.h"

// compute units of the current device (cached per device)
static int device_cus() {
    static std::mutex mu;
    static std::map<int, int> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(dev);
    if (it != cache.end()) return it->second;
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 0;
    cache[dev] = n;
    return n;
}

// The A/B knobs of the tile rule, read HERE only (experiments build; thmr_knob is a constant nullptr in the shipped library: {-1, 0}).
// engine.hip read_knobs takes `opts` as the plan's tile_opts, launch_split3_tiles ORs it into GemmArgs::tile_opts: one environment for both.
Split3TileKnobs split3_tile_knobs() {
    using namespace split3_rule;
    auto is = [](const char* name, char c) { const char* v = thmr_knob(name); return v && v[0] == c; };
    const char* tile = thmr_knob("THMR_SPLIT3_TILE");                    // a variant id (0 / 2) for every launch that asks for the rule
    return {tile ? atoi(tile) : -1, (is("THMR_SPLIT3_NARROW8", '1') ? kOptNarrow8 : 0) | (is("THMR_SPLIT3_TAIL8", '1') ? kOptTail8 : 0) | (is("THMR_SPLIT3_RING3", '0') ? kOptRing2 : 0) |
                                        (is("THMR_SPLIT3_FRONT", '0') ? kOptNoFront : 0) | (is("THMR_SPLIT3_TAIL", '0') ? kOptNoTail : 0)};
}

static_assert(split3_rule::kEpiNone == EPI_NONE && split3_rule::kEpiBiasResid == EPI_BIAS_RESID &&
              split3_rule::kTailEpis == (1u << EPI_NONE | 1u << EPI_BIAS | 1u << EPI_BIAS_GELU | 1u << EPI_BIAS_RESID | 1u << EPI_BIAS_QSCALE),
              "gemm_split3_rule.h restates the epilogue ids");

static int launch_split3_tiles(const GemmArgs& a, int epi, int variant, hipStream_t s) {
    static const Split3TileKnobs knobs = split3_tile_knobs();
    if (variant < 0) variant = knobs.forced_tile;
    const split3_rule::Choice c = split3_rule::choose(a.M, a.N, a.ksplit, a.a_blk != 0, epi, variant, a.tile_opts | knobs.opts, device_cus());
    switch (c.kind) {
        case split3_rule::Choice::TILES: return launch_split16_tiles(a, epi, c.shape, s);
        // ("not mine", 1, would be a disagreement with the rule, which knows the tail's epilogues)
        case split3_rule::Choice::TAIL: { const int r = launch_split16_tiles_tail(a, epi, c.q, c.tail_from, c.tail8, s); return r > 0 ? -1 : r; }
#ifdef THMR_EXPERIMENTS
        case split3_rule::Choice::EXP: return launch_split3_exp_tiles(a, epi, c.shape, s);
#endif
        default: return -1;
    }
}

// a.A / a.W point at split3 operands (lda / ldw = their row strides in fp32-equivalents, i.e. 6 lda bytes); C, bias, resid are fp32.
// variant: -1 = the rule, or an id of split3_rule::choose (gemm_split3_rule.h)
int launch_gemm_split3(const GemmArgs& a, int epi, int variant, hipStream_t s) {
    if (a.M <= 0 || a.N <= 0 || a.K <= 0 || (a.K % SBK) != 0 || (a.lda % 8) != 0 || (a.ldw % 8) != 0) return -1;
    if (a.lda * 6 * 256 >= (int64_t(1) << 32) || a.ldw * 6 * 256 >= (int64_t(1) << 32)) return -1;     // 32-bit lane offsets within a tile
    if (a.cs_out != nullptr || a.ksplit > 1) return -1;
    if (a.c_split != nullptr && ((a.N % 8) != 0 || (a.ldcs % 8) != 0 || a.ldcs < a.N || epi == EPI_BIAS_RESID)) return -1;
    return launch_split3_tiles(a, epi, variant, s);
}

// Split-K on the split3 big tiles (the mode's 3 ... 31 crops: the N = 1280 GEMMs have 25-240 tiles of 128 x 256): `ksplit` copies of the tile
// grid in ONE launch, copy sp reducing K slice sp into part[sp][M][N] (raw fp32 partial tiles, no epilogue), summed in a fixed order by the
// residual + LayerNorm kernel that follows proj / fc2 anyway.  Tile by the same rule over tiles * ksplit (bit-identical either way).
int launch_gemm_split3_splitk(const GemmArgs& a0, int ksplit, float* part, hipStream_t s) {
    if (ksplit < 2 || part == nullptr) return -1;
    if (a0.M <= 0 || a0.N <= 0 || a0.K <= 0 || (a0.K % (SBK * ksplit)) != 0 || (a0.lda % 8) != 0 || (a0.ldw % 8) != 0) return -1;
    if (a0.lda * 6 * 256 >= (int64_t(1) << 32) || a0.ldw * 6 * 256 >= (int64_t(1) << 32) || a0.cs_out != nullptr || a0.c_split != nullptr) return -1;
    GemmArgs a = a0;
    a.ksplit = ksplit;
    a.C = part; a.ldc = a.N;
    a.bias = nullptr; a.resid = nullptr; a.ldr = 0;
    return launch_split3_tiles(a, EPI_NONE, -1, s);
}

size_t gemm_split3_persist_ws_bytes() { return (size_t)P_NWG * P_SLAB * 4 + (P_NWG + 64) * sizeof(unsigned); }

bool gemm_split3_persist_ok(const GemmArgs& a) {
    // (round 6: M may be ragged — an odd number of crops — for the product kernel of gemm_split16.hip; the row-blocked operands hold whole
    // 32-row blocks, which 192 B rows always are)
    if (a.M <= 0 || a.N <= 0 || a.K < 2 * SBK || (a.K % SBK) != 0 || (a.M % 32) != 0 || (a.N % PBN) != 0) return false;
    if ((int64_t)((a.M + PBM - 1) / PBM) * (a.N / PBN) < P_NWG) return false;     // every lane's list holds >= 8 tiles: a range >= one tile
    if ((a.lda % 8) != 0 || (a.ldw % 8) != 0 || a.lda * 6 * 256 >= (int64_t(1) << 32) || a.ldw * 6 * 256 >= (int64_t(1) << 32)) return false;
    if (a.cs_out != nullptr || a.ksplit > 1) return false;
    if (a.c_split != nullptr && ((a.N % 8) != 0 || (a.ldcs % 8) != 0 || a.ldcs < a.N)) return false;
    return true;
}

// ws: gemm_split3_persist_ws_bytes() of device memory, ZEROED once when it is allocated; one launch at a time per workspace.  Layout: 256 slabs,
// then 256 flag words (gemm_split16.hip: the epoch of the launch that published the slab), then the control words: + 0 error, + 1 epoch,
// + 2 arrival counter, + 4 / + 5 the address of a host-mapped error word (gemm_split3_persist_bind_host_err; zero = none).  mode: 0 fp32 output; 2 split3 output (a.c_split) — both gemm_split16.hip's kernel (one epilogue for both
// outputs); 10 / 11 / 12 = the 32x32x16 stream kernels of the experiments build (gemm_split3_exp.hip)
int launch_gemm_split3_persist(const GemmArgs& a, int epi, int mode, void* ws_mem, hipStream_t s) {
    if (!gemm_split3_persist_ok(a) || ws_mem == nullptr) return -1;
    if (mode == 0 || mode == 2) {
        if ((mode == 0) != (a.c_split == nullptr)) return -1;
        return launch_split16_persist(a, epi, ws_mem, false, s);
    }
#ifdef THMR_EXPERIMENTS
    return launch_split3_exp_persist(a, epi, mode, ws_mem, s);
#else
    return -1;
#endif
}

bool gemm_split3_persist_narrow_ok(const GemmArgs& a) {
    const int ks = a.ksplit > 1 ? a.ksplit : 1;                                    // split-K: the stream's units are (tile, K slice) pairs, raw partial sums
    if (a.M <= 0 || a.N <= 0 || (a.K % (SBK * ks)) != 0 || a.K / ks < 3 * SBK || (a.N % 128) != 0) return false;      // (M may be ragged: a multiple of 192 rows)
    if ((int64_t)((a.M + 127) / 128) * (a.N / 128) * ks < P_NWG) return false;     // every lane's list holds >= 8 units: a range >= one unit
    if ((a.lda % 8) != 0 || (a.ldw % 8) != 0 || a.lda * 6 * 128 >= (int64_t(1) << 32) || a.ldw * 6 * 128 >= (int64_t(1) << 32)) return false;
    if (a.cs_out != nullptr || a.a_blk) return false;
    if (ks > 1 && (a.c_split != nullptr || a.bias != nullptr || a.resid != nullptr)) return false;
    if (a.c_split != nullptr && ((a.N % 8) != 0 || (a.ldcs % 8) != 0 || a.ldcs < a.N)) return false;
    return true;
}

int launch_gemm_split3_persist_narrow(const GemmArgs& a, int epi, void* ws_mem, hipStream_t s) {
    if (!gemm_split3_persist_narrow_ok(a) || ws_mem == nullptr || (a.ksplit > 1 && epi != EPI_NONE)) return -1;
    return launch_split16_persist(a, epi, ws_mem, true, s);
}

// split-K through the 128 x 128 stream: the arguments of launch_gemm_split3_splitk (raw partial sums of K slice sp into part[sp][M][N])
int launch_gemm_split3_splitk_stream(const GemmArgs& a0, int ksplit, float* part, void* ws_mem, hipStream_t s) {
    if (ksplit < 2 || part == nullptr) return -1;
    GemmArgs a = a0;
    a.ksplit = ksplit;
    a.C = part; a.ldc = a.N;
    a.bias = nullptr; a.resid = nullptr; a.ldr = 0;
    return launch_gemm_split3_persist_narrow(a, EPI_NONE, ws_mem, s);
}

// the workspace's error word (a consumer's bounded spin ran out): 0 = none.  Synchronises the stream.
int gemm_split3_persist_error(void* ws_mem, hipStream_t s, unsigned* err_out) {
    unsigned* flag = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(ws_mem) + (size_t)P_NWG * P_SLAB * 4);
    if (hipMemcpyAsync(err_out, flag + P_NWG, sizeof(unsigned), hipMemcpyDeviceToHost, s) != hipSuccess) return -2;
    if (hipStreamSynchronize(s) != hipSuccess) return -2;
    return 0;
}

// the host-mapped word a timed-out consumer also writes: *host_err_slot = its device-visible address (the slot must outlive the copy: the
// engine keeps it in its struct).  Enqueued on `s` behind the memset that zeroed the workspace.
int gemm_split3_persist_bind_host_err(void* ws_mem, unsigned* const* host_err_slot, hipStream_t s) {
    unsigned* flag = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(ws_mem) + (size_t)P_NWG * P_SLAB * 4);
    static_assert(sizeof(unsigned*) == 8, "the workspace keeps the address in two words");
    return hipMemcpyAsync(flag + P_NWG + 4, host_err_slot, sizeof(unsigned*), hipMemcpyHostToDevice, s) == hipSuccess ? 0 : -2;
}

// grow-never workspace per (device, stream) for the stateless operators (thmr_op_gemm_split3 with a persistent variant)
void* gemm_split3_persist_op_ws(hipStream_t s) {
    static std::mutex mu;
    static std::map<std::pair<int, void*>, void*> pool;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::unique_lock<std::mutex> lk(mu);
    void*& p = pool[{dev, (void*)s}];
    if (!p) {
        if (hipMalloc(&p, gemm_split3_persist_ws_bytes()) != hipSuccess) { p = nullptr; return nullptr; }
        if (hipMemset(p, 0, gemm_split3_persist_ws_bytes()) != hipSuccess) { (void)hipFree(p); p = nullptr; return nullptr; }
    }
    return p;
}
