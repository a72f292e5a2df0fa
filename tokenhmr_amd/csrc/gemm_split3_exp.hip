// EXPERIMENTS build only (the shipped object of this file is empty): every split3 GEMM kernel on v_mfma_f32_32x32x16_bf16, six MFMAs per
// 16 k (operand format: split3_convert.hip).  Round 4 replaced them with the 16x16x32 kernels of gemm_split16.hip (another grouping of k
// inside the MFMA, so equal to rounding only); they stay for the A/B under their variant ids (op_gemm_variants.h).
//
// Per-tile kernel (gfx950): block tile (WM TM 32) x (WN TN 32), 8 waves of 64 x 64 on 128 x 256 by default, ONE workgroup per CU (two LDS
// stages of 72 KB), two waves per SIMD.
//   * staging: global_load_lds_dwordx4, saddr form (gemm_device.h); the LDS image of a stage is chunk-linear (row r = 12 chunks), and
//     since the LDS side of the copy is lane-linear the bank swizzle is applied to the SOURCE: physical slot p of row r holds logical
//     chunk (p - rot(r)) mod 12 with rot(r) = (r >> 2) & 3.  A row is 192 B = 48 banks, so the 16 lanes of one ds_read_b128 group
//     (16 consecutive rows, same logical chunk) would collide four ways; with the rotation they cover all 64 banks exactly once.
//   * per K tile and wave: 2 steps of 16 k; a step = 3 (TM + TN) ds_read_b128 and 6 TM TN MFMAs, accumulators walked round-robin.
//   * schedule of K tile kt (buffer kt & 1), no VALU instruction in the loop:
//       step 0 : MFMAs on fragment set 0, the reads of step 1's fragments in their shadow
//       barrier: this wave's copies of tile kt+1 (issued one step EARLIER, during step 1 of tile kt-1) have landed and its reads of
//                buffer kt & 1 have returned
//       step 1 : MFMAs on fragment set 1; in their shadow the reads of tile kt+1's step-0 fragments and the copies of tile kt+2 into
//                the buffer everybody just finished reading
//     so a copy has a whole step (>= 24 MFMAs of this wave plus its SIMD partner's) to land and no fragment read is exposed.
//
// Stream kernel: the same product (six v_mfma_f32_32x32x16_bf16 per 16 k) as PERSISTENT workgroups
// over a tile stream.  Same 128 x 256 tile, same 8 waves of 64 x 64, same LDS image and same K loop as gemm_split3_kernel — and the same
// bits: every output element is ONE accumulator chain over k = 0 ... K-1 in the same order, here too.  What changes is who runs which
// part of which tile, and when (vit.py:82-87,104-126 are the four products this serves at 32 crops and more).
//
// Why (profiles/r3ah_split3_kernel_stats.csv): with one workgroup per tile and one workgroup per CU the four ViT GEMMs of a
// 64-crop batch have 1440 / 480 / 1920 / 480 tiles for 256 CUs = 5.625 / 1.875 / 7.5 / 1.875 rounds — every one of them idles 6.25 % of
// the chip in a ragged last round — and every tile pays its own pipeline fill (two K tiles of LDS-DMA latency) and its own epilogue with
// nothing running underneath (fc1's GELU + split3 epilogue: 812 us against 716 us for the same tiles at the qkv rate).
//
// Decomposition.  256 workgroups (one per CU), workgroup b = (xcd = b & 7, lane = b >> 3).  Lane i of the eight XCDs owns the tile list
// {i, i + 32, i + 64, ...} in the XCD-aware logical order of gemm_device.h::tile_coords — T_i tiles of nk K tiles each = T_i nk steps, cut into
// eight equal consecutive step ranges, one per XCD.  So the 32 workgroups of an XCD walk 32 NEIGHBOURING tiles (8 x 4: the L2 footprint of
// gemm_split3_kernel's dispatch order) in lockstep, all with the same range boundaries, and a tile that straddles a boundary is split ALONG K
// between the same lane of two neighbouring XCDs.
//
// The K split keeps the association: the first part (k tiles [0, p)) is computed by XCD x as the FIRST thing it does, its raw fp32
// accumulators go to a workspace slab (write-through stores) and a flag is published; XCD x + 1 runs the rest (k tiles [p, nk)) as the LAST
// thing it does, starting from those accumulators instead of zeros — the accumulator chain merely travels through memory, bit for bit.
// (Summing two independently accumulated halves would be another association: a crop's result would depend on which tile it lands in.)
// The producer never waits for anybody and the consumer needs the slab some hundred microseconds after it was written, so the spin on the
// flag is nominal; it is bounded all the same (error word, no hang).  Placement-independent: cdna_hip_programming.md Guideline 16, R1 form
// (sc1 payload stores, every storing wave drains before a workgroup barrier, one lane publishes; sc1 loads on the consumer).
//
// Pipeline.  The two-stage LDS-DMA pipeline runs ACROSS tile boundaries: while the last K tiles of one tile are multiplied the first two K
// tiles of the next one are already being copied, the epilogue's stores drain under the next tile's MFMAs, and the only exposed cost per
// tile is the epilogue's own VALU work.  For a split3 OUTPUT (fc1: GELU, then three bf16 pieces per value, 8 consecutive columns per
// 16-byte chunk) that requires an epilogue that leaves the stage buffers alone: MODE 2 multiplies with the operand ROLES swapped (the MFMA's
// "A" is the weight fragment), which leaves a lane with one ROW of the output and 4-column groups in its registers, and eight
// v_permlane32_swap per accumulator turn those into two groups of 8 consecutive columns — no LDS, no barrier.  MODE 1 keeps the LDS
// transposition of gemm_split3_kernel (coalesced 384-byte row pieces) and pays a pipeline drain + refill per tile for it.
#include "common.h"
#include "gemm_device.h"
#include "gemm_split_device.h"

#ifdef THMR_EXPERIMENTS

namespace {

// ABL (timing-only experiments, results are garbage): bit0 no copies in the loop, bit1 no per-tile barrier, bit2 no fragment reads.
// RS: step 0 issues one fragment read every RS-th MFMA (0 = as early as possible: one per MFMA).
// ABLK: A is a ROW-BLOCKED split3 operand (GemmArgs::a_blk): its stage image in LDS is the memory image, [block of 32 rows][12 chunks of the K
// tile][32 rows][16 B] — linear copies, fragment reads of 512 contiguous bytes per 32 lanes (no swizzle needed).
template <int WM, int WN, int TM, int TN, int EPI, int ABL = 0, int RS = 0, bool ABLK = false>
__global__ __launch_bounds__(WM * WN * 64) void gemm_split3_kernel(GemmArgs a, int tiles_m, int tiles_n, int nwg) {
    constexpr int NW = WM * WN;
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    constexpr int A_Q = BM * SLOTS / 64, B_Q = BN * SLOTS / 64;       // wave instructions (1 KiB each) per stage
    static_assert(A_Q % NW == 0 && B_Q % NW == 0, "tile / waves mismatch");
    constexpr int A_P = A_Q / NW, B_P = B_Q / NW, NP = A_P + B_P;     // copies per wave and K tile
    constexpr int A_STAGE = BM * ROWB, B_STAGE = BN * ROWB;
    static_assert(2 * (A_STAGE + B_STAGE) <= 160 * 1024, "LDS");

    __shared__ __attribute__((aligned(16))) char smem[2 * (A_STAGE + B_STAGE)];
    char* As = smem;                       // [2][BM][192]
    char* Bs = smem + 2 * A_STAGE;         // [2][BN][192]

    int tile_m, tile_n;
    int logical = logical_block(nwg, 0);
    int nk = a.K / SBK;
    int ksp = 0;
    if (a.ksplit > 1) {      // split-K: this block belongs to copy ksp of the tile grid and reduces K slice ksp into part[ksp] (wave-uniform)
        const int tiles = tiles_m * tiles_n;
        ksp = logical / tiles;
        logical -= ksp * tiles;
        nk /= a.ksplit;
        a.C += (int64_t)ksp * a.M * a.ldc;
    }
    tile_coords(tiles_m, tiles_n, logical, tile_m, tile_n);
    const int bm0 = tile_m * BM, bn0 = tile_n * BN;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wave / WN) * TM * 32;
    const int wn0 = (wave % WN) * TN * 32;
    const int lrow = lane & 31, lhalf = lane >> 5;

    // ---- copies: wave instruction q = wave + i NW of an operand fills LDS chunks 64 q ... 64 q + 63 of its stage; lane -> chunk c,
    // row c / 12, physical slot c % 12, which holds logical chunk (slot - rot(row)) mod 12.  Rows past the edge are clamped.
    const int64_t arow = a.lda * 6, wrow = a.ldw * 6;                  // bytes per matrix row
    constexpr int A_KSTEP = ABLK ? SLOTS * 512 : ROWB;               // bytes a K tile advances the A source by (per 32-row block / per row)
    const char* Abase = reinterpret_cast<const char*>(a.A) + (int64_t)bm0 * arow + (int64_t)ksp * nk * A_KSTEP;
    const char* Wbase = reinterpret_cast<const char*>(a.W) + (int64_t)bn0 * wrow + (int64_t)ksp * nk * ROWB;
    uint32_t Aoff[A_P], Woff[B_P];
#pragma unroll
    for (int i = 0; i < A_P; ++i) {
        const int c = (wave + i * NW) * 64 + lane;
        if constexpr (ABLK) {      // LDS chunk c = (block c / 384, chunk-of-the-K-tile (c % 384) / 32, row-in-block c % 32): the memory order
            const int row = (c / 384) * 32 + (c & 31), rg = min(bm0 + row, a.M - 1) - bm0;
            Aoff[i] = (uint32_t)(rg >> 5) * (uint32_t)(a.lda * 192) + (uint32_t)((c % 384) >> 5) * 512u + (uint32_t)(rg & 31) * 16u;
        } else {
            const int row = c / SLOTS, slot = c - row * SLOTS;
            const int j = (slot + SLOTS - ((row >> 2) & 3)) % SLOTS;
            Aoff[i] = (uint32_t)(min(bm0 + row, a.M - 1) - bm0) * (uint32_t)arow + (uint32_t)j * 16u;
        }
    }
#pragma unroll
    for (int i = 0; i < B_P; ++i) {
        const int c = (wave + i * NW) * 64 + lane, row = c / SLOTS, slot = c - row * SLOTS;
        const int j = (slot + SLOTS - ((row >> 2) & 3)) % SLOTS;
        Woff[i] = (uint32_t)(min(bn0 + row, a.N - 1) - bn0) * (uint32_t)wrow + (uint32_t)j * 16u;
    }
    auto dma_piece = [&](int kt, int buf, int p) {                     // p, buf: compile-time after unrolling
        // wave-uniform, added on the SALU
        if (p < A_P) dma16_saddr(Abase + (int64_t)kt * A_KSTEP, Aoff[p], lds_addr_b(As + buf * A_STAGE + (wave + p * NW) * 1024));
        else dma16_saddr(Wbase + (int64_t)kt * ROWB, Woff[p - A_P], lds_addr_b(Bs + buf * B_STAGE + (wave + (p - A_P) * NW) * 1024));
    };

    // ---- fragments: step s of a K tile multiplies k-groups 2 s (lanes 0-31) and 2 s + 1 (lanes 32-63); chunk j = 3 kgroup + piece
    // sits in physical slot (j + rot(row)) mod 12, rot(row) = (lrow >> 2) & 3 for every row this lane reads (tile offsets are x 32)
    uint32_t fo[2][3];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int pc = 0; pc < 3; ++pc)
            fo[s][pc] = (uint32_t)lrow * ROWB + (uint32_t)((((2 * s + lhalf) * 3 + pc) + ((lrow >> 2) & 3)) % SLOTS) * 16u;
    const char* Afr = As + wm0 * ROWB;                                 // (row-blocked A: wm0 / 32 blocks of 12 x 512 bytes = the same offset)
    const char* Bfr = Bs + wn0 * ROWB;
    uint32_t foa[2][3];                                                // A fragments of a row-blocked stage: chunk (k-group, piece) x 512 + row x 16
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) foa[s][pc] = ABLK ? (uint32_t)(((2 * s + lhalf) * 3 + pc) * 512 + lrow * 16) : fo[s][pc];

    bf16x8 af[2][TM][3], bf[2][TN][3];
    constexpr int NR = 3 * (TM + TN);                                  // fragment reads per step
    // read r of step s of the tile in buffer `buf` into fragment set `set`: A pieces first, in the order the products use them
    auto read_one = [&](int buf, int s, int set, int r) {
        if (r < 3 * TM) {
            const int mi = r / 3, pc = r % 3;
            af[set][mi][pc] = *reinterpret_cast<const bf16x8*>(Afr + buf * A_STAGE + mi * 32 * ROWB + foa[s][pc]);
        } else {
            const int q = r - 3 * TM, ni = q / 3, pc = q % 3;
            bf[set][ni][pc] = *reinterpret_cast<const bf16x8*>(Bfr + buf * B_STAGE + ni * 32 * ROWB + fo[s][pc]);
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // ---- prologue: tiles 0 and 1 in flight, tile 0's step-0 fragments in registers
#pragma unroll
    for (int p = 0; p < NP; ++p) dma_piece(0, 0, p);
#pragma unroll
    for (int p = 0; p < NP; ++p) dma_piece(min(1, nk - 1), 1, p);
    dma_wait_barrier();
#pragma unroll
    for (int r = 0; r < NR; ++r) read_one(0, 0, 0, r);

    constexpr int G = NPROD * TM * TN;                                 // MFMAs per step
    constexpr int RS0 = RS > 0 ? RS : 1;                               // step 0: one read every RS0-th MFMA
    static_assert(NR * RS0 <= G && NR + NP <= G, "tile too small for the staging interleave");

    auto ktile = [&](int kt, auto bufc) {
        constexpr int buf = decltype(bufc){};
        const int kt2 = min(kt + 2, nk - 1);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (s == 1 && !(ABL & 2)) {
                __builtin_amdgcn_sched_barrier(0);
                dma_wait_barrier();
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int p = 0; p < NPROD; ++p)
#pragma unroll
                for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                    for (int ni = 0; ni < TN; ++ni) {
                        const int idx = (p * TM + mi) * TN + ni;
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s][mi][piece_a(p)], bf[s][ni][piece_w(p)],
                                                                              acc[mi][ni], 0, 0, 0);
                        bool any = false;
                        if (s == 0) {
                            if (idx % RS0 == 0 && idx / RS0 < NR && !(ABL & 4)) { read_one(buf, 1, 1, idx / RS0); any = true; }
                        } else {
                            if (idx < NR) { if (!(ABL & 4)) { read_one(buf ^ 1, 0, 0, idx); any = true; } }
                            else if (idx - NR < NP && !(ABL & 1)) { dma_piece(kt2, buf, idx - NR); any = true; }
                        }
                        if (any) __builtin_amdgcn_sched_barrier(0);
                    }
        }
    };
    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
        ktile(kt, IntC<0>{});
        ktile(kt + 1, IntC<1>{});
    }
    if (kt < nk) ktile(kt, IntC<0>{});
    if constexpr ((ABL & 4) != 0) {
#pragma unroll
        for (int st = 0; st < 2; ++st) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int pc = 0; pc < 3; ++pc) asm volatile("" : "+v"(af[st][i][pc]));
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int pc = 0; pc < 3; ++pc) asm volatile("" : "+v"(bf[st][i][pc]));
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                   // no LDS-DMA write may outlive the workgroup's LDS allocation

    if (a.c_split) {                        // wave-uniform: the result as the next GEMM's split3 operand
        constexpr int WT = TN * 32 + 4;
        static_assert(NW * TM * 32 * WT * 4 <= 2 * (A_STAGE + B_STAGE), "transpose tile does not fit the stage buffers");
        __syncthreads();                                               // every wave is done reading the stage buffers
        store_tile_split3<TM, TN, EPI>(a, acc, reinterpret_cast<float*>(smem) + wave * (TM * 32 * WT), bm0 + wm0, bn0 + wn0, lane);
        return;
    }
    store_tile<TM, TN, EPI>(a, acc, bm0 + wm0, bn0 + wn0, lrow, lhalf);
}

// ---------------------------------------------------------------------------------------------------------------------
// Small-M split3 GEMM (few crops: the engine's split3 mode up to six crops) — the ring kernel of gemm_f32.hip on split3 operands:
// 64 x 64 tiles (2 x 2 waves of 32 x 32), ST-deep LDS ring of 24 KB stages fed by global_load_lds whose completion is tracked with
// s_waitcnt vmcnt(N), ONE barrier per 32-deep K tile in the middle of its 12 MFMAs, optional split-K into part[ksplit][M][N] (raw fp32
// partial tiles, summed in a fixed order by the residual + LayerNorm kernel that follows proj / fc2 anyway).  Per element K is summed
// in the order of gemm_split3_kernel (per 16 k: lh hl mm mh hm hh), so without split-K the two kernels are bit-identical.  A wave's
// chain is 12 MFMAs of 32 cycles per K tile instead of the fp32 ring kernel's 16 of 64: 0.375 of its matrix time.
template <int ST, int EPI, bool PARTIAL>
__global__ __launch_bounds__(256) void gemm_split3_ring_kernel(GemmArgs a, int tiles_m, int groups, int ksplit, float* part) {
    constexpr int NPW = 6;                                  // copies per wave and K tile (3 for A, 3 for W)
    constexpr int STAGE = 64 * ROWB;                        // 12 KB per operand and stage
    static_assert((ST & (ST - 1)) == 0 && ST >= 4, "ring depth must be a power of two >= 4");
    __shared__ __attribute__((aligned(16))) char smem[ST * 2 * STAGE];
    char* As = smem;                       // [ST][64][192]
    char* Bs = smem + ST * STAGE;          // [ST][64][192]

    const int xcd = blockIdx.x & 7, within = blockIdx.x >> 3;
    const int gl = within / tiles_m, tile_m = within - gl * tiles_m;
    const int g = gl * 8 + xcd;
    if (g >= groups) return;
    const int tile_n = g / ksplit, sp = g - tile_n * ksplit;
    const int bm0 = tile_m * 64, bn0 = tile_n * 64;
    const int kper = a.K / ksplit, kbeg = sp * kper, nk = kper / SBK;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;
    const int lrow = lane & 31, lhalf = lane >> 5;

    const int64_t arow = a.lda * 6, wrow = a.ldw * 6;
    const char* Abase = reinterpret_cast<const char*>(a.A) + (int64_t)bm0 * arow + (int64_t)(kbeg >> 3) * 48;
    const char* Wbase = reinterpret_cast<const char*>(a.W) + (int64_t)bn0 * wrow + (int64_t)(kbeg >> 3) * 48;
    uint32_t Aoff[3], Woff[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const int c = (wave + 4 * p) * 64 + lane, row = c / SLOTS, slot = c - row * SLOTS;
        const int j = (slot + SLOTS - ((row >> 2) & 3)) % SLOTS;
        Aoff[p] = (uint32_t)(min(bm0 + row, a.M - 1) - bm0) * (uint32_t)arow + (uint32_t)j * 16u;
        Woff[p] = (uint32_t)(min(bn0 + row, a.N - 1) - bn0) * (uint32_t)wrow + (uint32_t)j * 16u;
    }
    auto dma_tile = [&](int kt, auto stc) {      // K tile kt -> ring slot stc (= kt % ST, an integral constant)
        constexpr int st = decltype(stc){};
        const int64_t k0b = (int64_t)kt * ROWB;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            dma16_saddr(Abase + k0b, Aoff[p], lds_addr_b(As + st * STAGE + (wave + 4 * p) * 1024));
            dma16_saddr(Wbase + k0b, Woff[p], lds_addr_b(Bs + st * STAGE + (wave + 4 * p) * 1024));
        }
    };
    uint32_t fo[2][3];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int pc = 0; pc < 3; ++pc)
            fo[s][pc] = (uint32_t)lrow * ROWB + (uint32_t)((((2 * s + lhalf) * 3 + pc) + ((lrow >> 2) & 3)) % SLOTS) * 16u;
    const char* Afr = As + wm0 * ROWB;
    const char* Bfr = Bs + wn0 * ROWB;
    bf16x8 af[2][3], bf[2][3];
    auto read_frags = [&](auto stc, int s, int set) {
        constexpr int st = decltype(stc){};
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) {
            af[set][pc] = *reinterpret_cast<const bf16x8*>(Afr + st * STAGE + fo[s][pc]);
            bf[set][pc] = *reinterpret_cast<const bf16x8*>(Bfr + st * STAGE + fo[s][pc]);
        }
    };
    f32x16 acc[1][1];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[0][0][e] = 0.f;
    // one step of 16 k: product 0, then the fragment reads of the NEXT step (nxt() may be empty) in the shadow of products 1-5
    auto step = [&](int set, auto nxt) {
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[set][piece_a(0)], bf[set][piece_w(0)], acc[0][0], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        nxt();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int p = 1; p < NPROD; ++p)
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[set][piece_a(p)], bf[set][piece_w(p)], acc[0][0], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    };

    // prologue: K tiles 0 .. ST-2 in flight; tile 0 must have landed (for every wave) before the first fragment read
    static_for<ST - 1>([&](auto t) {
        if (t < nk) dma_tile(t, t);
    });
    if (nk >= ST - 1) wait_vm_barrier<(ST - 2) * NPW>(); else wait_vm_barrier<0>();
    read_frags(IntC<0>{}, 0, 0);

    auto tile = [&](int kt, auto stc, bool last) {      // stc = kt % ST; `last` is a literal at every call site
        constexpr int S = decltype(stc){};
        step(0, [&] { read_frags(stc, 1, 1); });
        if (!last) {
            // tile kt+1 landed (in-order completion: at most the ST-3 younger tiles may still be in flight); after the barrier every
            // wave is past tile kt-1, whose ring slot receives tile kt+ST-1
            if (kt + ST - 2 < nk) wait_vm_barrier<(ST - 3) * NPW>(); else wait_vm_barrier<0>();
            if (kt + ST - 1 < nk) dma_tile(kt + ST - 1, IntC<(S + ST - 1) % ST>{});
        }
        step(1, [&] { if (!last) read_frags(IntC<(S + 1) % ST>{}, 0, 0); });
    };
    int kt = 0;
    for (; kt + ST <= nk - 1; kt += ST) static_for<ST>([&](auto sc) { tile(kt + sc, sc, false); });
    static_for<ST>([&](auto sc) {            // < ST tiles left before the last one; kt is a multiple of ST
        if (kt + sc < nk - 1) tile(kt + sc, sc, false);
    });
    static_for<ST>([&](auto sc) {
        if (((nk - 1) & (ST - 1)) == sc) tile(nk - 1, sc, true);
    });

    if constexpr (PARTIAL) {
        GemmArgs pa = a;
        pa.C = part + (int64_t)sp * a.M * a.N;
        pa.ldc = a.N;
        store_tile<1, 1, EPI_NONE>(pa, acc, bm0 + wm0, bn0 + wn0, lrow, lhalf);
    } else {
        if (a.c_split) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();                                           // every wave is done reading the ring
            store_tile_split3<1, 1, EPI>(a, acc, reinterpret_cast<float*>(smem) + wave * (32 * 36), bm0 + wm0, bn0 + wn0, lane);
            return;
        }
        store_tile<1, 1, EPI>(a, acc, bm0 + wm0, bn0 + wn0, lrow, lhalf);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// 256 x 256 block tile, 4 waves of 128 x 128 (ONE wave per SIMD, 256 accumulator registers), 16-deep stages — fewer LDS bytes per MFMA:
// a step needs 24 ds_read_b128 for 96 MFMAs (0.25 per MFMA against the 64 x 64 wave tile's 0.5) and the tile 125 B of copies per MFMA
// (192).  The schedule ablation of the 128 x 256 kernel prices the fragment reads at 20 % and the copies at 12.5 % of its time
// (profiles/r3v_split3_schedule_ablation.jsonl); this variant trades that against having no second wave per SIMD.
// A stage is 512 rows x 96 B = 48 KB (two stages); 6 chunks per row = 24 banks, rows r and r + 8 of a ds_read_b128 lane group collide,
// hence rot(r) = (r >> 3) & 1.  Per K tile (one step of 16 k): the copies of tile kt + 2 into the buffer whose fragments were read during
// the previous tile, the reads of tile kt + 1's fragments from the other buffer, 96 MFMAs; barrier.  Same K order per element as the other
// tiles (per 16 k: lh hl mm mh hm hh) -> bit-identical results.
template <int EPI>
__global__ __launch_bounds__(256) void gemm_split3_wide_kernel(GemmArgs a, int tiles_m, int tiles_n, int nwg) {
    constexpr int TM = 4, TN = 4, WN = 2, NW = 4, BM = 256, BN = 256;
    constexpr int WSLOTS = 6, WROWB = 96;                             // 16 k: 2 k-groups x 3 pieces
    constexpr int A_STAGE = BM * WROWB, B_STAGE = BN * WROWB;         // 24 KB each
    constexpr int A_P = BM * WSLOTS / 64 / NW, B_P = BN * WSLOTS / 64 / NW, NP = A_P + B_P;     // 6 + 6 copies per wave and tile
    __shared__ __attribute__((aligned(16))) char smem[2 * (A_STAGE + B_STAGE)];
    char* As = smem;
    char* Bs = smem + 2 * A_STAGE;

    int tile_m, tile_n;
    tile_coords(tiles_m, tiles_n, logical_block(nwg, 0), tile_m, tile_n);
    const int bm0 = tile_m * BM, bn0 = tile_n * BN;
    const int nk = a.K / 16;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wave / WN) * TM * 32, wn0 = (wave % WN) * TN * 32;
    const int lrow = lane & 31, lhalf = lane >> 5;

    const int64_t arow = a.lda * 6, wrow = a.ldw * 6;
    const char* Abase = reinterpret_cast<const char*>(a.A) + (int64_t)bm0 * arow;
    const char* Wbase = reinterpret_cast<const char*>(a.W) + (int64_t)bn0 * wrow;
    uint32_t Aoff[A_P], Woff[B_P];
#pragma unroll
    for (int i = 0; i < A_P; ++i) {
        const int c = (wave + i * NW) * 64 + lane, row = c / WSLOTS, slot = c - row * WSLOTS;
        const int j = (slot + WSLOTS - ((row >> 3) & 1)) % WSLOTS;
        Aoff[i] = (uint32_t)(min(bm0 + row, a.M - 1) - bm0) * (uint32_t)arow + (uint32_t)j * 16u;
        Woff[i] = (uint32_t)(min(bn0 + row, a.N - 1) - bn0) * (uint32_t)wrow + (uint32_t)j * 16u;
    }
    auto dma_piece = [&](int kt, int buf, int p) {
        const int64_t k0b = (int64_t)kt * WROWB;
        if (p < A_P) dma16_saddr(Abase + k0b, Aoff[p], lds_addr_b(As + buf * A_STAGE + (wave + p * NW) * 1024));
        else dma16_saddr(Wbase + k0b, Woff[p - A_P], lds_addr_b(Bs + buf * B_STAGE + (wave + (p - A_P) * NW) * 1024));
    };
    uint32_t fo[3];
#pragma unroll
    for (int pc = 0; pc < 3; ++pc)
        fo[pc] = (uint32_t)lrow * WROWB + (uint32_t)(((lhalf * 3 + pc) + ((lrow >> 3) & 1)) % WSLOTS) * 16u;
    const char* Afr = As + wm0 * WROWB;
    const char* Bfr = Bs + wn0 * WROWB;
    bf16x8 af[2][TM][3], bf[2][TN][3];
    constexpr int NR = 3 * (TM + TN);
    auto read_one = [&](int buf, int set, int r) {
        if (r < 3 * TM) {
            const int mi = r / 3, pc = r % 3;
            af[set][mi][pc] = *reinterpret_cast<const bf16x8*>(Afr + buf * A_STAGE + mi * 32 * WROWB + fo[pc]);
        } else {
            const int q = r - 3 * TM, ni = q / 3, pc = q % 3;
            bf[set][ni][pc] = *reinterpret_cast<const bf16x8*>(Bfr + buf * B_STAGE + ni * 32 * WROWB + fo[pc]);
        }
    };
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

#pragma unroll
    for (int p = 0; p < NP; ++p) dma_piece(0, 0, p);
#pragma unroll
    for (int p = 0; p < NP; ++p) dma_piece(min(1, nk - 1), 1, p);
    dma_wait_barrier();
#pragma unroll
    for (int r = 0; r < NR; ++r) read_one(0, 0, r);

    auto ktile = [&](int kt, auto bufc) {
        constexpr int buf = decltype(bufc){};                        // buffer and fragment set of tile kt
        const int kt2 = min(kt + 2, nk - 1);
#pragma unroll
        for (int p = 0; p < NPROD; ++p)
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) {
                    const int idx = (p * TM + mi) * TN + ni;
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[buf][mi][piece_a(p)], bf[buf][ni][piece_w(p)], acc[mi][ni], 0, 0, 0);
                    bool any = false;
                    if (idx < NP) { dma_piece(kt2, buf, idx); any = true; }
                    else if (idx - NP < NR) { read_one(buf ^ 1, buf ^ 1, idx - NP); any = true; }
                    if (any) __builtin_amdgcn_sched_barrier(0);
                }
        __builtin_amdgcn_sched_barrier(0);
        dma_wait_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
        ktile(kt, IntC<0>{});
        ktile(kt + 1, IntC<1>{});
    }
    if (kt < nk) ktile(kt, IntC<0>{});

    if (a.c_split) {
        // one 32-row slice of the wave tile at a time through a wave-private 32 x 132 fp32 tile (the stage buffers are dead)
        constexpr int WT = TN * 32 + 4;
        static_assert(NW * 32 * WT * 4 <= 2 * (A_STAGE + B_STAGE), "transpose tile does not fit the stage buffers");
        float* T = reinterpret_cast<float*>(smem) + wave * (32 * WT);
        static_for<TM>([&](auto mic) {
            constexpr int mi = decltype(mic){};
            store_tile_split3<1, TN, EPI>(a, reinterpret_cast<f32x16(&)[1][TN]>(acc[mi]), T, bm0 + wm0 + mi * 32, bn0 + wn0, lane);
        });
        return;
    }
    store_tile<TM, TN, EPI>(a, acc, bm0 + wm0, bn0 + wn0, lrow, lhalf);
}

template <int WM, int WN, int TM, int TN, int ABL, int RS>
int launch_split3_abl(const GemmArgs& a, hipStream_t s) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const int tiles_m = (a.M + BM - 1) / BM, tiles_n = (a.N + BN - 1) / BN, nwg = tiles_m * tiles_n;
    hipLaunchKernelGGL((gemm_split3_kernel<WM, WN, TM, TN, EPI_NONE, ABL, RS>), dim3(nwg), dim3(WM * WN * 64), 0, s, a, tiles_m, tiles_n, nwg);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_split3_wide(const GemmArgs& a, int epi, hipStream_t s) {
    if (a.ksplit > 1 || a.a_blk) return -1;
    const int tiles_m = (a.M + 255) / 256, tiles_n = (a.N + 255) / 256, nwg = tiles_m * tiles_n;
    const dim3 grid(nwg), block(256);
#define THMR_WIDE_CASE(E)                                                                                       \
    case E:                                                                                                     \
        hipLaunchKernelGGL((gemm_split3_wide_kernel<E>), grid, block, 0, s, a, tiles_m, tiles_n, nwg);          \
        break;
    switch (epi) {
        THMR_WIDE_CASE(EPI_NONE)
        THMR_WIDE_CASE(EPI_BIAS)
        THMR_WIDE_CASE(EPI_BIAS_GELU)
        THMR_WIDE_CASE(EPI_BIAS_RESID)
        THMR_WIDE_CASE(EPI_BIAS_QSCALE)
        default: return -1;
    }
#undef THMR_WIDE_CASE
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

template <int WM, int WN, int TM, int TN>
int launch_split3_cfg(const GemmArgs& a, int epi, hipStream_t s) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const int tiles_m = (a.M + BM - 1) / BM, tiles_n = (a.N + BN - 1) / BN, nwg = tiles_m * tiles_n * (a.ksplit > 1 ? a.ksplit : 1);
    const dim3 grid(nwg), block(WM * WN * 64);
    if (a.a_blk) {      // row-blocked A (fc2's operand): the two epilogues fc2 runs with — raw split-K partials and bias + residual
        if (epi == EPI_NONE) hipLaunchKernelGGL((gemm_split3_kernel<WM, WN, TM, TN, EPI_NONE, 0, 0, true>), grid, block, 0, s, a, tiles_m, tiles_n, nwg);
        else if (epi == EPI_BIAS_RESID) hipLaunchKernelGGL((gemm_split3_kernel<WM, WN, TM, TN, EPI_BIAS_RESID, 0, 0, true>), grid, block, 0, s, a, tiles_m, tiles_n, nwg);
        else return -1;
        return hipGetLastError() == hipSuccess ? 0 : -2;
    }
#define THMR_SPLIT_CASE(E)                                                                                                  \
    case E:                                                                                                                 \
        hipLaunchKernelGGL((gemm_split3_kernel<WM, WN, TM, TN, E>), grid, block, 0, s, a, tiles_m, tiles_n, nwg);    \
        break;
    switch (epi) {
        THMR_SPLIT_CASE(EPI_NONE)
        THMR_SPLIT_CASE(EPI_BIAS)
        THMR_SPLIT_CASE(EPI_BIAS_GELU)
        THMR_SPLIT_CASE(EPI_BIAS_RESID)
        THMR_SPLIT_CASE(EPI_BIAS_QSCALE)
        default: return -1;
    }
#undef THMR_SPLIT_CASE
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

struct PersistWs {
    float* part;        // [8 * PG] slabs of P_SLAB floats: slab (x, i) = first part of the tile shared by lane i of XCDs x and x + 1
    unsigned* flag;     // [8 * PG] 0 / 1, set by the producer, cleared by the consumer (stream order separates launches); [8 * PG] = error word
};

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

// MODE 2 epilogue: acc[mi][ni] holds the TRANSPOSED 32 x 32 tile (lane & 31 = row m of the output, registers = columns n:
// n = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)).  v_permlane32_swap(X = reg j of column block g, Y = reg j of block g + 1) exchanges X's upper
// 32 lanes with Y's lower 32: afterwards lanes 0-31 hold columns 8 h ... 8 h + 7 of blocks (g, g + 1) = 16 g' + 0 ... 7 and lanes 32-63
// columns 16 g' + 8 ... 15.  Then bias + activation + split3 per value and three 16-byte stores (48 contiguous bytes) per group.
template <int TM, int TN, int EPI>
__device__ __forceinline__ void store_tile_split3_swapped(const GemmArgs& a, f32x16 (&acc)[TM][TN], int m0, int n0, int lane) {
    const int lrow = lane & 31, lhalf = lane >> 5;
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
        const int m = m0 + mi * 32 + lrow;
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
#pragma unroll
            for (int gp = 0; gp < 2; ++gp) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const u32x2_t sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[mi][ni][8 * gp + j]),
                                                                       __float_as_uint(acc[mi][ni][8 * gp + 4 + j]), false, false);
                    v[j] = __uint_as_float(sw.x);
                    v[4 + j] = __uint_as_float(sw.y);
                }
                const int n = n0 + ni * 32 + gp * 16 + lhalf * 8;
                float bias[8];
                if constexpr (EPI != EPI_NONE) {
                    const f32x4 b0 = *reinterpret_cast<const f32x4*>(a.bias + n), b1 = *reinterpret_cast<const f32x4*>(a.bias + n + 4);
                    bias[0] = b0[0]; bias[1] = b0[1]; bias[2] = b0[2]; bias[3] = b0[3];
                    bias[4] = b1[0]; bias[5] = b1[1]; bias[6] = b1[2]; bias[7] = b1[3];
                } else {
#pragma unroll
                    for (int u = 0; u < 8; ++u) bias[u] = 0.f;
                }
                if constexpr (EPI == EPI_BIAS_GELU) {
#pragma unroll
                    for (int u = 0; u < 8; u += 2) {
                        const f32x2 gl = gelu_erf2(f32x2{v[u] + bias[u], v[u + 1] + bias[u + 1]});
                        v[u] = gl.x;
                        v[u + 1] = gl.y;
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = gemm_epilogue<EPI>(a, v[u], bias[u], m, n + u);
                }
                uint32_t H[4], M[4], L[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) split3_pair(v[2 * u], v[2 * u + 1], H[u], M[u], L[u]);
                char* cb = reinterpret_cast<char*>(a.c_split);
                const bool blk = a.cs_blk != 0;
                *reinterpret_cast<u32x4*>(cb + split3_chunk_off(a.ldcs, m, n >> 3, 0, blk)) = u32x4{H[0], H[1], H[2], H[3]};
                *reinterpret_cast<u32x4*>(cb + split3_chunk_off(a.ldcs, m, n >> 3, 1, blk)) = u32x4{M[0], M[1], M[2], M[3]};
                *reinterpret_cast<u32x4*>(cb + split3_chunk_off(a.ldcs, m, n >> 3, 2, blk)) = u32x4{L[0], L[1], L[2], L[3]};
            }
        }
    }
}

// MODE: 0 = fp32 output (store_tile), pipeline continuous across tiles
//       1 = split3 output through the LDS transposition (store_tile_split3): pipeline drained and refilled per tile
//       2 = split3 output with swapped operand roles + v_permlane32_swap: pipeline continuous
// ABLK: A is a row-blocked split3 operand (GemmArgs::a_blk; see gemm_split3_kernel)
template <int EPI, int MODE, bool ABLK = false>
__global__ __launch_bounds__(512) void gemm_split3_persist_kernel(GemmArgs a, int tiles_m, int tiles_n, PersistWs ws) {
    constexpr int NW = 8, WN = 4, TM = 2, TN = 2;
    constexpr bool SWAP = MODE == 2, CONT = MODE != 1;
    constexpr int A_Q = PBM * SLOTS / 64, B_Q = PBN * SLOTS / 64;
    constexpr int A_P = A_Q / NW, B_P = B_Q / NW, NP = A_P + B_P;      // 3 + 6 copies per wave and K tile
    constexpr int A_STAGE = PBM * ROWB, B_STAGE = PBN * ROWB;
    static_assert(2 * (A_STAGE + B_STAGE) <= 160 * 1024, "LDS");

    __shared__ __attribute__((aligned(16))) char smem[2 * (A_STAGE + B_STAGE)];
    char* As = smem;
    char* Bs = smem + 2 * A_STAGE;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wave / WN) * TM * 32;
    const int wn0 = (wave % WN) * TN * 32;
    const int lrow = lane & 31, lhalf = lane >> 5;

    // ---- this workgroup's step range of its lane's tile list, as segments: [first part of a shared tile] [whole tiles] [rest of a shared tile]
    const int xcd = blockIdx.x & 7, ln = blockIdx.x >> 3;
    const int nk = a.K / SBK;
    const int T = (tiles_m * tiles_n - ln + PG - 1) / PG;              // >= 8 (launcher)
    const int S0 = (int)((int64_t)xcd * T * nk / 8), S1 = (int)((int64_t)(xcd + 1) * T * nk / 8);
    const int j0 = S0 / nk, k0 = S0 - j0 * nk;
    const int j1 = (S1 - 1) / nk, k1 = S1 - j1 * nk;
    const int has_pre = k1 < nk ? 1 : 0, has_post = k0 > 0 ? 1 : 0;    // a range is >= nk steps long, so the two are never the same tile
    const int jf0 = j0 + has_post, nfull = max(j1 - has_pre - jf0 + 1, 0);
    const int nseg = has_pre + nfull + has_post;
    // segment n -> tile j of the lane's list, K tiles [kb, ke), kind 0 whole / 1 first part (store the accumulators) / 2 rest (load them)
    auto seg_of = [&](int n, int& j, int& kb, int& ke, int& kind) {
        const int m = n - has_pre;
        if (has_pre && n == 0) { j = j1; kb = 0; ke = k1; kind = 1; }
        else if (m < nfull) { j = jf0 + m; kb = 0; ke = nk; kind = 0; }
        else { j = j0; kb = k0; ke = nk; kind = 2; }
    };
    auto tile_of = [&](int j, int& bm0, int& bn0) {
        int tm, tn;
        tile_coords(tiles_m, tiles_n, j * PG + ln, tm, tn);
        bm0 = __builtin_amdgcn_readfirstlane(tm * PBM);              // wave-uniform by construction (blockIdx and kernel arguments only)
        bn0 = __builtin_amdgcn_readfirstlane(tn * PBN);
    };

    // ---- copies (M % 128 == 0 and N % 256 == 0: no clamping, the lane offsets are the same for every tile)
    const int64_t arow = a.lda * 6, wrow = a.ldw * 6;
    uint32_t Aoff[A_P], Woff[B_P];
#pragma unroll
    for (int i = 0; i < A_P; ++i) {
        const int c = (wave + i * NW) * 64 + lane;
        if constexpr (ABLK) {
            Aoff[i] = (uint32_t)(c / 384) * (uint32_t)(a.lda * 192) + (uint32_t)(c % 384) * 16u;       // linear within a 32-row block
        } else {
            const int row = c / SLOTS, slot = c - row * SLOTS;
            Aoff[i] = (uint32_t)row * (uint32_t)arow + (uint32_t)((slot + SLOTS - ((row >> 2) & 3)) % SLOTS) * 16u;
        }
    }
    constexpr int A_KSTEP = ABLK ? SLOTS * 512 : ROWB;               // bytes a K tile advances the A source by
#pragma unroll
    for (int i = 0; i < B_P; ++i) {
        const int c = (wave + i * NW) * 64 + lane, row = c / SLOTS, slot = c - row * SLOTS;
        Woff[i] = (uint32_t)row * (uint32_t)wrow + (uint32_t)((slot + SLOTS - ((row >> 2) & 3)) % SLOTS) * 16u;
    }
    // fetch cursor: the K tile the NEXT copy brings in (two ahead of the multiply), wave-uniform
    int fn = 0, fk = 0, fke = 0;
    const char *fA = nullptr, *fW = nullptr;
    auto fetch_seg = [&](int n) {
        int j, kb, ke, kind, bm0, bn0;
        seg_of(n, j, kb, ke, kind);
        tile_of(j, bm0, bn0);
        fk = kb;
        fke = ke;
        fA = reinterpret_cast<const char*>(a.A) + (int64_t)bm0 * arow + (int64_t)kb * A_KSTEP;
        fW = reinterpret_cast<const char*>(a.W) + (int64_t)bn0 * wrow + (int64_t)kb * ROWB;
    };
    auto fetch_advance = [&]() {
        if (fk + 1 < fke) { ++fk; fA += A_KSTEP; fW += ROWB; }
        else if (CONT && fn + 1 < nseg) fetch_seg(++fn);
        // else: past the end (of the segment in MODE 1): the last K tile is copied again, into a buffer nobody reads any more
    };
    auto dma_piece = [&](int buf, int p) {
        if (p < A_P) dma16_saddr(fA, Aoff[p], lds_addr_b(As + buf * A_STAGE + (wave + p * NW) * 1024));
        else dma16_saddr(fW, Woff[p - A_P], lds_addr_b(Bs + buf * B_STAGE + (wave + (p - A_P) * NW) * 1024));
    };

    // ---- fragments (as gemm_split3_kernel)
    uint32_t fo[2][3];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int pc = 0; pc < 3; ++pc)
            fo[s][pc] = (uint32_t)lrow * ROWB + (uint32_t)((((2 * s + lhalf) * 3 + pc) + ((lrow >> 2) & 3)) % SLOTS) * 16u;
    const char* Afr = As + wm0 * ROWB;
    const char* Bfr = Bs + wn0 * ROWB;
    uint32_t foa[2][3];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) foa[s][pc] = ABLK ? (uint32_t)(((2 * s + lhalf) * 3 + pc) * 512 + lrow * 16) : fo[s][pc];
    bf16x8 af[2][TM][3], bf[2][TN][3];
    constexpr int NR = 3 * (TM + TN);
    auto read_one = [&](int buf, int s, int set, int r) {
        if (r < 3 * TM) {
            const int mi = r / 3, pc = r % 3;
            af[set][mi][pc] = *reinterpret_cast<const bf16x8*>(Afr + buf * A_STAGE + mi * 32 * ROWB + foa[s][pc]);
        } else {
            const int q = r - 3 * TM, ni = q / 3, pc = q % 3;
            bf[set][ni][pc] = *reinterpret_cast<const bf16x8*>(Bfr + buf * B_STAGE + ni * 32 * ROWB + fo[s][pc]);
        }
    };
    f32x16 acc[TM][TN];
    constexpr int G = NPROD * TM * TN;
    static_assert(NR + NP <= G, "tile too small for the staging interleave");

    // one K tile out of buffer `buf` (gemm_split3_kernel's schedule): step 0's MFMAs over fragment set 0 with the reads of step 1's
    // fragments in their shadow; barrier; step 1's MFMAs with the reads of the next K tile's first fragments (other buffer) and the copies of
    // the K tile after next (into this buffer) in their shadow
    auto ktile = [&](auto bufc) {
        constexpr int buf = decltype(bufc){};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (s == 1) {
                __builtin_amdgcn_sched_barrier(0);
                dma_wait_barrier();
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int p = 0; p < NPROD; ++p)
#pragma unroll
                for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                    for (int ni = 0; ni < TN; ++ni) {
                        const int idx = (p * TM + mi) * TN + ni;
                        if constexpr (SWAP)
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bf[s][ni][piece_w(p)], af[s][mi][piece_a(p)], acc[mi][ni], 0, 0, 0);
                        else
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s][mi][piece_a(p)], bf[s][ni][piece_w(p)], acc[mi][ni], 0, 0, 0);
                        bool any = false;
                        if (s == 0) {
                            if (idx < NR) { read_one(buf, 1, 1, idx); any = true; }
                        } else {
                            if (idx < NR) { read_one(buf ^ 1, 0, 0, idx); any = true; }
                            else if (idx - NR < NP) { dma_piece(buf, idx - NR); any = true; }
                        }
                        if (any) __builtin_amdgcn_sched_barrier(0);
                    }
        }
        fetch_advance();
    };

    // fill: the first two K tiles of segment n into buffers 0 / 1, tile 0's first fragments into set 0
    auto fill = [&](int n) {
        fetch_seg(n);
        fn = n;
#pragma unroll
        for (int p = 0; p < NP; ++p) dma_piece(0, p);
        fetch_advance();
#pragma unroll
        for (int p = 0; p < NP; ++p) dma_piece(1, p);
        fetch_advance();
        dma_wait_barrier();
#pragma unroll
        for (int r = 0; r < NR; ++r) read_one(0, 0, 0, r);
    };

    static_assert((int64_t)P_NWG * P_SLAB * 4 < (int64_t(1) << 31), "slab offsets are 32-bit");
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(ws.part, 0, P_NWG * P_SLAB * 4, 0x00020000);
    const uint32_t slab_lane = (uint32_t)(wave * (TM * TN * 4) * 1024 + lane * 16);     // a wave's 16 chunk rows of 1 KiB each
    int pub_pending = 0;         // the slab's stores are issued; the flag goes out after the next K tile's barrier (every wave drained)
    int par = 0;                 // buffer of the next K tile
    auto after_tile = [&]() {
        if (pub_pending) {
            if (tid == 0) __hip_atomic_store(ws.flag + xcd * PG + ln, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            pub_pending = 0;
        }
    };

    if constexpr (CONT) fill(0);
    for (int n = 0; n < nseg; ++n) {
        int j, kb, ke, kind, bm0, bn0;
        seg_of(n, j, kb, ke, kind);
        tile_of(j, bm0, bn0);
        if constexpr (!CONT) {
            fill(n);
            par = 0;
        }
        if (kind == 2) {
            // the accumulators of k tiles [0, kb) from lane ln of the previous XCD: one thread polls one word, then sc1 loads
            if (tid == 0) {
                unsigned spins = 0;
                unsigned* f = ws.flag + (xcd - 1) * PG + ln;
                while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
                    __builtin_amdgcn_s_sleep(2);
                    if (++spins > (1u << 22)) {                        // ~0.5 s: report, never hang
                        __hip_atomic_store(ws.flag + P_NWG, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        break;
                    }
                }
                __hip_atomic_store(f, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // re-armed for the next launch (stream order)
            }
            asm volatile("s_barrier" ::: "memory");
            const uint32_t base = (uint32_t)((xcd - 1) * PG + ln) * (uint32_t)(P_SLAB * 4) + slab_lane;
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(rsrc, base + (uint32_t)(((mi * TN + ni) * 4 + q) * 1024), 0, 16);
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[mi][ni][q * 4 + c] = __uint_as_float(r[c]);
                    }
        } else {
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;
        }

        int cnt = ke - kb;
        if (cnt > 0 && par) { ktile(IntC<1>{}); after_tile(); --cnt; par = 0; }
        for (; cnt >= 2; cnt -= 2) {
            ktile(IntC<0>{});
            after_tile();
            ktile(IntC<1>{});
            after_tile();
        }
        if (cnt) { ktile(IntC<0>{}); after_tile(); par = 1; }

        if (kind == 1) {
            // raw accumulators -> slab (xcd, ln), write-through; published after the next K tile's barrier
            const uint32_t base = (uint32_t)(xcd * PG + ln) * (uint32_t)(P_SLAB * 4) + slab_lane;
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const u32x4 v = {__float_as_uint(acc[mi][ni][q * 4]), __float_as_uint(acc[mi][ni][q * 4 + 1]),
                                         __float_as_uint(acc[mi][ni][q * 4 + 2]), __float_as_uint(acc[mi][ni][q * 4 + 3])};
                        __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, base + (uint32_t)(((mi * TN + ni) * 4 + q) * 1024), 0, 16);
                    }
            pub_pending = 1;
        } else if constexpr (MODE == 0) {
            store_tile<TM, TN, EPI>(a, acc, bm0 + wm0, bn0 + wn0, lrow, lhalf);
        } else if constexpr (MODE == 2) {
            store_tile_split3_swapped<TM, TN, EPI>(a, acc, bm0 + wm0, bn0 + wn0, lane);
        } else {
            constexpr int WT = TN * 32 + 4;
            static_assert(NW * TM * 32 * WT * 4 <= 2 * (A_STAGE + B_STAGE), "transpose tile does not fit the stage buffers");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // the copies past the segment's end have landed
            __syncthreads();                                           // every wave is done with the stage buffers
            store_tile_split3<TM, TN, EPI>(a, acc, reinterpret_cast<float*>(smem) + wave * (TM * 32 * WT), bm0 + wm0, bn0 + wn0, lane);
            __syncthreads();                                           // ... and with the transpose tiles, before the next fill
        }
        if constexpr (!CONT) {
            if (pub_pending) {                                         // MODE 1 has no next K tile to hide behind: drain and publish now
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                after_tile();
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                   // no LDS-DMA write may outlive the workgroup's LDS allocation
    if (pub_pending) {                                                 // (a first part is never a range's last segment; kept for safety)
        __syncthreads();
        after_tile();
    }
}

template <int EPI, int MODE, bool ABLK = false>
int launch_persist_cfg(const GemmArgs& a, const PersistWs& ws, hipStream_t s) {
    const int tiles_m = a.M / PBM, tiles_n = a.N / PBN;
    hipLaunchKernelGGL((gemm_split3_persist_kernel<EPI, MODE, ABLK>), dim3(P_NWG), dim3(512), 0, s, a, tiles_m, tiles_n, ws);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

// the one-workgroup-per-tile variants of launch_gemm_split3 that run a kernel of this file; -1 for any other id
int launch_split3_exp_tiles(const GemmArgs& a, int epi, int variant, hipStream_t s) {
    switch (variant) {
        case 20: return launch_split3_cfg<2, 4, 2, 2>(a, epi, s);      // the product tiles until round 4: 128 x 256 on 8 waves, 128 x 128 on 4
        case 22: return launch_split3_cfg<2, 2, 2, 2>(a, epi, s);
        case 1: return launch_split3_cfg<2, 2, 2, 4>(a, epi, s);    // 4 waves of 64 x 128: 3 % slower (r3v)
        case 4: return launch_split3_wide(a, epi, s);               // 256 x 256, 4 waves of 128 x 128, 16-deep stages: the same rate (r3ak)
        // experiments on the default tile, EPI_NONE only: 3 = step-0 fragment reads every 2nd MFMA (the first version's schedule);
        // 31 / 32 / 34 / 37 = timing-only ablations (no copies / no barrier / no fragment reads / none of the three): garbage results
        case 3: return epi == EPI_NONE ? launch_split3_abl<2, 4, 2, 2, 0, 2>(a, s) : -1;
        case 31: return epi == EPI_NONE ? launch_split3_abl<2, 4, 2, 2, 1, 0>(a, s) : -1;
        case 32: return epi == EPI_NONE ? launch_split3_abl<2, 4, 2, 2, 2, 0>(a, s) : -1;
        case 34: return epi == EPI_NONE ? launch_split3_abl<2, 4, 2, 2, 4, 0>(a, s) : -1;
        case 37: return epi == EPI_NONE ? launch_split3_abl<2, 4, 2, 2, 7, 0>(a, s) : -1;
        default: return -1;
    }
}

// modes 10 (fp32 output) / 11 (split3 output through LDS) / 12 (split3 output, swapped roles) of launch_gemm_split3_persist, which has
// checked gemm_split3_persist_ok(a) and the workspace
int launch_split3_exp_persist(const GemmArgs& a, int epi, int mode, void* ws_mem, hipStream_t s) {
    mode -= 10;
    if ((mode == 0) != (a.c_split == nullptr) || mode < 0 || mode > 2 || (a.M % PBM) != 0) return -1;      // (the 32x32x16 kernels: whole row tiles only)
    // the 32x32x16 kernels of this file keep round 4's 0 / 1 flags (set by the producer, cleared by the consumer); the product kernel leaves
    // epochs in them: zero the flag words (not the control words) first
    if (hipMemsetAsync(reinterpret_cast<char*>(ws_mem) + (size_t)P_NWG * P_SLAB * 4, 0, P_NWG * sizeof(unsigned), s) != hipSuccess) return -2;
    if (a.c_split != nullptr && epi == EPI_BIAS_RESID) return -1;
    PersistWs ws;
    ws.part = reinterpret_cast<float*>(ws_mem);
    ws.flag = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(ws_mem) + (size_t)P_NWG * P_SLAB * 4);
    if (a.a_blk) {      // row-blocked A (fc2's operand): bias + residual, or no epilogue
        if (mode != 0) return -1;
        if (epi == EPI_BIAS_RESID) return launch_persist_cfg<EPI_BIAS_RESID, 0, true>(a, ws, s);
        if (epi == EPI_NONE) return launch_persist_cfg<EPI_NONE, 0, true>(a, ws, s);
        return -1;
    }
#define THMR_PERSIST_CASE(E, MD) \
    if (epi == E && mode == MD) return launch_persist_cfg<E, MD>(a, ws, s);
    THMR_PERSIST_CASE(EPI_NONE, 0)
    THMR_PERSIST_CASE(EPI_BIAS, 0)
    THMR_PERSIST_CASE(EPI_BIAS_RESID, 0)
    THMR_PERSIST_CASE(EPI_BIAS_QSCALE, 0)
    THMR_PERSIST_CASE(EPI_BIAS_GELU, 0)
    THMR_PERSIST_CASE(EPI_BIAS_GELU, 2)
    THMR_PERSIST_CASE(EPI_NONE, 2)
    THMR_PERSIST_CASE(EPI_BIAS_GELU, 1)      // split3 output through the LDS transposition: 796 vs 784 us on the fc1 shape (profiles/r4a_split3_gemm_persistent_b64.jsonl)
    THMR_PERSIST_CASE(EPI_NONE, 1)
#undef THMR_PERSIST_CASE
    return -1;
}

// small-M split3 GEMM: 64x64 tiles on a 4-deep LDS-DMA ring; ksplit > 1 writes raw partial sums to part[ksplit][M][N] and applies NO
// epilogue (launch_splitk_resid_ln / launch_splitk_epilogue then do)
int launch_gemm_split3_ring(const GemmArgs& a, int epi, int ksplit, float* part, hipStream_t s) {
    if (a.M <= 0 || a.N <= 0 || a.K <= 0 || ksplit < 1 || (a.K % (SBK * ksplit)) != 0 || (a.lda % 8) != 0 || (a.ldw % 8) != 0) return -1;
    if (a.lda * 6 * 64 >= (int64_t(1) << 32) || a.ldw * 6 * 64 >= (int64_t(1) << 32) || (ksplit > 1 && part == nullptr)) return -1;
    if (a.cs_out != nullptr || a.ksplit > 1 || a.a_blk) return -1;
    if (a.c_split != nullptr && ((a.N % 8) != 0 || (a.ldcs % 8) != 0 || a.ldcs < a.N || epi == EPI_BIAS_RESID || ksplit > 1)) return -1;
    const int tiles_m = (a.M + 63) / 64, tiles_n = (a.N + 63) / 64;
    const int groups = tiles_n * ksplit;
    dim3 grid(8 * tiles_m * ((groups + 7) / 8)), block(256);
    if (ksplit > 1) {
        hipLaunchKernelGGL((gemm_split3_ring_kernel<4, EPI_NONE, true>), grid, block, 0, s, a, tiles_m, groups, ksplit, part);
        return hipGetLastError() == hipSuccess ? 0 : -2;
    }
#define THMR_SRING_CASE(E)                                                                                              \
    case E:                                                                                                             \
        hipLaunchKernelGGL((gemm_split3_ring_kernel<4, E, false>), grid, block, 0, s, a, tiles_m, groups, 1, nullptr);   \
        break;
    switch (epi) {
        THMR_SRING_CASE(EPI_NONE)
        THMR_SRING_CASE(EPI_BIAS)
        THMR_SRING_CASE(EPI_BIAS_GELU)
        THMR_SRING_CASE(EPI_BIAS_RESID)
        THMR_SRING_CASE(EPI_BIAS_QSCALE)
        default: return -1;
    }
#undef THMR_SRING_CASE
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

#endif  // THMR_EXPERIMENTS
