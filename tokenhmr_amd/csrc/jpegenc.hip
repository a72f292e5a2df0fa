// Baseline JPEG encoding of device images (include/tokenhmr_hip.h).  A fixed number of launches over a whole batch:
//   transform   one 8x8 block per 8 lanes: strided load + conversion + colour + downsample, the row pass, a transpose through LDS (rows
//               padded to 9 words), the column pass, quantisation; int16 coefficients in zigzag order, blocks in scan order
//   count       one block per lane: its code length in bits (the DC predictor is the nearest real block of its component before it),
//               prefix-summed over the segment of SEG_BLOCKS blocks a workgroup holds
//   bit scan    one workgroup per image: the exclusive scan of its segments' sums
//   pack        one block per lane again: the codes go, MSB first, to the block's bit offset in the UNSTUFFED scan; a lane assembles
//               32-bit words in registers and ORs each into a zeroed buffer (the two boundary words are shared with its neighbours)
//   stuff       the 0xFF bytes of every CHUNK of the unstuffed scans are counted, scanned (one workgroup walks the images in order, which
//               also packs the files' scans densely), and the bytes scattered with the 0x00 inserted — into the pinned staging, so the
//               host needs one synchronisation and no second copy.  It comes after packing: stuffing depends on byte alignment.
// Images flagged THMR_JPEG_OPTIMIZE are coded with their own tables, in the same call; they add two launches between transform and count:
//   histogram   one block per lane, like count: its symbols go into an LDS histogram of the workgroup (a segment never spans two
//               images), which is added to the image's global histogram with integer atomics — order-independent, so the files stay
//               deterministic.  The global histograms are zeroed on the stream by every call.
//   tables      one wave per (image, table): jpegem::optimal_table, the routine of thmr_jpeg_optimal_table, with its searches and its
//               per-symbol steps spread over the wave; lane 0 writes bits / huffval (copied to the pinned staging with the scans'
//               places, for the DHT segments the host writes) and the code words in the TABLE_WORDS layout
// count and pack then read the image's own code words: the table is chosen per workgroup.  Unflagged images take the Annex K tables.
// The arithmetic and the coding rules live in jpegenc_math.h, which the CPU encode (jpegenc_host.h) shares: both write the same bytes.
// Headers, DQT / DHT and EOI are written on the host.  The source image and its pixel conversion (image_source.h) and the item checks
// (image_item_host.h) are the PNG encoder's too; item_of and block_scan are batch_device.h's.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "batch_device.h"
#include "handle_util.h"
#include "jpegenc_host.h"

namespace {

thread_local ErrorSink<thmr_jpeg_encoder> g_jenc_err{true};        // also behind thmr_last_error(NULL)

constexpr int TRANSFORM_BLOCKS = 32;        // blocks per workgroup of the transform: 8 lanes each
constexpr int SEG_BLOCKS = 256;             // blocks per segment: one workgroup of count / pack, one lane each
constexpr int CHUNK = 1024;                 // bytes of an unstuffed scan per workgroup of the stuffing kernels: one word per lane
constexpr int64_t MAX_BATCH_BLOCKS = (int64_t)1 << 28;
static_assert(SEG_BLOCKS % TRANSFORM_BLOCKS == 0 && SEG_BLOCKS == 256 && CHUNK == 4 * 256, "a workgroup has 256 lanes and never spans two images");

// One image as the kernels see it.
struct JpegItemDev {
    const void* pixels;
    jpegem::Frame f;
    int64_t blk0, nblk;         // its blocks are [blk0, blk0 + nblk) of the batch; blk0 is a multiple of SEG_BLOCKS
    int64_t seg0, nseg;         // its segments
    int64_t chunk0;             // the first chunk of its unstuffed scan, which has room for the worst case
    int32_t opt, reserved;      // opt: -1, or its index among the images coded with their own tables
    uint16_t q[128];            // [class * 64 + zigzag position]
};
static_assert(sizeof(JpegItemDev) % 8 == 0, "descriptors are read as an array");
constexpr size_t TABLE_BYTES = sizeof(uint32_t) * 2 * jpegem::TABLE_WORDS;
static_assert(TABLE_BYTES % 16 == 0, "the descriptors follow the code tables");

__global__ __launch_bounds__(256) void jpegenc_transform_kernel(const JpegItemDev* __restrict__ items, int n, int16_t* __restrict__ coef) {
    __shared__ int ws[TRANSFORM_BLOCKS][72];
    const int lb = threadIdx.x >> 3, lane = threadIdx.x & 7;
    const int64_t g = (int64_t)blockIdx.x * TRANSFORM_BLOCKS + lb;
    const JpegItemDev& it = items[item_of<&JpegItemDev::blk0>(items, n, g)];
    const int64_t b = g - it.blk0;
    bool live = b < it.nblk;
    int comp = 0, bx = 0, by = 0;
    if (live) {
        const int64_t m = b / it.f.bpm;
        const int my = (int)(m / it.f.mcux);
        bool dummy;
        jpegem::block_place(it.f, (int)(m - (int64_t)my * it.f.mcux), my, (int)(b - m * it.f.bpm), comp, bx, by, dummy);
        live = !dummy;
    }
    int v[8];
    if (live) {
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = jpegem::component_sample(it.f, it.pixels, comp, by * 8 + lane, bx * 8 + c) - 128;
        jpegem::fdct8(v, true);
#pragma unroll
        for (int c = 0; c < 8; ++c) ws[lb][lane * 9 + c] = v[c];
    }
    __syncthreads();
    if (live) {
        const uint16_t* q = it.q + (comp ? 64 : 0);
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = ws[lb][r * 9 + lane];
        jpegem::fdct8(v, false);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int z = jpegem::zigzag_of_natural(r * 8 + lane);
            coef[g * 64 + z] = (int16_t)jpegem::quantise(v[r], q[z]);
        }
    }
}

// What histogram, count and pack share: the block of lane `threadIdx.x` of segment `blockIdx.x`, loaded and walked symbol by symbol
// through visit(cls, slot, value bits, count of value bits).  Returns whether the lane has a block.
template <typename Visit>
__device__ bool walk_lane_block(const JpegItemDev& it, int64_t g, const int16_t* __restrict__ coef, Visit&& visit) {
    const int64_t b = g - it.blk0;
    if (b >= it.nblk) return false;
    const int64_t m = b / it.f.bpm;
    const int my = (int)(m / it.f.mcux);
    int comp, bx, by;
    bool dummy;
    jpegem::block_place(it.f, (int)(m - (int64_t)my * it.f.mcux), my, (int)(b - m * it.f.bpm), comp, bx, by, dummy);
    const int cls = comp ? 1 : 0;
    if (dummy) {
        jpegem::walk_dummy([&](int slot, uint32_t value, int s) { visit(cls, slot, value, s); });
        return true;
    }
    __align__(16) int16_t zz[64];
#pragma unroll
    for (int i = 0; i < 8; ++i) reinterpret_cast<uint4*>(zz)[i] = reinterpret_cast<const uint4*>(coef + g * 64)[i];
    const int64_t pred = jpegem::dc_predecessor(it.f, b);
    const int diff = zz[0] - (pred < 0 ? 0 : coef[(it.blk0 + pred) * 64]);
    jpegem::walk_block(zz, diff, [&](int slot, uint32_t value, int s) { visit(cls, slot, value, s); });
    return true;
}

// The same block coded through emit(bits, count) with the code words of both classes at `tables`.
template <typename Emit>
__device__ bool code_lane_block(const JpegItemDev& it, int64_t g, const int16_t* __restrict__ coef, const uint32_t* tables, Emit&& emit) {
    return walk_lane_block(it, g, coef, [&](int cls, int slot, uint32_t value, int s) {
        const uint32_t e = tables[cls * jpegem::TABLE_WORDS + slot];
        emit(((e & 0xFFFFu) << s) | value, (int)(e >> 16) + s);
    });
}

// The code words of the workgroup's image into LDS: its own (opt_tables) where it is flagged, else the Annex K ones.
__device__ void load_tables(const JpegItemDev& it, const uint32_t* __restrict__ tables, const uint32_t* __restrict__ opt_tables, uint32_t* lds) {
    const uint32_t* src = it.opt >= 0 ? opt_tables + (size_t)it.opt * 2 * jpegem::TABLE_WORDS : tables;
    for (int i = threadIdx.x; i < 2 * jpegem::TABLE_WORDS; i += 256) lds[i] = src[i];
    __syncthreads();
}

// Flagged images only: hist[opt][cls * TABLE_WORDS + slot] += the symbols of this segment.
__global__ __launch_bounds__(256) void jpegenc_histogram_kernel(const JpegItemDev* __restrict__ items, int n, const int16_t* __restrict__ coef,
                                                                uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[2 * jpegem::TABLE_WORDS];
    const int64_t g = (int64_t)blockIdx.x * SEG_BLOCKS + threadIdx.x;
    const JpegItemDev& it = items[item_of<&JpegItemDev::blk0>(items, n, (int64_t)blockIdx.x * SEG_BLOCKS)];
    if (it.opt < 0) return;             // the whole workgroup
    for (int i = threadIdx.x; i < 2 * jpegem::TABLE_WORDS; i += 256) h[i] = 0;
    __syncthreads();
    walk_lane_block(it, g, coef, [&](int cls, int slot, uint32_t, int) { atomicAdd(&h[cls * jpegem::TABLE_WORDS + slot], 1u); });
    __syncthreads();
    uint32_t* mine = hist + (size_t)it.opt * 2 * jpegem::TABLE_WORDS;
    for (int i = threadIdx.x; i < 2 * jpegem::TABLE_WORDS; i += 256)
        if (h[i]) atomicAdd(&mine[i], h[i]);
}

// jpegem::optimal_table's steps on one wave of 64 lanes (the whole workgroup): one() on lane 0, each() strided over the lanes, compact()
// by ballot and a count of the lanes below, 64 entries a round, min2() a local pass and six exchanges over the wave.  The barriers order the LDS traffic between the steps.
struct WavePar {
    template <typename F> __device__ void one(F&& f) {
        if (threadIdx.x == 0) f();
        __syncthreads();
    }
    template <typename F> __device__ void each(int n, F&& f) {
        for (int i = threadIdx.x; i < n; i += 64) f(i);
        __syncthreads();
    }
    template <typename Pred, typename Put> __device__ int compact(int n, Pred&& pred, Put&& put) {
        int base = 0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + (int)threadIdx.x;
            const bool used = i < n && pred(i);
            const unsigned long long mask = __ballot(used);
            if (used) put(i, base + __popcll(mask & (((unsigned long long)1 << threadIdx.x) - 1)));
            base += __popcll(mask);
        }
        __syncthreads();
        return base;
    }
    template <typename Key> __device__ void min2(int n, Key&& key, uint64_t& k1, uint64_t& k2) {
        k1 = k2 = jpegem::OPT_NO_KEY;
        for (int i = threadIdx.x; i < n; i += 64) {
            const uint64_t k = key(i);
            if (k < k1) { k2 = k1; k1 = k; } else if (k < k2) k2 = k;
        }
        // six exchanges, each between lanes whose keys so far come from disjoint sets of lanes: inside a row of 16 lanes by DPP (the
        // neighbour, the other pair of the quad, the mirror image in the half row, in the row), then across the rows
        join(k1, k2, dpp<0xB1>(k1), dpp<0xB1>(k2));             // quad_perm [1, 0, 3, 2]
        join(k1, k2, dpp<0x4E>(k1), dpp<0x4E>(k2));             // quad_perm [2, 3, 0, 1]
        join(k1, k2, dpp<0x141>(k1), dpp<0x141>(k2));           // row_half_mirror
        join(k1, k2, dpp<0x140>(k1), dpp<0x140>(k2));           // row_mirror
        join(k1, k2, __shfl_xor((unsigned long long)k1, 16, 64), __shfl_xor((unsigned long long)k2, 16, 64));
        join(k1, k2, __shfl_xor((unsigned long long)k1, 32, 64), __shfl_xor((unsigned long long)k2, 32, 64));
        __syncthreads();
    }
    // The two smallest of (k1, k2) and (o1, o2), which share no key but OPT_NO_KEY.
    static __device__ void join(uint64_t& k1, uint64_t& k2, uint64_t o1, uint64_t o2) {
        const uint64_t lo = k1 < o1 ? k1 : o1, hi = k1 < o1 ? o1 : k1, second = k2 < o2 ? k2 : o2;
        k1 = lo; k2 = hi < second ? hi : second;
    }
    template <int CTRL> static __device__ uint64_t dpp(uint64_t v) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, false);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, false);
        return (uint64_t)hi << 32 | lo;
    }
};

// Workgroup (image, table) = (blockIdx.x / 4, blockIdx.x % 4), tables in the order DC0, AC0, DC1, AC1: out[blockIdx.x], and its code
// words into the image's TABLE_WORDS layout.  A grey image has no DC1 / AC1.
__global__ __launch_bounds__(64) void jpegenc_tables_kernel(const JpegItemDev* __restrict__ items, int n, const int32_t* __restrict__ opt_item,
                                                            const uint32_t* __restrict__ hist, uint32_t* __restrict__ opt_tables,
                                                            jpegem::OptimalTable* __restrict__ out) {
    __shared__ jpegem::OptimalWork w;
    __shared__ jpegem::OptimalTable t;              // built in LDS: lane 0 reads it back for the code words
    const int o = blockIdx.x >> 2, cls = (blockIdx.x >> 1) & 1, ac = blockIdx.x & 1;
    if (cls && items[opt_item[o]].f.ncomp == 1) return;
    const size_t at = ((size_t)o * 2 + cls) * jpegem::TABLE_WORDS + (ac ? 16 : 0);
    const int nhist = ac ? 256 : 16;
    for (int i = threadIdx.x; i < nhist; i += 64) opt_tables[at + i] = 0;
    WavePar par;
    jpegem::optimal_table(reinterpret_cast<const int32_t*>(hist + at), nhist, w, par, &t);
    jpegem::code_words(t, w, par, opt_tables + at);
    static_assert(sizeof(jpegem::OptimalTable) % 4 == 0, "copied by words");
    for (int i = threadIdx.x; i < (int)(sizeof(t) / 4); i += 64) reinterpret_cast<uint32_t*>(&out[blockIdx.x])[i] = reinterpret_cast<const uint32_t*>(&t)[i];
}

__global__ __launch_bounds__(256) void jpegenc_count_kernel(const JpegItemDev* __restrict__ items, int n, const uint32_t* __restrict__ tables,
                                                            const uint32_t* __restrict__ opt_tables, const int16_t* __restrict__ coef,
                                                            uint32_t* __restrict__ blkoff, uint32_t* __restrict__ segsum) {
    __shared__ uint32_t codes[2 * jpegem::TABLE_WORDS];
    __shared__ uint32_t part[4];
    const int64_t g = (int64_t)blockIdx.x * SEG_BLOCKS + threadIdx.x;
    const JpegItemDev& it = items[item_of<&JpegItemDev::blk0>(items, n, g)];
    load_tables(it, tables, opt_tables, codes);
    uint32_t bits = 0;
    code_lane_block(it, g, coef, codes, [&](uint32_t, int k) { bits += (uint32_t)k; });
    uint32_t total;
    blkoff[g] = block_scan(bits, part, total);
    if (threadIdx.x == 0) segsum[blockIdx.x] = total;
}

// One workgroup per image: segoff = the exclusive scan of its segments' sums, ibits = its scan's bits before the padding.
__global__ __launch_bounds__(256) void jpegenc_bitscan_kernel(const JpegItemDev* __restrict__ items, const uint32_t* __restrict__ segsum,
                                                              unsigned long long* __restrict__ segoff, unsigned long long* __restrict__ ibits) {
    __shared__ unsigned long long part[4];
    const JpegItemDev& it = items[blockIdx.x];
    unsigned long long carry = 0;
    for (int64_t s0 = 0; s0 < it.nseg; s0 += 256) {
        const int64_t s = s0 + threadIdx.x;
        unsigned long long total;
        const unsigned long long before = block_scan<unsigned long long>(s < it.nseg ? segsum[it.seg0 + s] : 0, part, total);
        if (s < it.nseg) segoff[it.seg0 + s] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) ibits[blockIdx.x] = carry;
}

// MSB-first bits into 32-bit words of a zeroed buffer: word w holds stream bytes 4w ... 4w + 3, the first in its top byte.
struct WordPacker {
    uint32_t* words;
    int64_t w;
    uint64_t acc;
    int n;              // bits of acc in use, below 32 between calls; the first word's bits before the start stay zero
    __device__ WordPacker(uint32_t* words_, uint64_t at) : words(words_), w((int64_t)(at >> 5)), acc(0), n((int)(at & 31)) {}
    __device__ void operator()(uint32_t bits, int k) {          // k <= 26: 16 + 10 (AC), 11 + 11 (DC, Annex K) or 12 + 11 (DC, an image's own table)
        acc = (acc << k) | bits;
        n += k;
        if (n >= 32) {
            atomicOr(&words[w++], (uint32_t)(acc >> (n - 32)));
            n -= 32;
            acc &= ((uint64_t)1 << n) - 1;
        }
    }
    __device__ void flush() { if (n) atomicOr(&words[w], (uint32_t)(acc << (32 - n))); }
};

__global__ __launch_bounds__(256) void jpegenc_pack_kernel(const JpegItemDev* __restrict__ items, int n, const uint32_t* __restrict__ tables,
                                                           const uint32_t* __restrict__ opt_tables, const int16_t* __restrict__ coef,
                                                           const uint32_t* __restrict__ blkoff, const unsigned long long* __restrict__ segoff,
                                                           const unsigned long long* __restrict__ ibits, uint32_t* __restrict__ unstuffed) {
    __shared__ uint32_t codes[2 * jpegem::TABLE_WORDS];
    const int64_t g = (int64_t)blockIdx.x * SEG_BLOCKS + threadIdx.x;
    const int i = item_of<&JpegItemDev::blk0>(items, n, g);
    const JpegItemDev& it = items[i];
    load_tables(it, tables, opt_tables, codes);
    if (g - it.blk0 >= it.nblk) return;
    WordPacker pk(unstuffed + it.chunk0 * (CHUNK / 4), segoff[blockIdx.x] + blkoff[g]);
    code_lane_block(it, g, coef, codes, pk);
    if (g - it.blk0 == it.nblk - 1) {           // the last byte is padded with ones
        const int pad = (int)((8 - (ibits[i] & 7)) & 7);
        if (pad) pk((1u << pad) - 1, pad);
    }
    pk.flush();
}

// The 0xFF bytes among the (up to four) bytes of word `word` that lie below `left` bytes: a mask, bit k for byte k.
__device__ int ff_mask(uint32_t word, int64_t left) {
    int m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < left && ((word >> (24 - 8 * k)) & 0xFF) == 0xFF) m |= 1 << k;
    return m;
}

__global__ __launch_bounds__(256) void jpegenc_ffcount_kernel(const JpegItemDev* __restrict__ items, int n, const unsigned long long* __restrict__ ibits,
                                                              const uint32_t* __restrict__ unstuffed, uint32_t* __restrict__ ffcount) {
    __shared__ uint32_t part[4];
    const int64_t g = blockIdx.x;
    const int i = item_of<&JpegItemDev::chunk0>(items, n, g);
    const int64_t bytes = (int64_t)((ibits[i] + 7) >> 3), at = (g - items[i].chunk0) * CHUNK + threadIdx.x * 4;
    if ((g - items[i].chunk0) * CHUNK >= bytes) return;        // the whole workgroup: a chunk of the worst case the scan did not reach
    uint32_t total;
    block_scan<uint32_t>(at < bytes ? __popc(ff_mask(unstuffed[g * (CHUNK / 4) + threadIdx.x], bytes - at)) : 0, part, total);
    if (threadIdx.x == 0) ffcount[g] = total;
}

// One workgroup walks the images in order: where each chunk's bytes go in the staging, and each scan's place and stuffed length.
__global__ __launch_bounds__(256) void jpegenc_ffscan_kernel(const JpegItemDev* __restrict__ items, int n, const unsigned long long* __restrict__ ibits,
                                                             const uint32_t* __restrict__ ffcount, int64_t* __restrict__ chunkout, int64_t* __restrict__ meta) {
    __shared__ unsigned long long part[4];
    int64_t base = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t bytes = (int64_t)((ibits[i] + 7) >> 3), nchunk = (bytes + CHUNK - 1) / CHUNK;
        unsigned long long carry = 0;
        for (int64_t c0 = 0; c0 < nchunk; c0 += 256) {
            const int64_t c = c0 + threadIdx.x;
            unsigned long long total;
            const unsigned long long before = block_scan<unsigned long long>(c < nchunk ? ffcount[items[i].chunk0 + c] : 0, part, total);
            if (c < nchunk) chunkout[items[i].chunk0 + c] = base + c * CHUNK + (int64_t)(carry + before);
            carry += total;
        }
        if (threadIdx.x == 0) { meta[2 * i] = base; meta[2 * i + 1] = bytes + (int64_t)carry; }
        base += bytes + (int64_t)carry;
    }
}

__global__ __launch_bounds__(256) void jpegenc_scatter_kernel(const JpegItemDev* __restrict__ items, int n, const unsigned long long* __restrict__ ibits,
                                                              const uint32_t* __restrict__ unstuffed, const int64_t* __restrict__ chunkout,
                                                              uint8_t* __restrict__ packed, int64_t packed_bytes) {
    __shared__ uint32_t part[4];
    const int64_t g = blockIdx.x;
    const int i = item_of<&JpegItemDev::chunk0>(items, n, g);
    const int64_t bytes = (int64_t)((ibits[i] + 7) >> 3), at = (g - items[i].chunk0) * CHUNK + threadIdx.x * 4;
    if ((g - items[i].chunk0) * CHUNK >= bytes) return;
    const uint32_t word = at < bytes ? unstuffed[g * (CHUNK / 4) + threadIdx.x] : 0;
    const int mask = at < bytes ? ff_mask(word, bytes - at) : 0;
    uint32_t total;
    int64_t o = chunkout[g] + threadIdx.x * 4 + block_scan<uint32_t>(__popc(mask), part, total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (at + k >= bytes) break;
        if (o < packed_bytes) packed[o] = (uint8_t)(word >> (24 - 8 * k));
        ++o;
        if ((mask >> k) & 1) {
            if (o < packed_bytes) packed[o] = 0;
            ++o;
        }
    }
}

}  // namespace

struct thmr_jpeg_encoder {
    int device = 0;
    DevBuf<int16_t> coef;
    DevBuf<uint32_t> unstuffed;
    DevBuf<char> work;          // per block, per segment, per chunk and per image words
    DevBuf<char> desc;          // the code tables, then the descriptors
    PinnedBuf<char> host;       // the same, then each image's (place, length), then the stuffed scans, which the device writes
    std::string err;
};

extern "C" {

int64_t thmr_jpeg_encode_bound(int32_t width, int32_t height, int32_t channels, int32_t subsampling) {
    return jpegeh::bound(width, height, channels, subsampling);
}

int64_t thmr_jpeg_encode_bound_flags(int32_t width, int32_t height, int32_t channels, int32_t subsampling, int32_t flags) {
    return jpegeh::bound(width, height, channels, subsampling, flags);
}

int thmr_jpeg_encode_host_flags(thmr_png_item* item, int32_t quality, int32_t subsampling, int32_t flags) {
    if (!item) return g_jenc_err.invalid(nullptr, "null item");
    item->written = 0;
    std::string err;
    if (const int rc = jpegeh::check_item(*item, quality, subsampling, err, flags)) return g_jenc_err.fail(nullptr, rc, err);
    if (const int rc = jpegeh::encode(*item, quality, subsampling, flags, err)) return g_jenc_err.fail(nullptr, rc, err);
    return 0;
}

int thmr_jpeg_encode_host(thmr_png_item* item, int32_t quality, int32_t subsampling) { return thmr_jpeg_encode_host_flags(item, quality, subsampling, 0); }

int thmr_jpeg_optimal_table(const int32_t* freq, uint8_t* bits, uint8_t* huffval, int32_t* nsym) {
    if (!freq || !bits || !huffval || !nsym) return g_jenc_err.invalid(nullptr, "null freq, bits, huffval or nsym");
    int64_t sum = 0;
    for (int i = 0; i < 256; ++i) {
        if (freq[i] < 0) return g_jenc_err.invalid(nullptr, "frequency " + std::to_string(i) + " is negative");
        sum += freq[i];
    }
    if (sum == 0) return g_jenc_err.invalid(nullptr, "every frequency is zero");
    if (sum > 1000000000) return g_jenc_err.invalid(nullptr, "the frequencies sum to more than 10^9");
    jpegem::OptimalTable t;
    jpegeh::optimal_table(freq, 256, t);
    if (t.nsym < 0) return g_jenc_err.fail(nullptr, THMR_ERR_UNSUPPORTED, "unsupported: the frequencies give a Huffman code of more than 32 bits before the limit");
    memcpy(bits, t.bits, 17);
    memcpy(huffval, t.huffval, (size_t)t.nsym);
    *nsym = t.nsym;
    return 0;
}

int thmr_jpeg_histogram_host(const thmr_png_item* item, int32_t quality, int32_t subsampling, int32_t* freq) {
    if (!item || !freq) return g_jenc_err.invalid(nullptr, "null item or freq");
    thmr_png_item it = *item;
    uint8_t unused;
    it.out = &unused;           // not written: the check asks for one
    it.capacity = jpegeh::bound(it.width, it.height, it.channels, subsampling, THMR_JPEG_OPTIMIZE);
    std::string err;
    if (const int rc = jpegeh::check_item(it, quality, subsampling, err, THMR_JPEG_OPTIMIZE)) return g_jenc_err.fail(nullptr, rc, err);
    int32_t hist[2 * jpegem::TABLE_WORDS];
    jpegeh::histogram(it, quality, subsampling, hist);
    memset(freq, 0, sizeof(int32_t) * 1024);
    for (int cls = 0; cls < 2; ++cls) {
        memcpy(freq + cls * 512, hist + cls * jpegem::TABLE_WORDS, sizeof(int32_t) * 16);
        memcpy(freq + cls * 512 + 256, hist + cls * jpegem::TABLE_WORDS + 16, sizeof(int32_t) * 256);
    }
    return 0;
}

const char* thmr_jpeg_encoder_last_error(const thmr_jpeg_encoder* e) { return g_jenc_err.read(e); }

int thmr_jpeg_encoder_create(int32_t device, thmr_jpeg_encoder** out) {
    return handle_create(device, out, g_jenc_err, "no such HIP device (without one, thmr_jpeg_encode_host encodes on the CPU)");
}

void thmr_jpeg_encoder_destroy(thmr_jpeg_encoder* e) { handle_destroy(e); }

}  // extern "C"

namespace {

// Both batch entry points.  flags: null for none.
int encode_batch(thmr_jpeg_encoder* e, thmr_png_item* items, const int32_t* qualities, const int32_t* subsamplings, const int32_t* flags, int32_t n, void* stream,
                 const char* who) {
    // every argument is checked before the handle, and the handle before any HIP call: a refusal never touches the device
    if (n <= 0 || n > 65535) return g_jenc_err.invalid(e, "n must be 1 ... 65535");
    if (!items || !qualities || !subsamplings) return g_jenc_err.invalid(e, "null item, quality or subsampling table");
    std::vector<JpegItemDev> ids((size_t)n);
    std::vector<int32_t> opt_item;              // the flagged items, in order
    int64_t blks = 0, chunks = 0, packed_bytes = 0;
    for (int i = 0; i < n; ++i) {
        thmr_png_item& it = items[i];
        it.written = 0;
        std::string err;
        const int32_t fl = flags ? flags[i] : 0;
        if (const int rc = jpegeh::check_item(it, qualities[i], subsamplings[i], err, fl)) return g_jenc_err.fail(e, rc, "item " + std::to_string(i) + ": " + err);
        JpegItemDev& d = ids[(size_t)i];
        memset(&d, 0, sizeof(d));
        d.pixels = it.pixels;
        d.f = jpegem::frame_of(jpegeh::image_of(it), subsamplings[i] == THMR_JPEG_420);
        d.blk0 = blks; d.nblk = jpegeh::blocks(it.width, it.height, it.channels, subsamplings[i]);
        d.seg0 = blks / SEG_BLOCKS; d.nseg = (d.nblk + SEG_BLOCKS - 1) / SEG_BLOCKS;
        d.chunk0 = chunks;
        d.opt = -1;
        if (fl & THMR_JPEG_OPTIMIZE) { d.opt = (int32_t)opt_item.size(); opt_item.push_back(i); }
        jpegeh::quant_tables(qualities[i], d.q);
        const int64_t scan = jpegeh::scan_bytes_max(d.nblk, fl);
        blks += d.nseg * SEG_BLOCKS;
        chunks += (scan + CHUNK - 1) / CHUNK;
        packed_bytes += 2 * scan;
        if (blks > MAX_BATCH_BLOCKS) return g_jenc_err.invalid(e, "item " + std::to_string(i) + ": the batch has more than 2^28 blocks");
    }
    if (!e) return g_jenc_err.invalid(e, "null handle");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t err;
    bool capturing;
    if (const int rc = enter_stream(e, st, g_jenc_err, &capturing)) return rc;
    if (capturing)
        return g_jenc_err.fail(e, THMR_ERR_STATE, std::string(who) + " returns files in host memory and cannot run inside a stream capture");

    const int64_t segs = blks / SEG_BLOCKS;
    const size_t nopt = opt_item.size();
    // descriptors: the Annex K code words | the items | (4-byte aligned already) the flagged items' indices
    const size_t desc_bytes = (TABLE_BYTES + sizeof(JpegItemDev) * (size_t)n + 4 * nopt + 255) & ~size_t(255);
    // meta: each image's (place, length) | the flagged images' four tables each
    const size_t meta_used = (size_t)n * 16 + nopt * 4 * sizeof(jpegem::OptimalTable);
    const size_t meta_bytes = (meta_used + 255) & ~size_t(255);
    const size_t hbytes = desc_bytes + meta_bytes + (size_t)packed_bytes;
    // work: blkoff [blks] u32 | segsum [segs] u32 | ffcount [chunks] u32 | (8-byte aligned) segoff [segs] | ibits [n] | chunkout [chunks] | meta [2 n] |
    //       tables out [4 nopt] | hist [nopt][2 TABLE_WORDS] u32 | code words [nopt][2 TABLE_WORDS] u32
    const size_t w32 = (((size_t)blks + (size_t)segs + (size_t)chunks) * 4 + 7) & ~size_t(7);
    const size_t w64 = ((size_t)segs + (size_t)n + (size_t)chunks + 2 * (size_t)n) * 8;
    const size_t wbytes = w32 + w64 + nopt * (4 * sizeof(jpegem::OptimalTable) + 2 * TABLE_BYTES);
    const size_t cn = (size_t)blks * 64, un = (size_t)chunks * (CHUNK / 4);
    const auto grow = {e->coef.want(cn, cn + cn / 4, "hipMalloc(coefficients)"), e->unstuffed.want(un, un + un / 4, "hipMalloc(unstuffed scans)"),
                       e->work.want(wbytes, wbytes + wbytes / 4, "hipMalloc(work)"), e->desc.want(desc_bytes, desc_bytes + desc_bytes / 4, "hipMalloc(descriptors)"),
                       e->host.want(hbytes, hbytes + hbytes / 4, "hipHostMalloc(staging)")};
    const char* what;
    if ((err = grow_synced(st, grow, what)) != hipSuccess) return g_jenc_err.hip(e, what, err);
    void* packed_dev = nullptr;
    if ((err = hipHostGetDevicePointer(&packed_dev, e->host.ptr(), 0)) != hipSuccess) return g_jenc_err.hip(e, "hipHostGetDevicePointer", err);
    packed_dev = static_cast<char*>(packed_dev) + desc_bytes + meta_bytes;
    memcpy(e->host, jpegeh::code_tables().t, TABLE_BYTES);
    memcpy(e->host.ptr() + TABLE_BYTES, ids.data(), sizeof(JpegItemDev) * (size_t)n);
    if (nopt) memcpy(e->host.ptr() + TABLE_BYTES + sizeof(JpegItemDev) * (size_t)n, opt_item.data(), 4 * nopt);
    if ((err = hipMemcpyAsync(e->desc, e->host, desc_bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return g_jenc_err.hip(e, "hipMemcpyAsync", err);
    if ((err = hipMemsetAsync(e->unstuffed, 0, un * 4, st)) != hipSuccess) return g_jenc_err.hip(e, "hipMemsetAsync", err);
    const uint32_t* tables = reinterpret_cast<const uint32_t*>(e->desc.ptr());
    const JpegItemDev* idev = reinterpret_cast<const JpegItemDev*>(e->desc.ptr() + TABLE_BYTES);
    uint32_t* blkoff = reinterpret_cast<uint32_t*>(e->work.ptr());
    uint32_t* segsum = blkoff + blks;
    uint32_t* ffcount = segsum + segs;
    unsigned long long* segoff = reinterpret_cast<unsigned long long*>(e->work.ptr() + w32);
    unsigned long long* ibits = segoff + segs;
    int64_t* chunkout = reinterpret_cast<int64_t*>(ibits + n);
    int64_t* meta = chunkout + chunks;
    jpegem::OptimalTable* tabout = reinterpret_cast<jpegem::OptimalTable*>(meta + 2 * n);         // meta and the tables are copied back as one piece
    uint32_t* hist = reinterpret_cast<uint32_t*>(tabout + 4 * nopt);
    uint32_t* opt_tables = hist + nopt * 2 * jpegem::TABLE_WORDS;
    const int32_t* opt_dev = reinterpret_cast<const int32_t*>(idev + n);
    // the histograms are grow-only scratch: zeroed by every call; so are the tables a grey image leaves out
    if (nopt && (err = hipMemsetAsync(tabout, 0, nopt * (4 * sizeof(jpegem::OptimalTable) + TABLE_BYTES), st)) != hipSuccess) return g_jenc_err.hip(e, "hipMemsetAsync", err);
    hipLaunchKernelGGL(jpegenc_transform_kernel, dim3((unsigned)(blks / TRANSFORM_BLOCKS)), dim3(256), 0, st, idev, n, e->coef.ptr());
    if (nopt) {
        hipLaunchKernelGGL(jpegenc_histogram_kernel, dim3((unsigned)segs), dim3(256), 0, st, idev, n, e->coef.ptr(), hist);
        hipLaunchKernelGGL(jpegenc_tables_kernel, dim3((unsigned)(4 * nopt)), dim3(64), 0, st, idev, n, opt_dev, hist, opt_tables, tabout);
    }
    hipLaunchKernelGGL(jpegenc_count_kernel, dim3((unsigned)segs), dim3(256), 0, st, idev, n, tables, opt_tables, e->coef.ptr(), blkoff, segsum);
    hipLaunchKernelGGL(jpegenc_bitscan_kernel, dim3((unsigned)n), dim3(256), 0, st, idev, segsum, segoff, ibits);
    hipLaunchKernelGGL(jpegenc_pack_kernel, dim3((unsigned)segs), dim3(256), 0, st, idev, n, tables, opt_tables, e->coef.ptr(), blkoff, segoff, ibits,
                       e->unstuffed.ptr());
    hipLaunchKernelGGL(jpegenc_ffcount_kernel, dim3((unsigned)chunks), dim3(256), 0, st, idev, n, ibits, e->unstuffed.ptr(), ffcount);
    hipLaunchKernelGGL(jpegenc_ffscan_kernel, dim3(1), dim3(256), 0, st, idev, n, ibits, ffcount, chunkout, meta);
    hipLaunchKernelGGL(jpegenc_scatter_kernel, dim3((unsigned)chunks), dim3(256), 0, st, idev, n, ibits, e->unstuffed.ptr(), chunkout,
                       static_cast<uint8_t*>(packed_dev), packed_bytes);
    if ((err = hipGetLastError()) != hipSuccess) return g_jenc_err.hip(e, "jpeg encoder kernel launch", err);
    const int64_t* mh = reinterpret_cast<const int64_t*>(e->host.ptr() + desc_bytes);
    if ((err = hipMemcpyAsync(e->host.ptr() + desc_bytes, meta, meta_used, hipMemcpyDeviceToHost, st)) != hipSuccess) return g_jenc_err.hip(e, "hipMemcpyAsync", err);
    if ((err = hipStreamSynchronize(st)) != hipSuccess) return g_jenc_err.hip(e, "hipStreamSynchronize", err);
    const uint8_t* ph = reinterpret_cast<const uint8_t*>(e->host.ptr() + desc_bytes + meta_bytes);
    const jpegem::OptimalTable* th = reinterpret_cast<const jpegem::OptimalTable*>(mh + 2 * n);
    for (int i = 0; i < n; ++i) {
        const int64_t at = mh[2 * i], len = mh[2 * i + 1];
        const int32_t fl = flags ? flags[i] : 0;
        if (at < 0 || len < 0 || len > 2 * jpegeh::scan_bytes_max(ids[(size_t)i].nblk, fl) || at + len > packed_bytes)
            return g_jenc_err.fail(e, THMR_ERR_STATE, "item " + std::to_string(i) + ": the scan exceeds its bound");
        const jpegem::OptimalTable* own = ids[(size_t)i].opt >= 0 ? th + 4 * ids[(size_t)i].opt : nullptr;
        for (int t = 0; own && t < (ids[(size_t)i].f.ncomp == 1 ? 2 : 4); ++t) {
            if (own[t].nsym < 0)
                return g_jenc_err.fail(e, THMR_ERR_UNSUPPORTED, "item " + std::to_string(i) + ": unsupported: the image's statistics give a Huffman code of more than 32 bits before the limit");
            if (own[t].nsym < 1 || own[t].nsym > (t & 1 ? 162 : 12)) return g_jenc_err.fail(e, THMR_ERR_STATE, "item " + std::to_string(i) + ": a table the device built is malformed");
        }
        uint8_t* p = items[i].out + jpegeh::write_header(items[i].out, ids[(size_t)i].f, ids[(size_t)i].q, own);
        memcpy(p, ph + at, (size_t)len);
        p[len] = 0xFF; p[len + 1] = 0xD9;
        items[i].written = (p + len + 2) - items[i].out;
    }
    return 0;
}

}  // namespace

extern "C" {

int thmr_jpeg_encode_batch(thmr_jpeg_encoder* e, thmr_png_item* items, const int32_t* qualities, const int32_t* subsamplings, int32_t n, void* stream) {
    return encode_batch(e, items, qualities, subsamplings, nullptr, n, stream, "thmr_jpeg_encode_batch");
}

int thmr_jpeg_encode_batch_flags(thmr_jpeg_encoder* e, thmr_png_item* items, const int32_t* qualities, const int32_t* subsamplings, const int32_t* flags, int32_t n,
                                 void* stream) {
    if (n > 0 && items && qualities && subsamplings && !flags) return g_jenc_err.invalid(e, "null flags table");
    return encode_batch(e, items, qualities, subsamplings, flags, n, stream, "thmr_jpeg_encode_batch_flags");
}

}  // extern "C"
