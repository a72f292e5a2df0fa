// PNG encoding of device images (include/tokenhmr_hip.h).  Three launches over a whole batch: convert + filter of every row
// (one wave per row), deflate of every segment of the filtered streams (one wave per segment, the segment in LDS), and the gather of
// the segments into one packed stream that crosses to the host.  The arithmetic and every selection rule live in png_math.h, which the
// CPU encode (png_host.h) shares: both write the same bytes.  The source image and its pixel conversion (image_source.h) and the item
// checks (image_item_host.h) are the JPEG encoder's too; item_of and the wave scans are batch_device.h's.  A batch with a dynamic-Huffman item (compression THMR_PNG_DYNAMIC) runs
// the DYNAMIC instantiation of png_deflate_kernel; a batch without one runs the other, the code it always ran.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "batch_device.h"
#include "handle_util.h"
#include "png_host.h"

namespace {

thread_local ErrorSink<thmr_png> g_png_err{true};        // also behind thmr_last_error(NULL)

// One image as the kernels see it.
struct PngItemDev {
    const void* pixels;
    pngm::Image im;
    int64_t filt_off;           // byte offset of its filtered stream (a multiple of 16)
    int32_t total;              // bytes of the filtered stream
    int32_t row0, seg0, nseg;   // its rows / segments are [row0, row0 + h) / [seg0, seg0 + nseg) of the batch
    int32_t ncand, cand[pngm::MAX_CAND];
    int32_t dynamic;            // compression THMR_PNG_DYNAMIC
};
static_assert(sizeof(PngItemDev) % 8 == 0, "descriptors are read as an array");

constexpr int SLOT = pngm::SEGMENT + pngm::SEGMENT / 8 + 64;     // bytes a segment's coded form can take: 3 + 9 bits a byte + the trailer
constexpr int RING = 128;                                         // words of the LDS bit buffer: one step adds at most 64 * 31 bits (64 * 48 in a dynamic block)
constexpr int64_t FINISH_CHUNK = 256 << 10;                       // bytes of a stream copied out and CRC-summed as one piece of work
constexpr int FINISH_THREADS = 16;                                // at most: what one command gets of a GPU box
static_assert(SLOT % 4 == 0 && pngm::SEGMENT % 16 == 0, "slots are written in words, segments loaded in 16-byte pieces");

// Convert + filter: one wave per row.  The five costs are summed over the row and reduced across the wave; the winner is written.
__global__ __launch_bounds__(256) void png_filter_kernel(const PngItemDev* __restrict__ items, int n, uint8_t* __restrict__ filt, int total_rows) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= total_rows) return;
    const PngItemDev& it = items[item_of<&PngItemDev::row0>(items, n, g)];
    const pngm::Image im = it.im;
    const int y = g - it.row0, rb = pngm::row_bytes(im);
    uint64_t sum[5] = {0, 0, 0, 0, 0};
    for (int i = lane; i < rb; i += 64) {
        int x, a, b, c;
        pngm::neighbours(im, it.pixels, y, i, x, a, b, c);
#pragma unroll
        for (int f = 0; f < 5; ++f) sum[f] += pngm::cost(pngm::residual(f, x, a, b, c));
    }
#pragma unroll
    for (int f = 0; f < 5; ++f) sum[f] = wave_sum(sum[f]);
    const int f = pngm::best_filter(sum);
    uint8_t* row = filt + it.filt_off + (int64_t)y * (1 + rb);
    if (lane == 0) row[0] = (uint8_t)f;
    for (int i = lane; i < rb; i += 64) {
        int x, a, b, c;
        pngm::neighbours(im, it.pixels, y, i, x, a, b, c);
        row[1 + i] = pngm::residual(f, x, a, b, c);
    }
}

// ORs k bits into the ring at stream bit `at`.  Words are owned by bit position, so the order of the ORs does not matter.
__device__ void ring_put(uint32_t* ring, int64_t at, uint64_t bits, int k) {
    if (k == 0) return;
    const uint64_t v = bits << (at & 31);
    const int w = (int)(at >> 5);
    atomicOr(&ring[w & (RING - 1)], (uint32_t)v);
    if (v >> 32) atomicOr(&ring[(w + 1) & (RING - 1)], (uint32_t)(v >> 32));
}

// Words [from, to) of the stream leave the ring for the slot, and the ring's copies are cleared for their next use.
__device__ void ring_flush(uint32_t* ring, uint32_t* slot, int from, int to, int lane) {
    for (int w = from + lane; w < to; w += 64) {
        if (w < SLOT / 4) slot[w] = ring[w & (RING - 1)];
        ring[w & (RING - 1)] = 0;
    }
}

// The greedy chain through a window of cnt positions from its first one: the mask of the positions it visits, and in pos how far it
// gets (at or past cnt).  adv: each lane's step, its match length or 1; any_match: whether some lane has a match at all.
__device__ uint64_t chain_through(int adv, bool any_match, int cnt, int& pos) {
    if (!any_match) {
        pos = cnt;
        return cnt == 64 ? ~0ull : ((1ull << cnt) - 1);
    }
    uint64_t sel = 0;
    for (pos = 0; pos < cnt;) {
        sel |= 1ull << pos;
        pos += __builtin_amdgcn_readlane(adv, pos);
    }
    return sel;
}

// One step of the bit stream: lane l appends k bits of t (k = 0: nothing) behind those of the lanes before it; the ring's complete
// words then leave for the slot.  WIDE: k can exceed 32.
template <bool WIDE>
__device__ void ring_step(uint32_t* ring, uint32_t* slot, int64_t& bits, int& flushed, uint64_t t, int k, int lane) {
    const int incl = wave_scan_inclusive(k, lane);
    // ring_put shifts its bits by up to 31 inside 64: it takes at most 33 bits at a time (a fixed-code token has 31).  A token of a
    // dynamic block has up to 15 + 5 + 15 + 13 = 48, so it goes in as its low 32 bits and the rest.
    static_assert(2 * pngm::MAX_BITS + 5 + 13 <= 64, "a token fits the 64-bit token word, and two puts of at most 32 bits");
    const int64_t at = bits + incl - k;
    ring_put(ring, at, t & 0xFFFFFFFFull, k < 32 ? k : 32);
    if (WIDE && k > 32) ring_put(ring, at + 32, t >> 32, k - 32);
    bits += __builtin_amdgcn_readlane(incl, 63);
    __syncthreads();
    const int complete = (int)(bits >> 5);
    ring_flush(ring, slot, flushed, complete, lane);
    flushed = complete;
    __syncthreads();
}

// Deflate: one wave per segment.  Per step the 64 lanes find the match at 64 consecutive positions (a function of the bytes alone), the
// greedy chain through them is walked from the step's first position, the chosen tokens' bit lengths are prefix-summed and the tokens
// ORed into an LDS ring, whose complete words go to the segment's slot.  The next step starts where the chain left the window.
// DYNAMIC is the instantiation for a batch with a dynamic item (compression THMR_PNG_DYNAMIC); a fixed item's segment comes out of it
// as out of the other.  A dynamic item's segment walks its chain twice.  The first walk counts the tokens' symbols into an LDS
// histogram and sums their fixed-code bits; lane 0 then builds the block's codes and header (pngm::dynamic_block, a few thousand serial
// steps while the other segments' waves run), and the block rule picks dynamic, fixed or stored before a bit is written.  The second
// walk emits with the codes looked up in LDS; the header goes first, 64 pieces a step through the same ring (a step adds at most
// 64 * 48 bits, the ring holds 4096 and never more than one word is left unflushed).
template <bool DYNAMIC>
__global__ __launch_bounds__(64) void png_deflate_kernel(const PngItemDev* __restrict__ items, int n_items, const uint8_t* __restrict__ filt,
                                                         uint8_t* __restrict__ slots, uint32_t* __restrict__ meta) {
    __shared__ __align__(16) uint8_t seg[pngm::SEGMENT + 16];
    __shared__ uint32_t ring[RING];
    __shared__ pngm::DynBlock code;
    __shared__ int64_t dynamic_bits;
    static_assert(sizeof(pngm::DynBlock) % 4 == 0, "cleared in words");
    const int lane = threadIdx.x, g = blockIdx.x;
    const PngItemDev& it = items[item_of<&PngItemDev::seg0>(items, n_items, g)];
    const int s = g - it.seg0;
    const int64_t off = (int64_t)s * pngm::SEGMENT;
    const int n = (int64_t)it.total - off < pngm::SEGMENT ? (int)(it.total - off) : pngm::SEGMENT;
    const bool last = s == it.nseg - 1;
    const bool want = DYNAMIC && it.dynamic != 0;
    const uint8_t* src = filt + it.filt_off + off;
    for (int i = lane * 16; i < n; i += 64 * 16) *reinterpret_cast<uint4*>(seg + i) = *reinterpret_cast<const uint4*>(src + i);
    for (int i = lane; i < RING; i += 64) ring[i] = 0;
    if constexpr (DYNAMIC)
        for (int i = lane; i < (int)(sizeof(pngm::DynBlock) / 4); i += 64) reinterpret_cast<int32_t*>(&code)[i] = 0;
    __syncthreads();
    if (lane < pngm::PAD) seg[n + lane] = 0;
    __syncthreads();

    uint64_t a = 0, b = 0;
    for (int i = lane; i < n; i += 64) { a += seg[i]; b += (uint64_t)(n - i) * seg[i]; }
    a = wave_sum(a); b = wave_sum(b);

    int ncand = it.ncand;
    int cand[pngm::MAX_CAND];
#pragma unroll
    for (int k = 0; k < pngm::MAX_CAND; ++k) cand[k] = it.cand[k];

    bool dyn = false, stored = false;
    int eob_bits = 7;
    uint32_t eob_code = 0;
    if (want) {                                          // (never in the fixed instantiation)
        uint64_t fixed = 0;
        for (int cur = 0; cur < n;) {
            const int p = cur + lane;
            int len = 0, dist = 0, pos;
            if (p < n) pngm::find_match(seg, p, n, cand, ncand, len, dist);
            const uint64_t sel = chain_through(len ? len : 1, __ballot(len > 0) != 0, min(64, n - cur), pos);
            if ((sel >> lane) & 1) {
                int lsym, e, extra, dsym, de, dextra;
                pngm::token_parts(seg[p], len, dist, lsym, e, extra, dsym, de, dextra);
                atomicAdd(&code.ll[lsym], 1);
                if (dsym >= 0) atomicAdd(&code.d[dsym], 1);
                fixed += (uint64_t)pngm::fixed_token_bits(lsym, e, dsym, de);
            }
            cur += pos;
        }
        const int64_t fixed_bits = 3 + (int64_t)wave_sum(fixed);         // before the end-of-block
        __syncthreads();
        if (lane == 0) dynamic_bits = pngm::dynamic_block(code);
        __syncthreads();
        dyn = dynamic_bits < fixed_bits + 7;
        if (dyn) {
            eob_bits = (int)((uint32_t)code.ll[pngm::END_OF_BLOCK] >> 16);
            eob_code = (uint32_t)code.ll[pngm::END_OF_BLOCK] & 0xFFFFu;
        }
        stored = pngm::coded_bytes(dyn ? dynamic_bits - eob_bits : fixed_bits, last, eob_bits) > (int64_t)n + 5;
    }

    uint32_t* slot = reinterpret_cast<uint32_t*>(slots + (int64_t)g * SLOT);
    int64_t bits = 0;
    int flushed = 0;
    if (!stored) {
        if (DYNAMIC && dyn) {
            const int pieces = pngm::header_pieces(code);
            for (int i0 = 0; i0 < pieces; i0 += 64) {
                uint64_t t = 0;
                int k = 0;
                if (i0 + lane < pieces) pngm::header_piece(code, i0 + lane, last, t, k);
                ring_step<DYNAMIC>(ring, slot, bits, flushed, t, k, lane);
            }
        } else {
            if (lane == 0) ring_put(ring, 0, (last ? 1u : 0u) | 2u, 3);
            bits = 3;
        }
        const int64_t give_up = ((int64_t)n + 6) * 8;    // a fixed item learns here that the stored block has won; the others know
        for (int cur = 0; cur < n && bits <= give_up;) {
            const int p = cur + lane;
            int len = 0, dist = 0, k = 0, pos;
            uint64_t t = 0;
            if (p < n) {
                pngm::find_match(seg, p, n, cand, ncand, len, dist);
                if (DYNAMIC && dyn) pngm::dynamic_token_bits(code, seg[p], len, dist, t, k);
                else pngm::token_bits(seg[p], len, dist, t, k);
            }
            const uint64_t sel = chain_through(len ? len : 1, __ballot(len > 0) != 0, min(64, n - cur), pos);
            if (!((sel >> lane) & 1)) k = 0;
            ring_step<DYNAMIC>(ring, slot, bits, flushed, t, k, lane);
            cur += pos;
        }
        stored = bits > give_up || pngm::coded_bytes(bits, last, eob_bits) > (int64_t)n + 5;
    }

    int bytes;
    if (stored) {
        uint8_t* sb = reinterpret_cast<uint8_t*>(slot);
        if (lane == 0) {
            sb[0] = last ? 1 : 0;
            sb[1] = (uint8_t)n; sb[2] = (uint8_t)(n >> 8); sb[3] = (uint8_t)~n; sb[4] = (uint8_t)(~n >> 8);
        }
        for (int i = lane; i < n; i += 64) sb[5 + i] = seg[i];
        bytes = n + 5;
    } else {
        if (lane == 0) ring_put(ring, bits, eob_code, eob_bits);
        bits += eob_bits;
        if (!last) {
            bits = (bits + 3 + 7) & ~(int64_t)7;         // an empty stored block: three zero bits, up to the byte, 00 00 FF FF
            if (lane == 0) ring_put(ring, bits, 0xFFFF0000u, 32);
            bits += 32;
        } else {
            bits = (bits + 7) & ~(int64_t)7;
        }
        __syncthreads();
        ring_flush(ring, slot, flushed, (int)((bits + 31) >> 5), lane);
        bytes = (int)(bits >> 3);
    }
    if (lane == 0) {
        uint32_t* m = meta + (int64_t)g * 4;
        m[0] = (uint32_t)bytes; m[1] = (uint32_t)(a % pngm::ADLER_MOD); m[2] = (uint32_t)(b % pngm::ADLER_MOD); m[3] = 0;
    }
}

// Gather: segment g's bytes go behind those of every segment before it.
__global__ __launch_bounds__(256) void png_gather_kernel(const uint32_t* __restrict__ meta, const uint8_t* __restrict__ slots, uint8_t* __restrict__ packed) {
    __shared__ uint64_t part[4];
    const int g = blockIdx.x, tid = threadIdx.x;
    uint64_t before = 0;
    for (int s = tid; s < g; s += 256) before += meta[(int64_t)s * 4];
    before = wave_sum(before);
    if ((tid & 63) == 0) part[tid >> 6] = before;
    __syncthreads();
    before = part[0] + part[1] + part[2] + part[3];
    const int bytes = (int)meta[(int64_t)g * 4];
    const uint8_t* src = slots + (int64_t)g * SLOT;
    uint8_t* dst = packed + before;
    for (int i = tid; i < bytes; i += 256) dst[i] = src[i];
}

}  // namespace

struct thmr_png {
    int device = 0;
    DevBuf<uint8_t> filt, slots, packed;
    DevBuf<char> desc;          // descriptors, then the segments' meta words
    PinnedBuf<char> host;       // the same, then the packed streams
    std::string err;
};

extern "C" {

int thmr_png_segment_bytes(void) { return pngm::SEGMENT; }

int64_t thmr_png_bound(int32_t width, int32_t height, int32_t channels) { return pngh::bound(width, height, channels); }

int thmr_png_encode_host(thmr_png_item* item) {
    if (!item) return g_png_err.invalid(nullptr, "null item");
    item->written = 0;
    std::string err;
    if (const int rc = pngh::check_item(*item, err)) return g_png_err.fail(nullptr, rc, err);
    try {
        pngh::encode(*item);
    } catch (const std::bad_alloc&) {
        return g_png_err.fail(nullptr, THMR_ERR_NOMEM, "out of host memory for the filtered stream");
    }
    return 0;
}

int thmr_png_code_lengths(const int32_t* freq, int32_t n, int32_t max_bits, int32_t* lens) {
    std::string err;
    if (const int rc = pngh::code_lengths(freq, n, max_bits, lens, err)) return g_png_err.fail(nullptr, rc, err);
    return 0;
}

const char* thmr_png_last_error(const thmr_png* p) { return g_png_err.read(p); }

int thmr_png_create(int32_t device, thmr_png** out) {
    return handle_create(device, out, g_png_err, "no such HIP device (without one, thmr_png_encode_host encodes on the CPU)");
}

void thmr_png_destroy(thmr_png* p) { handle_destroy(p); }

int thmr_png_encode_batch(thmr_png* p, thmr_png_item* items, int32_t n, void* stream) {
    // every argument is checked before the handle, and the handle before any HIP call: a refusal never touches the device
    if (n <= 0 || n > 65535) return g_png_err.invalid(p, "n must be 1 ... 65535");
    if (!items) return g_png_err.invalid(p, "null item table");
    std::vector<PngItemDev> ids((size_t)n);
    int64_t rows = 0, segs = 0, filt_bytes = 0, packed_bytes = 0;
    bool any_dynamic = false;
    for (int i = 0; i < n; ++i) {
        thmr_png_item& it = items[i];
        it.written = 0;
        std::string err;
        if (const int rc = pngh::check_item(it, err)) return g_png_err.fail(p, rc, "item " + std::to_string(i) + ": " + err);
        PngItemDev& d = ids[(size_t)i];
        memset(&d, 0, sizeof(d));
        d.pixels = it.pixels;
        d.im = pngh::image_of(it);
        d.total = (int32_t)pngh::stream_bytes(it.width, it.height, it.channels);
        d.filt_off = filt_bytes;
        d.row0 = (int32_t)rows; d.seg0 = (int32_t)segs; d.nseg = (int32_t)pngh::segments(d.total);
        d.ncand = pngm::candidates(it.channels, 1 + it.width * it.channels, d.cand);
        d.dynamic = it.compression == THMR_PNG_DYNAMIC;
        any_dynamic = any_dynamic || d.dynamic;
        rows += it.height; segs += d.nseg;
        filt_bytes += ((int64_t)d.total + 15 + 16) & ~(int64_t)15;        // a segment is loaded in whole 16-byte pieces
        packed_bytes += (int64_t)d.total + 5 * (int64_t)d.nseg;
        if (rows >= ((int64_t)1 << 31) || segs >= ((int64_t)1 << 24)) return g_png_err.invalid(p, "item " + std::to_string(i) + ": the batch has 2^31 rows or 2^24 segments");
    }
    if (!p) return g_png_err.invalid(p, "null handle");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e;
    bool capturing;
    if (const int rc = enter_stream(p, st, g_png_err, &capturing)) return rc;
    if (capturing)
        return g_png_err.fail(p, THMR_ERR_STATE, "thmr_png_encode_batch returns files in host memory and cannot run inside a stream capture");

    const size_t desc_bytes = (sizeof(PngItemDev) * (size_t)n + 255) & ~size_t(255);
    const size_t meta_bytes = (size_t)segs * 16;
    const size_t dbytes = desc_bytes + meta_bytes, hbytes = dbytes + (size_t)packed_bytes;
    const size_t fb = (size_t)filt_bytes, sb = (size_t)segs * SLOT, pb = (size_t)packed_bytes;
    const auto grow = {p->filt.want(fb, fb + fb / 4, "hipMalloc(filtered)"), p->slots.want(sb, sb + sb / 4, "hipMalloc(slots)"),
                       p->packed.want(pb, pb + pb / 4, "hipMalloc(packed)"), p->desc.want(dbytes, dbytes + dbytes / 4, "hipMalloc(descriptors)"),
                       p->host.want(hbytes, hbytes + hbytes / 4, "hipHostMalloc(staging)")};
    const char* what;
    if ((e = grow_synced(st, grow, what)) != hipSuccess) return g_png_err.hip(p, what, e);
    memcpy(p->host, ids.data(), sizeof(PngItemDev) * (size_t)n);
    if ((e = hipMemcpyAsync(p->desc, p->host, desc_bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return g_png_err.hip(p, "hipMemcpyAsync", e);
    const PngItemDev* idev = reinterpret_cast<const PngItemDev*>(p->desc.ptr());
    uint32_t* mdev = reinterpret_cast<uint32_t*>(p->desc.ptr() + desc_bytes);
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, idev, n, p->filt, (int)rows);
    // a batch of fixed items runs the fixed instantiation; one dynamic item sends the whole batch through the one that knows both
    if (any_dynamic) hipLaunchKernelGGL(png_deflate_kernel<true>, dim3((unsigned)segs), dim3(64), 0, st, idev, n, p->filt, p->slots, mdev);
    else hipLaunchKernelGGL(png_deflate_kernel<false>, dim3((unsigned)segs), dim3(64), 0, st, idev, n, p->filt, p->slots, mdev);
    hipLaunchKernelGGL(png_gather_kernel, dim3((unsigned)segs), dim3(256), 0, st, mdev, p->slots, p->packed);
    if ((e = hipGetLastError()) != hipSuccess) return g_png_err.hip(p, "png kernel launch", e);
    const uint32_t* mh = reinterpret_cast<const uint32_t*>(p->host.ptr() + desc_bytes);
    if ((e = hipMemcpyAsync(p->host.ptr() + desc_bytes, mdev, meta_bytes, hipMemcpyDeviceToHost, st)) != hipSuccess) return g_png_err.hip(p, "hipMemcpyAsync", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return g_png_err.hip(p, "hipStreamSynchronize", e);
    int64_t total = 0;
    for (int64_t s = 0; s < segs; ++s) {
        if (mh[s * 4] > (uint32_t)SLOT) return g_png_err.fail(p, THMR_ERR_STATE, "a segment reports more bytes than its slot holds");
        total += mh[s * 4];
    }
    if (total > packed_bytes) return g_png_err.fail(p, THMR_ERR_STATE, "the packed streams exceed their bound");
    const uint8_t* ph = reinterpret_cast<const uint8_t*>(p->host.ptr() + dbytes);
    if ((e = hipMemcpyAsync(p->host.ptr() + dbytes, p->packed, (size_t)total, hipMemcpyDeviceToHost, st)) != hipSuccess) return g_png_err.hip(p, "hipMemcpyAsync", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return g_png_err.hip(p, "hipStreamSynchronize", e);
    // The streams leave the staging for the callers' buffers in chunks, each with its CRC-32; beyond a megabyte several threads share
    // the chunks (the copy and the sum are the whole host cost of a call).  A file's CRC is combined from its chunks' afterwards.
    struct Chunk { int item; int64_t src, dst, len; uint32_t crc; };
    std::vector<Chunk> chunks;
    std::vector<int64_t> bodies((size_t)n);
    std::vector<uint32_t> adlers((size_t)n);
    int64_t at = 0;
    for (int i = 0; i < n; ++i) {
        const PngItemDev& d = ids[(size_t)i];
        uint32_t a = 1, b = 0;
        int64_t body = 0;
        for (int s = 0; s < d.nseg; ++s) {
            const uint32_t* m = mh + (int64_t)(d.seg0 + s) * 4;
            const int64_t off = (int64_t)s * pngm::SEGMENT;
            pngm::adler_append(a, b, m[1], m[2], (uint32_t)std::min<int64_t>(pngm::SEGMENT, d.total - off));
            body += m[0];
        }
        if (body > (int64_t)d.total + 5 * (int64_t)d.nseg) return g_png_err.fail(p, THMR_ERR_STATE, "item " + std::to_string(i) + ": the stream exceeds its bound");
        bodies[(size_t)i] = body; adlers[(size_t)i] = (b << 16) | a;
        for (int64_t o = 0; o < body; o += FINISH_CHUNK) chunks.push_back({i, at + o, o, std::min<int64_t>(FINISH_CHUNK, body - o), 0});
        at += body;
    }
    auto run = [&](size_t first, size_t step) {
        for (size_t k = first; k < chunks.size(); k += step) {
            Chunk& c = chunks[k];
            uint8_t* dst = items[c.item].out + pngh::IDAT_DATA_AT + 2 + c.dst;
            memcpy(dst, ph + c.src, (size_t)c.len);
            c.crc = pngh::crc32(dst, (size_t)c.len);
        }
    };
    const size_t threads = total < ((int64_t)1 << 20) ? 1 : std::min<size_t>({(size_t)FINISH_THREADS, chunks.size(), (size_t)std::max(1u, std::thread::hardware_concurrency())});
    if (threads <= 1) {
        run(0, 1);
    } else {
        std::vector<std::thread> pool;
        try {
            for (size_t t = 1; t < threads; ++t) pool.emplace_back(run, t, threads);
        } catch (const std::system_error&) {          // fewer threads than asked for: the chunks of the missing ones are done here
            for (size_t t = pool.size() + 1; t < threads; ++t) run(t, threads);
        }
        run(0, threads);
        for (std::thread& t : pool) t.join();
    }
    size_t k = 0;
    for (int i = 0; i < n; ++i) {
        uint32_t crc = 0;
        for (; k < chunks.size() && chunks[k].item == i; ++k) crc = pngh::crc32_combine(crc, chunks[k].crc, (uint64_t)chunks[k].len);
        items[i].written = pngh::finish_file(items[i].out, ids[(size_t)i].im.w, ids[(size_t)i].im.h, ids[(size_t)i].im.c, bodies[(size_t)i], adlers[(size_t)i], &crc);
    }
    return 0;
}

}  // extern "C"
