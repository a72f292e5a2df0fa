// Baseline JPEG decoding (include/tokenhmr_hip.h).  The host entry points wrap the parser and entropy decoder of jpeg_host.h;
// the device half runs two kernels over a whole batch: the dequantising JDCT_ISLOW inverse DCT of every kept block into component planes,
// then fancy upsampling + colour conversion of every window.  The arithmetic of both lives in jpeg_math.h, which the CPU decode shares;
// item_of is batch_device.h's, as in the two encoders (png.hip, jpegenc.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "batch_device.h"
#include "handle_util.h"
#include "jpeg_host.h"

namespace {

thread_local ErrorSink<thmr_jpeg> g_jpeg_err{true};      // also behind thmr_last_error(NULL)

// One item as the kernels see it.  Offsets are into the call's staging (coefficients) and the handle's plane scratch.
struct JpegItemDev {
    uint8_t* out;
    int64_t row_stride;
    int64_t coef_off;           // int16 index of this item's first coefficient in the staged coefficient area
    int64_t plane_off[3];       // byte offset of each component's plane
    int32_t blk0, nblk;         // this item's blocks are [blk0, blk0 + nblk) of the batch
    int32_t ncomp, hs, vs, cw, ch;
    int32_t x0, y0, w, h;
    int32_t bx0[3], by0[3], bw[3], bh[3], cblk[3];
    uint16_t q[3][64];
};

static_assert(sizeof(thmr_jpeg_info) == 32 && sizeof(thmr_jpeg_plan) == 496 && sizeof(thmr_jpeg_item) == 48, "tokenhmr_amd/_cabi.py mirrors these layouts");
static_assert(sizeof(JpegItemDev) % 8 == 0, "descriptors are read as an array");

constexpr int IDCT_BLOCKS = 32;      // 8x8 blocks per 256-thread workgroup: one block per 8 lanes

// Dequantise + inverse DCT.  Lane j of a block's 8 lanes takes column j in pass 1 and row j in pass 2; the 8x8 workspace is transposed
// through LDS (rows padded to 9 words: pass 1 writes a column of it per lane, pass 2 reads a row).  Each lane stores its row's 8 samples
// with one aligned 8-byte store.
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JpegItemDev* __restrict__ items, int n, const int16_t* __restrict__ coef,
                                                        uint8_t* __restrict__ planes, int total_blocks) {
    __shared__ int ws[IDCT_BLOCKS][8][9];
    const int j = threadIdx.x & 7, lb = threadIdx.x >> 3;
    const int g = blockIdx.x * IDCT_BLOCKS + lb;
    const bool live = g < total_blocks;
    int item = 0, c = 0, local = 0;
    if (live) {
        item = item_of<&JpegItemDev::blk0>(items, n, g);          // items without blocks share a blk0 with their successor
        local = g - items[item].blk0;
        if (items[item].ncomp == 3) c = local >= items[item].cblk[2] ? 2 : local >= items[item].cblk[1] ? 1 : 0;
        const int16_t* src = coef + items[item].coef_off + (int64_t)local * 64;
        const uint16_t* q = items[item].q[c];
        int v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = jpegm::mul(src[r * 8 + j], q[r * 8 + j]);
        jpegm::idct8(v, jpegm::CONST_BITS - jpegm::PASS1_BITS);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[lb][r][j] = v[r];
    }
    __syncthreads();
    if (live) {
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = ws[lb][j][k];
        jpegm::idct8(v, jpegm::CONST_BITS + jpegm::PASS1_BITS + 3);
        uint32_t w0 = 0, w1 = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            w0 |= (uint32_t)jpegm::range_limit_idct(v[k]) << (8 * k);
            w1 |= (uint32_t)jpegm::range_limit_idct(v[4 + k]) << (8 * k);
        }
        const int in_comp = local - items[item].cblk[c];
        const int bw = items[item].bw[c];
        const int by = in_comp / bw, bx = in_comp - by * bw;
        uint8_t* dst = planes + items[item].plane_off[c] + ((int64_t)by * 8 + j) * (8 * bw) + bx * 8;
        *reinterpret_cast<uint2*>(dst) = make_uint2(w0, w1);        // plane offsets and row strides are multiples of 8
    }
}

// Upsampling + colour: one thread per pixel of each window (blockIdx.y = item).
__global__ __launch_bounds__(256) void jpeg_colour_kernel(const JpegItemDev* __restrict__ items, const uint8_t* __restrict__ planes, int bgr) {
    const JpegItemDev& it = items[blockIdx.y];
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)it.w * it.h) return;
    const int yy = (int)(idx / it.w), xx = (int)(idx - (int64_t)yy * it.w);
    const int x = it.x0 + xx, y = it.y0 + yy;
    const jpegm::Plane py{planes + it.plane_off[0], 8 * it.bw[0], 8 * it.bx0[0], 8 * it.by0[0]};
    int r, g, b;
    const int Y = jpegm::at(py, y, x);
    if (it.ncomp == 1) {
        r = g = b = Y;
    } else {
        const jpegm::Plane pb{planes + it.plane_off[1], 8 * it.bw[1], 8 * it.bx0[1], 8 * it.by0[1]};
        const jpegm::Plane pr{planes + it.plane_off[2], 8 * it.bw[2], 8 * it.bx0[2], 8 * it.by0[2]};
        jpegm::ycc_to_rgb(Y, jpegm::chroma_at(pb, it.hs, it.vs, it.cw, it.ch, x, y), jpegm::chroma_at(pr, it.hs, it.vs, it.cw, it.ch, x, y), r, g, b);
    }
    uint8_t* o = it.out + (int64_t)yy * it.row_stride + (int64_t)xx * 3;
    o[0] = (uint8_t)(bgr ? b : r); o[1] = (uint8_t)g; o[2] = (uint8_t)(bgr ? r : b);
}

struct Stage {
    PinnedBuf<char> host;       // both of one capacity
    DevBuf<char> dev;
    hipEvent_t ev = nullptr;    // behind the last use of this set
    bool recorded = false;
};

int parse_supported(const uint8_t* data, size_t len, jpegh::Header& h, std::string& err) {
    const int rc = jpegh::parse_header(data, len, h, err);
    if (rc) return rc;
    if (h.unsupported) { err = "unsupported JPEG: " + h.why; return THMR_ERR_UNSUPPORTED; }
    return 0;
}

}  // namespace

struct thmr_jpeg {
    int device = 0;
    Stage stage[2];
    int turn = 0;
    DevBuf<uint8_t> planes;
    std::string err;
};

extern "C" {

int thmr_jpeg_probe(const uint8_t* data, size_t len, thmr_jpeg_info* info) {
    if (!info) return g_jpeg_err.invalid(nullptr, "null info");
    memset(info, 0, sizeof(*info));
    if (!data || len == 0) return g_jpeg_err.invalid(nullptr, "not a JPEG: empty buffer");
    jpegh::Header h;
    std::string err;
    const int rc = jpegh::parse_header(data, len, h, err);
    if (rc) return g_jpeg_err.fail(nullptr, rc, err);
    info->height = h.H; info->width = h.W; info->components = h.ncomp;
    info->h_samp = h.hs; info->v_samp = h.vs; info->restart_interval = h.restart_interval;
    info->supported = h.unsupported ? 0 : 1;
    if (h.unsupported) return g_jpeg_err.fail(nullptr, THMR_ERR_UNSUPPORTED, "unsupported JPEG: " + h.why);
    return 0;
}

int thmr_jpeg_entropy_decode(const uint8_t* data, size_t len, const int32_t* window, int16_t* coef, int64_t coef_capacity_blocks,
                             thmr_jpeg_plan* plan) {
    if (!plan) return g_jpeg_err.invalid(nullptr, "null plan");
    memset(plan, 0, sizeof(*plan));
    if (!data || len == 0) return g_jpeg_err.invalid(nullptr, "not a JPEG: empty buffer");
    jpegh::Header h;
    std::string err;
    int rc = parse_supported(data, len, h, err);
    if (rc) return g_jpeg_err.fail(nullptr, rc, err);
    if ((rc = jpegh::make_plan(h, window, *plan, err)) != 0) return g_jpeg_err.fail(nullptr, rc, err);
    if (!coef) return 0;
    if (coef_capacity_blocks < plan->n_blocks)
        return g_jpeg_err.invalid(nullptr, "the coefficient buffer holds " + std::to_string(coef_capacity_blocks) + " blocks, the window needs " +
                                                    std::to_string(plan->n_blocks));
    if ((rc = jpegh::entropy_decode(data, len, h, *plan, coef, err)) != 0) return g_jpeg_err.fail(nullptr, rc, err);
    return 0;
}

int thmr_jpeg_decode_host(const uint8_t* data, size_t len, const int32_t* window, int32_t bgr, uint8_t* out, int64_t row_stride) {
    if (!data || len == 0) return g_jpeg_err.invalid(nullptr, "not a JPEG: empty buffer");
    jpegh::Header h;
    std::string err;
    thmr_jpeg_plan plan;
    int rc = parse_supported(data, len, h, err);
    if (rc) return g_jpeg_err.fail(nullptr, rc, err);
    if ((rc = jpegh::make_plan(h, window, plan, err)) != 0) return g_jpeg_err.fail(nullptr, rc, err);
    if (plan.n_blocks == 0) return 0;
    if (!out) return g_jpeg_err.invalid(nullptr, "null out");
    if (row_stride < (int64_t)plan.win_w * 3) return g_jpeg_err.invalid(nullptr, "row_stride is less than win_w * 3");
    std::vector<int16_t> coef;
    std::vector<uint8_t> planes;
    try {
        coef.resize((size_t)plan.n_blocks * 64);
        planes.resize((size_t)jpegh::plane_bytes(plan));
    } catch (const std::bad_alloc&) {
        return g_jpeg_err.fail(nullptr, THMR_ERR_NOMEM, "out of host memory for the coefficient blocks");
    }
    if ((rc = jpegh::entropy_decode(data, len, h, plan, coef.data(), err)) != 0) return g_jpeg_err.fail(nullptr, rc, err);
    jpegh::reconstruct(plan, coef.data(), planes.data(), bgr, out, row_stride);
    return 0;
}

const char* thmr_jpeg_last_error(const thmr_jpeg* j) { return g_jpeg_err.read(j); }

int thmr_jpeg_create(int32_t device, thmr_jpeg** out) {
    return handle_create(device, out, g_jpeg_err, "no such HIP device (without one, thmr_jpeg_decode_host decodes on the CPU)");
}

void thmr_jpeg_destroy(thmr_jpeg* j) {
    if (!j) return;
    (void)hipSetDevice(j->device);
    for (Stage& s : j->stage)
        if (s.ev) { if (s.recorded) (void)hipEventSynchronize(s.ev); (void)hipEventDestroy(s.ev); }
    handle_destroy(j);
}

int thmr_jpeg_decode_batch(thmr_jpeg* j, const thmr_jpeg_item* items, int32_t n, int32_t bgr, void* stream) {
    // every argument is checked before the handle, and the handle before any HIP call: a refusal never touches the device
    if (n <= 0 || n > 65535) return g_jpeg_err.invalid(j, "n must be 1 ... 65535");
    if (!items) return g_jpeg_err.invalid(j, "null item table");
    std::vector<JpegItemDev> ids((size_t)n);
    int64_t total_blocks = 0, plane_total = 0, coef_total = 0, max_pix = 0;
    for (int i = 0; i < n; ++i) {
        const thmr_jpeg_item& it = items[i];
        const std::string who = "item " + std::to_string(i) + ": ";
        if (!it.plan) return g_jpeg_err.invalid(j, who + "null plan");
        const thmr_jpeg_plan& p = *it.plan;
        const bool samp_ok = p.components == 1 ? (p.h_samp == 1 && p.v_samp == 1)
                                               : ((p.h_samp == 1 && p.v_samp == 1) || (p.h_samp == 2 && (p.v_samp == 1 || p.v_samp == 2)));
        if ((p.components != 1 && p.components != 3) || !samp_ok || p.height < 1 || p.width < 1 || p.height > 32767 || p.width > 32767)
            return g_jpeg_err.invalid(j, who + "the plan's frame geometry / sampling is not one thmr_jpeg_entropy_decode produces");
        if (it.win_x0 < 0 || it.win_y0 < 0 || it.win_w < 0 || it.win_h < 0 || (int64_t)it.win_x0 + it.win_w > p.width ||
            (int64_t)it.win_y0 + it.win_h > p.height)
            return g_jpeg_err.invalid(j, who + "the window does not lie inside the frame");
        if (it.row_stride < (int64_t)it.win_w * 3) return g_jpeg_err.invalid(j, who + "row_stride is less than win_w * 3");
        JpegItemDev& d = ids[(size_t)i];
        memset(&d, 0, sizeof(d));
        d.blk0 = (int32_t)total_blocks;
        d.ncomp = p.components; d.hs = p.h_samp; d.vs = p.v_samp;
        d.cw = jpegh::ceil_div(p.width, p.h_samp); d.ch = jpegh::ceil_div(p.height, p.v_samp);
        if (it.win_w == 0 || it.win_h == 0) continue;          // nothing to write: the kernels see an empty item
        if (!it.out_dev) return g_jpeg_err.invalid(j, who + "null out_dev with a non-empty window");
        int32_t rx0[3], ry0[3], rw[3], rh[3];
        jpegh::required_blocks(p.height, p.width, p.components, p.h_samp, p.v_samp, it.win_x0, it.win_y0, it.win_w, it.win_h, rx0, ry0, rw, rh);
        int64_t blocks = 0;
        for (int c = 0; c < p.components; ++c) {
            const int gw = jpegh::ceil_div(jpegh::ceil_div(p.width, c ? p.h_samp : 1), 8), gh = jpegh::ceil_div(jpegh::ceil_div(p.height, c ? p.v_samp : 1), 8);
            if (p.bx0[c] < 0 || p.by0[c] < 0 || p.bw[c] < 1 || p.bh[c] < 1 || (int64_t)p.bx0[c] + p.bw[c] > gw || (int64_t)p.by0[c] + p.bh[c] > gh)
                return g_jpeg_err.invalid(j, who + "the plan's block rectangle of component " + std::to_string(c) + " lies outside the component");
            if (p.bx0[c] > rx0[c] || p.by0[c] > ry0[c] || p.bx0[c] + p.bw[c] < rx0[c] + rw[c] || p.by0[c] + p.bh[c] < ry0[c] + rh[c])
                return g_jpeg_err.invalid(j, who + "the plan's block rectangle of component " + std::to_string(c) + " does not cover the window");
            if (p.coef_block[c] != blocks) return g_jpeg_err.invalid(j, who + "the plan's coefficient offsets are not the packed layout");
            blocks += (int64_t)p.bw[c] * p.bh[c];
        }
        if (p.n_blocks != blocks) return g_jpeg_err.invalid(j, who + "the plan's block count does not match its rectangles");
        if (!it.coef) return g_jpeg_err.invalid(j, who + "null coefficients");
        if (total_blocks + blocks > (int64_t)1 << 28) return g_jpeg_err.invalid(j, who + "more than 2^28 blocks in one batch");
        d.out = it.out_dev; d.row_stride = it.row_stride;
        d.x0 = it.win_x0; d.y0 = it.win_y0; d.w = it.win_w; d.h = it.win_h;
        d.nblk = (int32_t)blocks;
        d.coef_off = coef_total;
        for (int c = 0; c < p.components; ++c) {
            d.bx0[c] = p.bx0[c]; d.by0[c] = p.by0[c]; d.bw[c] = p.bw[c]; d.bh[c] = p.bh[c]; d.cblk[c] = p.coef_block[c];
            d.plane_off[c] = plane_total + (int64_t)p.coef_block[c] * 64;
            memcpy(d.q[c], p.quant[c], sizeof(d.q[c]));
        }
        total_blocks += blocks; plane_total += blocks * 64; coef_total += blocks * 64;
        max_pix = std::max<int64_t>(max_pix, (int64_t)it.win_w * it.win_h);
    }
    if (!j) return g_jpeg_err.invalid(j, "null handle");
    if (total_blocks == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e;
    bool capturing;
    if (const int rc = enter_stream(j, st, g_jpeg_err, &capturing)) return rc;

    const size_t desc_bytes = (sizeof(JpegItemDev) * (size_t)n + 255) & ~size_t(255);
    const size_t bytes = desc_bytes + (size_t)coef_total * sizeof(int16_t);
    Stage& s = j->stage[j->turn];
    j->turn ^= 1;
    if (!capturing && s.recorded) {
        // the upload and the kernels that last read this set (two calls ago) are done before the host writes it again
        if ((e = hipEventSynchronize(s.ev)) != hipSuccess) return g_jpeg_err.hip(j, "hipEventSynchronize", e);
        s.recorded = false;
    }
    const size_t pl = (size_t)plane_total;
    const auto grow = {s.host.want(bytes, bytes + bytes / 4, "hipHostMalloc(staging)"),
                       s.dev.want(bytes, bytes + bytes / 4, "hipMalloc(staging)"), j->planes.want(pl, pl + pl / 4, "hipMalloc(planes)")};
    if (capturing && must_grow(grow))
        return g_jpeg_err.fail(j, THMR_ERR_STATE, "the staging would grow inside a stream capture: run the call once at these sizes first");
    const char* what;
    if ((e = grow_synced(st, grow, what)) != hipSuccess) return g_jpeg_err.hip(j, what, e);
    if (!s.ev && (e = hipEventCreateWithFlags(&s.ev, hipEventDisableTiming)) != hipSuccess) return g_jpeg_err.hip(j, "hipEventCreate", e);
    memcpy(s.host, ids.data(), sizeof(JpegItemDev) * (size_t)n);
    int16_t* hc = reinterpret_cast<int16_t*>(s.host.ptr() + desc_bytes);
    for (int i = 0; i < n; ++i)
        if (ids[(size_t)i].nblk) memcpy(hc + ids[(size_t)i].coef_off, items[i].coef, (size_t)ids[(size_t)i].nblk * 128);
    if ((e = hipMemcpyAsync(s.dev, s.host, bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return g_jpeg_err.hip(j, "hipMemcpyAsync", e);
    const JpegItemDev* idev = reinterpret_cast<const JpegItemDev*>(s.dev.ptr());
    const int16_t* cdev = reinterpret_cast<const int16_t*>(s.dev.ptr() + desc_bytes);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((total_blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS)), dim3(256), 0, st, idev, n, cdev,
                       j->planes, (int)total_blocks);
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((max_pix + 255) / 256), (unsigned)n), dim3(256), 0, st, idev, j->planes, bgr ? 1 : 0);
    if ((e = hipGetLastError()) != hipSuccess) return g_jpeg_err.hip(j, "jpeg kernel launch", e);
    if (!capturing) {
        if ((e = hipEventRecord(s.ev, st)) != hipSuccess) return g_jpeg_err.hip(j, "hipEventRecord", e);
        s.recorded = true;
    }
    return 0;
}

}  // extern "C"
