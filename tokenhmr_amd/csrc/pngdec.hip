// PNG decoding (include/tokenhmr_hip.h).  The host entry points wrap the chunk walk and the inflate of pngdec_host.h; the
// device half runs two kernels over a whole batch: the un-filtering of every kept row into the handle's scratch plane, then the
// conversion of every window pixel.  The arithmetic of both lives in pngdec_math.h, which the CPU decode shares; item_of is
// batch_device.h's, as in jpeg.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "batch_device.h"
#include "handle_util.h"
#include "pngdec_host.h"

namespace {

thread_local ErrorSink<thmr_png_decoder> g_pngdec_err;

constexpr int BAND = pngdm::BAND_ROWS;
static_assert(BAND == 64, "a band is one row per lane of a wave: the lanes hand their pixels down with __shfl_up");

// One item as the kernels see it.  Offsets are into the call's staging (rows) and the handle's plane scratch.
struct PngItemDev {
    uint8_t* out;
    int64_t row_stride;
    int64_t rows_off;           // byte offset of this item's first kept row (its filter byte) in the staged row area
    int64_t plane_off;          // byte offset of this item's unfiltered rows
    int32_t unit0, nunits;      // this item's units are [unit0, unit0 + nunits) of the batch
    int32_t krb, bpp, colour_type, bit_depth;
    int32_t x0, yskip, w, h;    // the window: its first row is kept row `yskip`
    uint8_t palette[256][3];
};

// One unit of the un-filter grid: kept rows [row, row + nrows) of its item.  The first row's filter ignores the row above (or it is
// row 0 of the frame); so does any later row that starts a strip of its own.
struct Unit {
    int32_t row, nrows;
};

static_assert(sizeof(PngItemDev) % 8 == 0, "descriptors are read as an array");

__device__ __forceinline__ uint64_t shfl_up1(uint64_t v) {
    const uint32_t lo = __shfl_up((uint32_t)v, 1), hi = __shfl_up((uint32_t)(v >> 32), 1);
    return (uint64_t)hi << 32 | lo;
}

// One unit, BPP bytes per pixel.  Lane l owns row band + l of the current band and works on pixel t - l in step t, so the lane above
// finished that pixel one step earlier: its value arrives by a shuffle (the upper neighbour), and the one it handed over the step
// before is the upper-left neighbour.  Lane 0 reads its upper row, the last row of the band before, from the plane.
template <int BPP>
__device__ __forceinline__ void unfilter_unit(const uint8_t* __restrict__ rows, uint8_t* plane, int krb, int nrows) {
    const int lane = threadIdx.x;
    const int npix = krb / BPP;
    const int64_t stride = 1 + (int64_t)krb;
    for (int band = 0; band < nrows; band += BAND) {
        const int nb = min(BAND, nrows - band);
        const bool active = lane < nb;
        const uint8_t* src = rows + (int64_t)(band + (active ? lane : 0)) * stride;
        const int f = active ? src[0] : 0;
        ++src;
        uint8_t* dst = plane + (int64_t)(band + (active ? lane : 0)) * krb;
        const uint8_t* above = (lane == 0 && band > 0) ? dst - krb : nullptr;
        uint64_t left = 0, upleft = 0, mine = 0;
        for (int t = 0; t < npix + nb - 1; ++t) {
            const uint64_t handed = shfl_up1(mine);          // every lane takes part
            const int p = t - lane;
            if (!active || p < 0 || p >= npix) continue;
            uint64_t up = lane ? handed : 0;
            if (above) {
                up = 0;
#pragma unroll
                for (int k = 0; k < BPP; ++k) up |= (uint64_t)above[p * BPP + k] << (8 * k);
            }
            uint64_t px = 0;
#pragma unroll
            for (int k = 0; k < BPP; ++k) {
                const int a = (int)(left >> (8 * k)) & 255, b = (int)(up >> (8 * k)) & 255, c = (int)(upleft >> (8 * k)) & 255;
                const uint8_t v = pngdm::reconstruct(f, src[p * BPP + k], a, b, c);
                dst[p * BPP + k] = v;
                px |= (uint64_t)v << (8 * k);
            }
            left = px; upleft = up; mine = px;
        }
        // the band's last row is read from the plane by lane 0 of the next band
        __threadfence();
        __syncthreads();
    }
}

__global__ __launch_bounds__(BAND) void png_unfilter_kernel(const PngItemDev* __restrict__ items, int n, const Unit* __restrict__ units,
                                                            const uint8_t* __restrict__ rows, uint8_t* planes) {
    const int g = blockIdx.x;
    const int item = item_of<&PngItemDev::unit0>(items, n, g);          // items without units share a unit0 with their successor
    const PngItemDev& it = items[item];
    const Unit u = units[g];
    const int krb = it.krb;
    const uint8_t* r = rows + it.rows_off + (int64_t)u.row * (1 + (int64_t)krb);
    uint8_t* pl = planes + it.plane_off + (int64_t)u.row * krb;
    switch (it.bpp) {
        case 1: unfilter_unit<1>(r, pl, krb, u.nrows); break;
        case 2: unfilter_unit<2>(r, pl, krb, u.nrows); break;
        case 3: unfilter_unit<3>(r, pl, krb, u.nrows); break;
        case 4: unfilter_unit<4>(r, pl, krb, u.nrows); break;
        case 6: unfilter_unit<6>(r, pl, krb, u.nrows); break;
        default: unfilter_unit<8>(r, pl, krb, u.nrows); break;
    }
}

// Palette, grey, alpha, 16-bit and channel order: one thread per pixel of each window (blockIdx.y = item).
__global__ __launch_bounds__(256) void png_convert_kernel(const PngItemDev* __restrict__ items, const uint8_t* __restrict__ planes, int bgr) {
    const PngItemDev& it = items[blockIdx.y];
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)it.w * it.h) return;
    const int yy = (int)(idx / it.w), xx = (int)(idx - (int64_t)yy * it.w);
    const uint8_t* px = planes + it.plane_off + (int64_t)(it.yskip + yy) * it.krb + (int64_t)(it.x0 + xx) * it.bpp;
    uint8_t o[3];
    pngdm::to_bgr(it.colour_type, it.bit_depth, px, &it.palette[0][0], bgr, o);
    uint8_t* dst = it.out + (int64_t)yy * it.row_stride + (int64_t)xx * 3;
    dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
}

struct Stage {
    PinnedBuf<char> host;       // both of one capacity
    DevBuf<char> dev;
    hipEvent_t ev = nullptr;    // behind the last use of this set
    bool recorded = false;
};

}  // namespace

struct thmr_png_decoder {
    int device = 0;
    Stage stage[2];
    int turn = 0;
    DevBuf<uint8_t> planes;
    std::string err;
};

extern "C" {

int thmr_png_decode_band_rows(void) { return BAND; }

int thmr_png_probe(const uint8_t* data, size_t len, int32_t* info) {
    if (!info) return g_pngdec_err.invalid(nullptr, "null info");
    memset(info, 0, sizeof(int32_t) * THMR_PNG_INFO_WORDS);
    if (!data || len == 0) return g_pngdec_err.invalid(nullptr, "not a PNG: empty buffer");
    pngdh::Header h;
    std::string err;
    const int rc = pngdh::parse(data, len, true, h, err);
    if (rc) return g_pngdec_err.fail(nullptr, rc, err);
    info[THMR_PNG_INFO_HEIGHT] = h.H; info[THMR_PNG_INFO_WIDTH] = h.W; info[THMR_PNG_INFO_BIT_DEPTH] = h.depth;
    info[THMR_PNG_INFO_COLOUR_TYPE] = h.ctype; info[THMR_PNG_INFO_INTERLACE] = h.interlace;
    info[THMR_PNG_INFO_BPP] = h.unsupported ? 0 : h.bpp;
    info[THMR_PNG_INFO_SUPPORTED] = h.unsupported ? 0 : 1;
    if (h.unsupported) return g_pngdec_err.fail(nullptr, THMR_ERR_UNSUPPORTED, "unsupported PNG: " + h.why);
    return 0;
}

int thmr_png_inflate_window(const uint8_t* data, size_t len, const int32_t* window, uint8_t* rows, int64_t capacity, int32_t* plan,
                            int64_t* bytes_needed) {
    if (!plan) return g_pngdec_err.invalid(nullptr, "null plan");
    memset(plan, 0, sizeof(pngdh::Plan));
    if (bytes_needed) *bytes_needed = 0;
    if (!data || len == 0) return g_pngdec_err.invalid(nullptr, "not a PNG: empty buffer");
    std::string err;
    pngdh::Plan p;
    memset(&p, 0, sizeof(p));
    const int rc = pngdh::inflate_window(data, len, window, rows, capacity, p, bytes_needed, err);
    memcpy(plan, &p, sizeof(p));            // the words of the header, in its order (pngdec_host.h asserts the layout)
    return rc ? g_pngdec_err.fail(nullptr, rc, err) : 0;
}

int thmr_png_inflate(const uint8_t* zdata, size_t len, uint8_t* out, int64_t capacity, int64_t* written) {
    if (!written) return g_pngdec_err.invalid(nullptr, "null written");
    *written = 0;
    if (!zdata || (!out && capacity > 0) || capacity < 0) return g_pngdec_err.invalid(nullptr, "null stream or output");
    std::string err;
    const int rc = pngdh::inflate_buffer(zdata, len, out, capacity, *written, err);
    return rc ? g_pngdec_err.fail(nullptr, rc, err) : 0;
}

int thmr_png_decode_host(const uint8_t* data, size_t len, const int32_t* window, int32_t bgr, uint8_t* out, int64_t row_stride) {
    if (!data || len == 0) return g_pngdec_err.invalid(nullptr, "not a PNG: empty buffer");
    std::string err;
    const int rc = pngdh::decode(data, len, window, bgr, out, row_stride, err);
    return rc ? g_pngdec_err.fail(nullptr, rc, err) : 0;
}

const char* thmr_png_decoder_last_error(const thmr_png_decoder* d) { return g_pngdec_err.read(d); }

int thmr_png_decoder_create(int32_t device, thmr_png_decoder** out) {
    return handle_create(device, out, g_pngdec_err, "no such HIP device (without one, thmr_png_decode_host decodes on the CPU)");
}

void thmr_png_decoder_destroy(thmr_png_decoder* d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    for (Stage& s : d->stage)
        if (s.ev) { if (s.recorded) (void)hipEventSynchronize(s.ev); (void)hipEventDestroy(s.ev); }
    handle_destroy(d);
}

namespace {
struct Item {               // one entry of each of the five tables
    const uint8_t* rows;
    int32_t win_x0, win_y0, win_w, win_h;
    uint8_t* out_dev;
    int64_t row_stride;
};
}  // namespace

int thmr_png_decode_batch(thmr_png_decoder* d, const uint8_t** rows_host, const int32_t** plans_host, const int32_t* windows_host,
                          uint8_t** out_dev, const int64_t* row_strides_host, int32_t n, int32_t bgr, void* stream) {
    // every argument is checked before the handle, and the handle before any HIP call: a refusal never touches the device
    if (n <= 0 || n > 65535) return g_pngdec_err.invalid(d, "n must be 1 ... 65535");
    if (!rows_host || !plans_host || !windows_host || !out_dev || !row_strides_host) return g_pngdec_err.invalid(d, "null item table");
    std::vector<PngItemDev> ids((size_t)n);
    std::vector<int64_t> row_bytes((size_t)n, 0);
    std::vector<Unit> units;
    int64_t rows_total = 0, plane_total = 0, max_pix = 0;
    for (int i = 0; i < n; ++i) {
        const Item it{rows_host[i], windows_host[4 * i], windows_host[4 * i + 1], windows_host[4 * i + 2], windows_host[4 * i + 3], out_dev[i],
                      row_strides_host[i]};
        const std::string who = "item " + std::to_string(i) + ": ";
        if (!plans_host[i]) return g_pngdec_err.invalid(d, who + "null plan");
        pngdh::Plan p;
        memcpy(&p, plans_host[i], sizeof(p));
        const int bpp = pngdm::bytes_per_pixel(p.colour_type, p.bit_depth);
        if (bpp == 0 || p.bpp != bpp || p.height < 1 || p.width < 1 || p.height > 32767 || p.width > 32767 || p.palette_entries < 0 ||
            p.palette_entries > 256 || (p.colour_type == 3 && p.palette_entries == 0))
            return g_pngdec_err.invalid(d, who + "the plan's frame geometry / format is not one thmr_png_inflate_window produces");
        if (it.win_x0 < 0 || it.win_y0 < 0 || it.win_w < 0 || it.win_h < 0 || (int64_t)it.win_x0 + it.win_w > p.width ||
            (int64_t)it.win_y0 + it.win_h > p.height)
            return g_pngdec_err.invalid(d, who + "the window does not lie inside the frame");
        if (it.row_stride < (int64_t)it.win_w * 3) return g_pngdec_err.invalid(d, who + "row_stride is less than win_w * 3");
        PngItemDev& v = ids[(size_t)i];
        memset(&v, 0, sizeof(v));
        v.unit0 = (int32_t)units.size();
        if (it.win_w == 0 || it.win_h == 0) continue;          // nothing to write: the kernels see an empty item
        if (!it.out_dev) return g_pngdec_err.invalid(d, who + "null out_dev with a non-empty window");
        if (p.row0 < 0 || p.rows_kept < 1 || (int64_t)p.row0 + p.rows_kept > p.height || p.kept_row_bytes < bpp ||
            p.kept_row_bytes > p.width * bpp || p.kept_row_bytes % bpp != 0)
            return g_pngdec_err.invalid(d, who + "the plan's kept rows lie outside the frame");
        if (it.win_y0 < p.row0 || it.win_y0 + it.win_h > p.row0 + p.rows_kept || (int64_t)(it.win_x0 + it.win_w) * bpp > p.kept_row_bytes)
            return g_pngdec_err.invalid(d, who + "the window reaches outside what the plan kept");
        if (!it.rows) return g_pngdec_err.invalid(d, who + "null rows");
        std::string err;
        if (pngdh::check_rows(p, it.rows, err) != 0) return g_pngdec_err.invalid(d, who + err);
        if (units.size() + (size_t)p.rows_kept > ((size_t)1 << 28)) return g_pngdec_err.invalid(d, who + "more than 2^28 rows in one batch");
        v.out = it.out_dev; v.row_stride = it.row_stride;
        v.rows_off = rows_total; v.plane_off = plane_total;
        v.krb = p.kept_row_bytes; v.bpp = bpp; v.colour_type = p.colour_type; v.bit_depth = p.bit_depth;
        v.x0 = it.win_x0; v.yskip = it.win_y0 - p.row0; v.w = it.win_w; v.h = it.win_h;
        memcpy(v.palette, p.palette, sizeof(v.palette));
        // the strips, read off the filter bytes: a None or Sub row starts one.  A strip that still fits into the open unit's band joins
        // it (its first row ignores the row above whatever the lane above hands it); a longer one gets a unit of its own.
        const int64_t stride = 1 + (int64_t)p.kept_row_bytes;
        for (int32_t r = 0; r < p.rows_kept;) {
            int32_t e = r + 1;
            while (e < p.rows_kept && it.rows[(int64_t)e * stride] > 1) ++e;
            const bool first = (int32_t)units.size() == v.unit0;
            if (!first && units.back().nrows + (e - r) <= BAND) units.back().nrows += e - r;
            else units.push_back(Unit{r, e - r});
            r = e;
        }
        v.nunits = (int32_t)units.size() - v.unit0;
        row_bytes[(size_t)i] = (int64_t)p.rows_kept * stride;
        rows_total += (int64_t)p.rows_kept * stride;
        plane_total += (int64_t)p.rows_kept * p.kept_row_bytes;
        max_pix = std::max<int64_t>(max_pix, (int64_t)it.win_w * it.win_h);
    }
    if (!d) return g_pngdec_err.invalid(d, "null handle");
    if (units.empty()) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e;
    bool capturing;
    if (const int rc = enter_stream(d, st, g_pngdec_err, &capturing)) return rc;

    const size_t desc_bytes = (sizeof(PngItemDev) * (size_t)n + 255) & ~size_t(255);
    const size_t unit_bytes = (sizeof(Unit) * units.size() + 255) & ~size_t(255);
    const size_t bytes = desc_bytes + unit_bytes + (size_t)rows_total;
    Stage& s = d->stage[d->turn];
    d->turn ^= 1;
    if (!capturing && s.recorded) {
        // the upload and the kernels that last read this set (two calls ago) are done before the host writes it again
        if ((e = hipEventSynchronize(s.ev)) != hipSuccess) return g_pngdec_err.hip(d, "hipEventSynchronize", e);
        s.recorded = false;
    }
    const size_t pl = (size_t)plane_total;
    const auto grow = {s.host.want(bytes, bytes + bytes / 4, "hipHostMalloc(staging)"),
                       s.dev.want(bytes, bytes + bytes / 4, "hipMalloc(staging)"), d->planes.want(pl, pl + pl / 4, "hipMalloc(planes)")};
    if (capturing && must_grow(grow))
        return g_pngdec_err.fail(d, THMR_ERR_STATE, "the staging would grow inside a stream capture: run the call once at these sizes first");
    const char* what;
    if ((e = grow_synced(st, grow, what)) != hipSuccess) return g_pngdec_err.hip(d, what, e);
    if (!s.ev && (e = hipEventCreateWithFlags(&s.ev, hipEventDisableTiming)) != hipSuccess) return g_pngdec_err.hip(d, "hipEventCreate", e);
    memcpy(s.host, ids.data(), sizeof(PngItemDev) * (size_t)n);
    memcpy(s.host.ptr() + desc_bytes, units.data(), sizeof(Unit) * units.size());
    uint8_t* hr = reinterpret_cast<uint8_t*>(s.host.ptr() + desc_bytes + unit_bytes);
    for (int i = 0; i < n; ++i)
        if (ids[(size_t)i].nunits)
            memcpy(hr + ids[(size_t)i].rows_off, rows_host[i], (size_t)row_bytes[(size_t)i]);
    if ((e = hipMemcpyAsync(s.dev, s.host, bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return g_pngdec_err.hip(d, "hipMemcpyAsync", e);
    const PngItemDev* idev = reinterpret_cast<const PngItemDev*>(s.dev.ptr());
    const Unit* udev = reinterpret_cast<const Unit*>(s.dev.ptr() + desc_bytes);
    const uint8_t* rdev = reinterpret_cast<const uint8_t*>(s.dev.ptr() + desc_bytes + unit_bytes);
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)units.size()), dim3(BAND), 0, st, idev, n, udev, rdev, d->planes.ptr());
    hipLaunchKernelGGL(png_convert_kernel, dim3((unsigned)((max_pix + 255) / 256), (unsigned)n), dim3(256), 0, st, idev, d->planes.ptr(), bgr ? 1 : 0);
    if ((e = hipGetLastError()) != hipSuccess) return g_pngdec_err.hip(d, "png decode kernel launch", e);
    if (!capturing) {
        if ((e = hipEventRecord(s.ev, st)) != hipSuccess) return g_pngdec_err.hip(d, "hipEventRecord", e);
        s.recorded = true;
    }
    return 0;
}

}  // extern "C"
