// The sequential half of the JPEG decoder: marker parsing and Huffman decoding of a baseline frame into quantised coefficient blocks, for
// the MCU rows and blocks a window needs.  Host only and free of HIP, so a stand-alone CPU program can include it (and a sanitizer build
// of such a program can check it).  Every read of the input goes through a bounds check against `len`; every loop is bounded by the
// segment length, the MCU count of the frame, or the bits the entropy-coded segment holds.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/tokenhmr_hip.h"
#include "jpeg_math.h"

namespace jpegh {

constexpr int OK = 0, INVALID = THMR_ERR_INVALID, UNSUPPORTED = THMR_ERR_UNSUPPORTED;

static const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffTable {
    bool defined = false;
    uint8_t vals[256];
    int32_t maxcode[18];     // largest code of each length, -1 if none
    int32_t valoff[17];      // vals index of the first code of a length, minus that code
    uint16_t look[512];      // 9-bit lookahead: (length << 8) | symbol, 0 = longer than 9 bits
};

struct Component {
    int id = 0, h = 1, v = 1, tq = 0, td = 0, ta = 0;
};

struct Header {
    int H = 0, W = 0, ncomp = 0;
    Component comp[4];
    int hs = 1, vs = 1;              // luma sampling (1,1 for grey)
    int restart_interval = 0;
    bool have_sof = false, jfif = false, adobe = false;
    int adobe_transform = -1;
    uint16_t quant[4][64];           // natural order
    bool quant_defined[4] = {false, false, false, false};
    HuffTable dc[4], ac[4];
    size_t scan_pos = 0;             // first byte of the entropy-coded segment
    int unsupported = 0;             // set with `why` when the frame is well-formed but of a kind not handled
    std::string why;
};

inline int build_huff(const uint8_t* bits /*16 counts*/, const uint8_t* vals, int nvals, HuffTable& t, std::string& err) {
    memset(t.look, 0, sizeof(t.look));
    memcpy(t.vals, vals, (size_t)nvals);
    int code = 0, p = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = bits[l - 1];
        t.valoff[l] = p - code;
        if (n) {
            if (code + n > (1 << l)) { err = "DHT: the code lengths overflow the code space"; return INVALID; }
            if (l <= 9)
                for (int i = 0; i < n; ++i) {
                    const int first = (code + i) << (9 - l);
                    for (int k = 0; k < (1 << (9 - l)); ++k) t.look[first + k] = (uint16_t)((l << 8) | vals[p + i]);
                }
            p += n; code += n;
            t.maxcode[l] = code - 1;
        } else {
            t.maxcode[l] = -1;
        }
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    t.defined = true;
    return OK;
}

// Parses SOI ... SOS.  INVALID: malformed; OK with h.unsupported set: well-formed, not handled (h.why names what was found).
inline int parse_header(const uint8_t* d, size_t len, Header& h, std::string& err) {
    if (!d || len < 4 || d[0] != 0xFF || d[1] != 0xD8) { err = "not a JPEG: no SOI marker"; return INVALID; }
    size_t pos = 2;
    auto unsup = [&](const std::string& m) { if (!h.unsupported) { h.unsupported = 1; h.why = m; } };
    for (;;) {
        if (pos >= len || d[pos] != 0xFF) { err = "truncated or corrupt: a marker was expected at byte " + std::to_string(pos); return INVALID; }
        while (pos < len && d[pos] == 0xFF) ++pos;          // fill bytes
        if (pos >= len) { err = "truncated inside a marker"; return INVALID; }
        const int m = d[pos++];
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;                    // TEM / a stray RSTn: no payload
        if (m == 0xD8) { err = "a second SOI marker"; return INVALID; }
        if (m == 0xD9) { err = "EOI before any scan"; return INVALID; }
        if (m == 0x00) { err = "a stuffed 0xFF00 outside a scan"; return INVALID; }
        if (pos + 2 > len) { err = "truncated inside a segment length"; return INVALID; }
        const size_t L = ((size_t)d[pos] << 8) | d[pos + 1];
        if (L < 2 || pos + L > len) { err = "truncated: segment 0xFF" + std::to_string(m) + " runs past the end"; return INVALID; }
        const uint8_t* s = d + pos + 2;
        const size_t n = L - 2;
        pos += L;
        if (m == 0xDB) {                // DQT
            size_t i = 0;
            while (i < n) {
                const int pq = s[i] >> 4, tq = s[i] & 15;
                ++i;
                if (pq > 1) { err = "DQT: bad precision"; return INVALID; }
                if (tq > 3) { err = "DQT: table id " + std::to_string(tq) + " is above 3"; return INVALID; }
                const size_t need = pq ? 128 : 64;
                if (i + need > n) { err = "DQT: truncated table"; return INVALID; }
                for (int k = 0; k < 64; ++k)
                    h.quant[tq][kNatural[k]] = pq ? (uint16_t)((s[i + 2 * k] << 8) | s[i + 2 * k + 1]) : s[i + k];
                h.quant_defined[tq] = true;
                i += need;
            }
        } else if (m == 0xC4) {         // DHT
            size_t i = 0;
            while (i < n) {
                const int tc = s[i] >> 4, th = s[i] & 15;
                ++i;
                if (tc > 1 || th > 3) { err = "DHT: bad table class / id " + std::to_string(tc) + "/" + std::to_string(th); return INVALID; }
                if (i + 16 > n) { err = "DHT: truncated counts"; return INVALID; }
                int total = 0;
                for (int k = 0; k < 16; ++k) total += s[i + k];
                if (total > 256 || i + 16 + (size_t)total > n) { err = "DHT: truncated or oversized value list"; return INVALID; }
                const int rc = build_huff(s + i, s + i + 16, total, tc ? h.ac[th] : h.dc[th], err);
                if (rc) return rc;
                i += 16 + (size_t)total;
            }
        } else if (m == 0xC0) {         // SOF0
            if (h.have_sof) { err = "a second SOF marker"; return INVALID; }
            if (n < 6) { err = "SOF: truncated"; return INVALID; }
            const int prec = s[0];
            h.H = (s[1] << 8) | s[2]; h.W = (s[3] << 8) | s[4]; h.ncomp = s[5];
            if (n != 6 + 3 * (size_t)h.ncomp) { err = "SOF: the length does not match the component count"; return INVALID; }
            if (h.W == 0 || h.ncomp == 0) { err = "SOF: zero width or no component"; return INVALID; }
            h.have_sof = true;
            if (prec != 8) unsup(std::to_string(prec) + "-bit samples");
            if (h.H == 0) unsup("height 0 (defined later by a DNL marker)");
            if (h.ncomp != 1 && h.ncomp != 3) unsup(std::to_string(h.ncomp) + " components");
            if (h.H > 32767 || h.W > 32767) unsup("a " + std::to_string(h.W) + "x" + std::to_string(h.H) + " frame: a side above 32767");
            for (int c = 0; c < h.ncomp && c < 4; ++c) {
                Component& k = h.comp[c];
                k.id = s[6 + 3 * c]; k.h = s[7 + 3 * c] >> 4; k.v = s[7 + 3 * c] & 15; k.tq = s[8 + 3 * c];
                if (k.h < 1 || k.h > 4 || k.v < 1 || k.v > 4) { err = "SOF: sampling factor outside 1..4"; return INVALID; }
                if (k.tq > 3) { err = "SOF: quantisation table id " + std::to_string(k.tq) + " is above 3"; return INVALID; }
            }
            if (h.ncomp > 4) { err = "SOF: more than 4 components"; return INVALID; }
            if (h.ncomp == 3) {
                const Component* k = h.comp;
                const bool ok = k[1].h == 1 && k[1].v == 1 && k[2].h == 1 && k[2].v == 1 &&
                                ((k[0].h == 1 && k[0].v == 1) || (k[0].h == 2 && k[0].v == 1) || (k[0].h == 2 && k[0].v == 2));
                if (!ok) {
                    std::string f;
                    for (int c = 0; c < 3; ++c) f += (c ? "," : "") + std::to_string(k[c].h) + "x" + std::to_string(k[c].v);
                    unsup("sampling factors " + f);
                } else {
                    h.hs = k[0].h; h.vs = k[0].v;
                }
            }
        } else if ((m >= 0xC1 && m <= 0xCF) && m != 0xC4 && m != 0xC8) {
            static const char* const names[16] = {"", "extended sequential (SOF1)", "progressive (SOF2)", "lossless (SOF3)", "", "differential sequential (SOF5)",
                                                  "differential progressive (SOF6)", "differential lossless (SOF7)", "", "arithmetic-coded sequential (SOF9)",
                                                  "arithmetic-coded progressive (SOF10)", "arithmetic-coded lossless (SOF11)", "arithmetic conditioning (DAC)",
                                                  "arithmetic-coded differential sequential (SOF13)", "arithmetic-coded differential progressive (SOF14)",
                                                  "arithmetic-coded differential lossless (SOF15)"};
            unsup(std::string(names[m - 0xC0]) + " JPEG");
            if (m != 0xCC) {            // keep the geometry of the frame for the probe
                if (h.have_sof) { err = "a second SOF marker"; return INVALID; }
                if (n < 6) { err = "SOF: truncated"; return INVALID; }
                h.H = (s[1] << 8) | s[2]; h.W = (s[3] << 8) | s[4]; h.ncomp = s[5];
                h.have_sof = true;
                h.scan_pos = pos;
                return OK;              // nothing after such a frame header is interpreted
            }
        } else if (m == 0xDD) {         // DRI
            if (n != 2) { err = "DRI: bad length"; return INVALID; }
            h.restart_interval = (s[0] << 8) | s[1];
        } else if (m == 0xE0) {
            if (n >= 5 && memcmp(s, "JFIF\0", 5) == 0) h.jfif = true;
        } else if (m == 0xEE) {
            if (n >= 12 && memcmp(s, "Adobe", 5) == 0) { h.adobe = true; h.adobe_transform = s[11]; }
        } else if (m == 0xDA) {         // SOS
            if (!h.have_sof) { err = "SOS before SOF"; return INVALID; }
            if (n < 1) { err = "SOS: truncated"; return INVALID; }
            const int ns = s[0];
            if (ns < 1 || ns > 4 || n != 4 + 2 * (size_t)ns) { err = "SOS: bad component count or length"; return INVALID; }
            h.scan_pos = pos;
            if (h.unsupported) return OK;
            if (ns != h.ncomp) { unsup("a scan of " + std::to_string(ns) + " of the frame's " + std::to_string(h.ncomp) + " components (multi-scan)"); return OK; }
            for (int c = 0; c < ns; ++c) {
                Component& k = h.comp[c];
                if (s[1 + 2 * c] != k.id) { err = "SOS: component selector does not match the frame header"; return INVALID; }
                k.td = s[2 + 2 * c] >> 4; k.ta = s[2 + 2 * c] & 15;
                if (k.td > 3 || k.ta > 3) { err = "SOS: Huffman table id above 3"; return INVALID; }
                if (!h.dc[k.td].defined || !h.ac[k.ta].defined) { err = "SOS: a Huffman table the scan names was never defined"; return INVALID; }
                if (!h.quant_defined[k.tq]) { err = "SOS: a quantisation table the frame names was never defined"; return INVALID; }
            }
            const uint8_t* t = s + 1 + 2 * ns;
            if (t[0] != 0 || t[1] != 63 || t[2] != 0) { err = "SOS: spectral selection / approximation of a non-baseline scan"; return INVALID; }
            if (h.ncomp == 3) {
                if (h.adobe && h.adobe_transform == 0) unsup("Adobe APP14 transform 0 (RGB stored without a colour transform)");
                else if (!h.adobe && !h.jfif && h.comp[0].id == 'R' && h.comp[1].id == 'G' && h.comp[2].id == 'B')
                    unsup("component ids 'R','G','B' (RGB stored without a colour transform)");
            }
            return OK;
        }
        // APPn, COM and anything else with a length: skipped
    }
}

struct BitReader {
    const uint8_t* d;
    size_t pos, len;
    uint64_t buf = 0;
    int cnt = 0;        // bits in buf
    int fake = 0;       // of which zero bits fed past a marker or the end of the data (always the lowest ones)
    bool hit = false;   // a marker or the end was reached: d[pos] is the 0xFF of the marker (or pos == len)

    inline void fill() {
        while (cnt <= 56) {
            unsigned b = 0;
            if (!hit) {
                if (pos >= len) hit = true;
                else if (d[pos] != 0xFF) b = d[pos++];
                else if (pos + 1 < len && d[pos + 1] == 0) { b = 0xFF; pos += 2; }
                else hit = true;
            }
            if (hit) fake += 8;
            buf = (buf << 8) | b;
            cnt += 8;
        }
    }
    inline unsigned peek(int n) { return (unsigned)(buf >> (cnt - n)) & ((1u << n) - 1u); }
    inline void skip(int n) { cnt -= n; }
    inline bool overrun() const { return cnt < fake; }          // bits past the entropy-coded data were consumed
};

// One Huffman symbol: at most 16 bits.  -1: the code is in no table.
inline int decode_symbol(BitReader& br, const HuffTable& t) {
    if (br.cnt < 16) br.fill();
    const unsigned e = t.look[br.peek(9)];
    if (e) { br.skip(e >> 8); return e & 255; }
    int l = 10;
    int code = (int)br.peek(10);
    while (l <= 16 && code > t.maxcode[l]) { ++l; if (l <= 16) code = (int)br.peek(l); }
    if (l > 16) return -1;
    br.skip(l);
    const int idx = code + t.valoff[l];
    return (idx >= 0 && idx < 256) ? t.vals[idx] : -1;
}

inline int receive_extend(BitReader& br, int s) {
    if (br.cnt < s) br.fill();
    const int v = (int)br.peek(s);
    br.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One block: blk (64 int16, zeroed by the caller) or null to decode and discard.
inline int decode_block(BitReader& br, const HuffTable& dc, const HuffTable& ac, int& pred, int16_t* blk, std::string& err) {
    int s = decode_symbol(br, dc);
    if (s < 0) { err = "a DC code that is not in its Huffman table"; return INVALID; }
    if (s > 15) { err = "a DC coefficient of more than 15 bits"; return INVALID; }
    if (s) pred = (int)((uint32_t)pred + (uint32_t)receive_extend(br, s));
    if (blk) blk[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {
        const int rs = decode_symbol(br, ac);
        if (rs < 0) { err = "an AC code that is not in its Huffman table"; return INVALID; }
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;         // EOB
            k += 16;
            continue;
        }
        k += r;
        if (k > 63) { err = "a coefficient index past 63"; return INVALID; }
        const int v = receive_extend(br, s);
        if (blk) blk[kNatural[k]] = (int16_t)v;
        ++k;
    }
    if (br.overrun()) { err = "the entropy-coded data ends (truncated file, or a marker) inside the MCU rows the window needs"; return INVALID; }
    return OK;
}

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// The block rectangle of each component that a non-empty window inside the frame needs.
inline void required_blocks(int H, int W, int ncomp, int hs, int vs, int x0, int y0, int w, int ht, int32_t* bx0, int32_t* by0, int32_t* bw,
                            int32_t* bh) {
    for (int c = 0; c < ncomp; ++c) {
        const int sx = c ? hs : 1, sy = c ? vs : 1;                 // this component's sub-sampling against the frame
        int a0, a1, b0, b1;
        jpegm::comp_sample_range(x0, w, sx, ceil_div(W, sx), a0, a1);
        jpegm::comp_sample_range(y0, ht, sy, ceil_div(H, sy), b0, b1);
        bx0[c] = a0 >> 3; bw[c] = (a1 >> 3) - bx0[c] + 1;
        by0[c] = b0 >> 3; bh[c] = (b1 >> 3) - by0[c] + 1;
    }
}

// The plan of a window: block rectangles, MCU rows, quantisation tables.  Needs a supported header.
inline int make_plan(const Header& h, const int32_t* window, thmr_jpeg_plan& p, std::string& err) {
    memset(&p, 0, sizeof(p));
    int x0 = 0, y0 = 0, w = h.W, ht = h.H;
    if (window) { x0 = window[0]; y0 = window[1]; w = window[2]; ht = window[3]; }
    if (x0 < 0 || y0 < 0 || w < 0 || ht < 0 || (int64_t)x0 + w > h.W || (int64_t)y0 + ht > h.H) {
        err = "the window does not lie inside the " + std::to_string(h.W) + "x" + std::to_string(h.H) + " frame";
        return INVALID;
    }
    p.height = h.H; p.width = h.W; p.components = h.ncomp; p.h_samp = h.hs; p.v_samp = h.vs;
    p.win_x0 = x0; p.win_y0 = y0; p.win_w = w; p.win_h = ht;
    for (int c = 0; c < h.ncomp; ++c) memcpy(p.quant[c], h.quant[h.comp[c].tq], sizeof(p.quant[c]));
    if (w == 0 || ht == 0) return OK;
    int mcu_lo = 0x7fffffff, mcu_hi = -1, blocks = 0;
    required_blocks(h.H, h.W, h.ncomp, h.hs, h.vs, x0, y0, w, ht, p.bx0, p.by0, p.bw, p.bh);
    for (int c = 0; c < h.ncomp; ++c) {
        p.coef_block[c] = blocks;
        blocks += p.bw[c] * p.bh[c];
        const int vblk = c ? 1 : h.vs;                               // block rows of this component per MCU row
        mcu_lo = p.by0[c] / vblk < mcu_lo ? p.by0[c] / vblk : mcu_lo;
        const int hi = (p.by0[c] + p.bh[c] - 1) / vblk;
        mcu_hi = hi > mcu_hi ? hi : mcu_hi;
    }
    p.n_blocks = blocks;
    p.mcu_row0 = mcu_lo; p.mcu_rows_kept = mcu_hi - mcu_lo + 1;
    return OK;
}

// Entropy-decodes MCU rows 0 .. the last one the plan needs, keeping the plan's blocks in coef (p.n_blocks * 64 int16).
inline int entropy_decode(const uint8_t* d, size_t len, const Header& h, thmr_jpeg_plan& p, int16_t* coef, std::string& err) {
    p.mcu_rows_decoded = 0;
    if (p.n_blocks == 0) return OK;
    const int mcu_w = 8 * h.hs, mcu_h = 8 * h.vs;
    const int mcus_x = ceil_div(h.W, mcu_w), mcus_y = ceil_div(h.H, mcu_h);
    const int last_row = p.mcu_row0 + p.mcu_rows_kept - 1;
    if (last_row >= mcus_y) { err = "plan: MCU rows outside the frame"; return INVALID; }
    BitReader br{d, h.scan_pos, len};
    int pred[3] = {0, 0, 0};
    int until_restart = h.restart_interval, next_rst = 0;
    for (int my = 0; my <= last_row; ++my) {
        for (int mx = 0; mx < mcus_x; ++mx) {
            if (h.restart_interval && until_restart == 0) {
                // byte-align, then the marker RSTn must follow (bytes a corrupt file leaves before it are skipped, as libjpeg does)
                br.buf = 0; br.cnt = 0; br.fake = 0; br.hit = false;
                size_t q = br.pos;
                while (q < len && d[q] != 0xFF) ++q;
                while (q < len && d[q] == 0xFF) ++q;
                if (q >= len || d[q] != 0xD0 + next_rst) { err = "the restart marker RST" + std::to_string(next_rst) + " is missing"; return INVALID; }
                br.pos = q + 1;
                next_rst = (next_rst + 1) & 7;
                until_restart = h.restart_interval;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < h.ncomp; ++c) {
                const int nh = c ? 1 : h.hs, nv = c ? 1 : h.vs;
                const HuffTable& dc = h.dc[h.comp[c].td];
                const HuffTable& ac = h.ac[h.comp[c].ta];
                for (int v = 0; v < nv; ++v)
                    for (int u = 0; u < nh; ++u) {
                        const int bx = mx * nh + u - p.bx0[c], by = my * nv + v - p.by0[c];
                        int16_t* blk = nullptr;
                        if (bx >= 0 && bx < p.bw[c] && by >= 0 && by < p.bh[c]) {
                            blk = coef + ((int64_t)p.coef_block[c] + (int64_t)by * p.bw[c] + bx) * 64;
                            memset(blk, 0, 128);
                        }
                        const int rc = decode_block(br, dc, ac, pred[c], blk, err);
                        if (rc) return rc;
                    }
            }
            if (h.restart_interval) --until_restart;
        }
        p.mcu_rows_decoded = my + 1;
    }
    return OK;
}

// The CPU half of the device stage: planes of the plan's block rectangles, then the window's pixels.  planes: scratch of
// plane_bytes(p) bytes.
inline int64_t plane_bytes(const thmr_jpeg_plan& p) {
    int64_t n = 0;
    for (int c = 0; c < p.components; ++c) n += (int64_t)p.bw[c] * p.bh[c] * 64;
    return n;
}

inline void reconstruct(const thmr_jpeg_plan& p, const int16_t* coef, uint8_t* planes, int bgr, uint8_t* out, int64_t row_stride) {
    jpegm::Plane pl[3];
    int64_t off = 0;
    for (int c = 0; c < p.components; ++c) {
        pl[c] = jpegm::Plane{planes + off, 8 * p.bw[c], 8 * p.bx0[c], 8 * p.by0[c]};
        for (int by = 0; by < p.bh[c]; ++by)
            for (int bx = 0; bx < p.bw[c]; ++bx) {
                uint8_t px[64];
                jpegm::idct_block(coef + ((int64_t)p.coef_block[c] + (int64_t)by * p.bw[c] + bx) * 64, p.quant[c], px);
                for (int r = 0; r < 8; ++r) memcpy(planes + off + ((int64_t)by * 8 + r) * pl[c].stride + bx * 8, px + r * 8, 8);
            }
        off += (int64_t)p.bw[c] * p.bh[c] * 64;
    }
    const int cw = ceil_div(p.width, p.h_samp), ch = ceil_div(p.height, p.v_samp);
    for (int yy = 0; yy < p.win_h; ++yy)
        for (int xx = 0; xx < p.win_w; ++xx) {
            const int x = p.win_x0 + xx, y = p.win_y0 + yy;
            int r, g, b;
            const int Y = jpegm::at(pl[0], y, x);
            if (p.components == 1) {
                r = g = b = Y;
            } else {
                jpegm::ycc_to_rgb(Y, jpegm::chroma_at(pl[1], p.h_samp, p.v_samp, cw, ch, x, y),
                                  jpegm::chroma_at(pl[2], p.h_samp, p.v_samp, cw, ch, x, y), r, g, b);
            }
            uint8_t* o = out + yy * row_stride + (int64_t)xx * 3;
            o[0] = (uint8_t)(bgr ? b : r); o[1] = (uint8_t)g; o[2] = (uint8_t)(bgr ? r : b);
        }
}

}  // namespace jpegh
