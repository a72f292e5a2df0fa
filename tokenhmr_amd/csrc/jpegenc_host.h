// The host half of the baseline JPEG encoder (include/tokenhmr_hip.h): argument checks, the quantisation and Huffman tables (Annex K,
// or the image's own with THMR_JPEG_OPTIMIZE), the
// container (SOI, APP0, DQT, SOF0, DHT, SOS ... EOI), and the whole encode on the CPU with the arithmetic of jpegenc_math.h — the oracle
// of the kernels, and what a caller without a device gets.  Host only, no HIP call.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "image_item_host.h"
#include "jpegenc_math.h"

namespace jpegeh {

using imgitem::image_of;

// Annex K, tables K.3 - K.6: codes per length 1 ... 16, then the symbols in code order.
struct HuffSpec { uint8_t bits[16]; const uint8_t* vals; int n; };
inline const HuffSpec& huff_spec(int cls, int ac) {
    static const uint8_t dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    static const uint8_t ac_luma[162] = {
        0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1,
        0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37,
        0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A,
        0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
        0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3,
        0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};
    static const uint8_t ac_chroma[162] = {
        0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1,
        0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36,
        0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
        0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A,
        0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA,
        0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};
    static const HuffSpec specs[4] = {{{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, dc_vals, 12},
                                      {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, ac_luma, 162},
                                      {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, dc_vals, 12},
                                      {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}, ac_chroma, 162}};
    return specs[cls * 2 + ac];
}

// The codes of both classes as the block coder reads them: [cls * TABLE_WORDS + symbol (DC) or 16 + symbol (AC)] = code | length << 16.
struct CodeTables {
    uint32_t t[2 * jpegem::TABLE_WORDS];
    CodeTables() {
        memset(t, 0, sizeof(t));
        for (int cls = 0; cls < 2; ++cls)
            for (int ac = 0; ac < 2; ++ac) {
                const HuffSpec& s = huff_spec(cls, ac);
                uint32_t code = 0;
                int k = 0;
                for (int len = 1; len <= 16; ++len, code <<= 1)
                    for (int i = 0; i < s.bits[len - 1]; ++i) t[cls * jpegem::TABLE_WORDS + ac * 16 + s.vals[k++]] = code++ | (uint32_t)len << 16;
            }
    }
};
inline const CodeTables& code_tables() {
    static const CodeTables T;
    return T;
}

// SOI 2, APP0 18, DQT 69 each, SOF0 10 + 3 per component, DHT 33 (DC) + 183 (AC) per class, SOS 8 + 2 per component.
inline int64_t header_bytes(int ncomp) { return ncomp == 1 ? 2 + 18 + 69 + 13 + 216 + 10 : 2 + 18 + 138 + 19 + 432 + 14; }

inline int64_t blocks(int32_t w, int32_t h, int32_t c, int32_t sub) {
    const bool s = c != 1 && sub == THMR_JPEG_420;
    const int64_t m = s ? 16 : 8;
    return ((w + m - 1) / m) * ((h + m - 1) / m) * (c == 1 ? 1 : s ? 6 : 3);
}

// Bytes the unstuffed scan of `nblk` blocks can take: every block at MAX_BLOCK_BITS (MAX_BLOCK_BITS_OPT with the image's own tables),
// and the padding to the byte.
inline int64_t scan_bytes_max(int64_t nblk, int32_t flags = 0) {
    return (nblk * ((flags & THMR_JPEG_OPTIMIZE) ? jpegem::MAX_BLOCK_BITS_OPT : jpegem::MAX_BLOCK_BITS) + 7) / 8;
}

// The worst case: a block takes at most MAX_BLOCK_BITS = 22 bits of DC (the longest DC code, 11 bits, with 11 value bits; luma's is
// 9 + 11) and 63 x (16 + 10) bits of AC, every MCU block counted as such (a dummy takes 6); each byte of the scan may be 0xFF and draw
// a zero byte behind it; then the header and EOI.  An optimised table has at most the 12 / 162 symbols of an Annex K one, so its DHT
// segment is no longer and header_bytes holds; its DC code can take 12 bits (12 symbols and the pseudo-symbol), one more per block.
inline int64_t bound(int32_t w, int32_t h, int32_t c, int32_t sub, int32_t flags = 0) {
    if (w < 1 || h < 1 || w > 65535 || h > 65535 || (c != 1 && c != 3 && c != 4) || (sub != THMR_JPEG_444 && sub != THMR_JPEG_420)) return 0;
    if (flags & ~THMR_JPEG_OPTIMIZE) return 0;
    return header_bytes(c == 1 ? 1 : 3) + 2 * scan_bytes_max(blocks(w, h, c, sub), flags) + 2;
}

// 0, or the status with the reason in err.  Pointers and capacity included.
inline int check_item(const thmr_png_item& it, int32_t quality, int32_t sub, std::string& err, int32_t flags = 0) {
    if (const int rc = imgitem::check_source(it, "reads", err)) return rc;
    if (flags & ~THMR_JPEG_OPTIMIZE) { err = "unknown flag bits " + std::to_string(flags & ~THMR_JPEG_OPTIMIZE) + " (THMR_JPEG_OPTIMIZE is the one flag)"; return THMR_ERR_INVALID; }
    if (sub == THMR_JPEG_422) { err = "unsupported: 4:2:2 subsampling (THMR_JPEG_422); the encoder writes 4:4:4 and 4:2:0"; return THMR_ERR_UNSUPPORTED; }
    if (sub != THMR_JPEG_444 && sub != THMR_JPEG_420) { err = "subsampling must be THMR_JPEG_444 or THMR_JPEG_420, got " + std::to_string(sub); return THMR_ERR_INVALID; }
    if (quality < 1 || quality > 100) { err = "quality must be 1 ... 100, got " + std::to_string(quality); return THMR_ERR_INVALID; }
    if (it.width < 1 || it.height < 1 || it.width > 65535 || it.height > 65535) {
        err = "width and height must be 1 ... 65535, got " + std::to_string(it.width) + " x " + std::to_string(it.height);
        return THMR_ERR_INVALID;
    }
    if (it.rounding != THMR_PNG_ROUND_NEAREST && it.rounding != THMR_PNG_ROUND_TRUNC) { err = "rounding must be THMR_PNG_ROUND_NEAREST or _TRUNC"; return THMR_ERR_INVALID; }
    if (it.compression != 0) { err = "compression must be 0 for a JPEG item, got " + std::to_string(it.compression); return THMR_ERR_INVALID; }
    if (flags && blocks(it.width, it.height, it.channels, sub) > jpegem::OPT_MAX_BLOCKS) {
        err = "optimised coding takes an image of at most 2^23 blocks, got " + std::to_string(blocks(it.width, it.height, it.channels, sub));
        return THMR_ERR_INVALID;
    }
    return imgitem::check_buffers(it, bound(it.width, it.height, it.channels, sub, flags), flags ? "thmr_jpeg_encode_bound_flags" : "thmr_jpeg_encode_bound", err);
}

// q[cls * 64 + zigzag position] for `quality`.
inline void quant_tables(int quality, uint16_t* q) {
    for (int cls = 0; cls < 2; ++cls)
        for (int k = 0; k < 64; ++k) q[cls * 64 + jpegem::zigzag_of_natural(k)] = (uint16_t)jpegem::quant_entry(cls, k, quality);
}

// Everything before the scan; returns its length (header_bytes, or less with the image's own tables).  opt: null for the Annex K
// tables, else the image's tables [cls * 2 + ac].
inline int64_t write_header(uint8_t* out, const jpegem::Frame& f, const uint16_t* q, const jpegem::OptimalTable* opt = nullptr) {
    uint8_t* p = out;
    auto marker = [&](int m, int len) { *p++ = 0xFF; *p++ = (uint8_t)m; *p++ = (uint8_t)(len >> 8); *p++ = (uint8_t)len; };
    *p++ = 0xFF; *p++ = 0xD8;
    marker(0xE0, 16);
    static const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    memcpy(p, jfif, 14); p += 14;
    const int ncls = f.ncomp == 1 ? 1 : 2;
    for (int cls = 0; cls < ncls; ++cls) {
        marker(0xDB, 67);
        *p++ = (uint8_t)cls;
        for (int k = 0; k < 64; ++k) *p++ = (uint8_t)q[cls * 64 + k];
    }
    marker(0xC0, 8 + 3 * f.ncomp);
    *p++ = 8;
    *p++ = (uint8_t)(f.im.h >> 8); *p++ = (uint8_t)f.im.h; *p++ = (uint8_t)(f.im.w >> 8); *p++ = (uint8_t)f.im.w;
    *p++ = (uint8_t)f.ncomp;
    for (int c = 0; c < f.ncomp; ++c) { *p++ = (uint8_t)(c + 1); *p++ = (c == 0 && f.sub) ? 0x22 : 0x11; *p++ = c ? 1 : 0; }
    for (int cls = 0; cls < ncls; ++cls)
        for (int ac = 0; ac < 2; ++ac) {
            const HuffSpec& s = huff_spec(cls, ac);
            const int n = opt ? opt[cls * 2 + ac].nsym : s.n;
            marker(0xC4, 2 + 1 + 16 + n);
            *p++ = (uint8_t)(ac << 4 | cls);
            memcpy(p, opt ? opt[cls * 2 + ac].bits + 1 : s.bits, 16); p += 16;
            memcpy(p, opt ? opt[cls * 2 + ac].huffval : s.vals, (size_t)n); p += n;
        }
    marker(0xDA, 6 + 2 * f.ncomp);
    *p++ = (uint8_t)f.ncomp;
    for (int c = 0; c < f.ncomp; ++c) { *p++ = (uint8_t)(c + 1); *p++ = c ? 0x11 : 0x00; }
    *p++ = 0; *p++ = 63; *p++ = 0;
    return p - out;
}

// MSB-first bit writer with the 0xFF 0x00 stuffing.
struct BitWriter {
    uint8_t* p;
    uint64_t acc = 0;
    int n = 0;
    void byte(uint8_t b) { *p++ = b; if (b == 0xFF) *p++ = 0; }
    void operator()(uint32_t bits, int k) {
        acc = (acc << k) | bits; n += k;
        while (n >= 8) { byte((uint8_t)(acc >> (n - 8))); n -= 8; }
    }
    void pad() { if (n) (*this)((1u << (8 - n)) - 1, 8 - n); }
};

// Every block of the scan in order through fn(cls, dummy, zz, diff): the transform and the DC prediction of the CPU encode.
template <typename Fn>
inline void for_each_block(const jpegem::Frame& f, const void* pixels, const uint16_t* q, Fn&& fn) {
    int16_t zz[64];
    int pred[3] = {0, 0, 0};
    for (int my = 0; my < f.mcuy; ++my)
        for (int mx = 0; mx < f.mcux; ++mx)
            for (int k = 0; k < f.bpm; ++k) {
                int comp, bx, by;
                bool dummy;
                jpegem::block_place(f, mx, my, k, comp, bx, by, dummy);
                const int cls = comp ? 1 : 0;
                if (dummy) { fn(cls, true, zz, 0); continue; }
                jpegem::forward_block(f, pixels, comp, bx, by, q + cls * 64, zz);
                fn(cls, false, zz, zz[0] - pred[comp]);
                pred[comp] = zz[0];
            }
}

// The statistics of the optimised mode: hist[cls * TABLE_WORDS + slot] counts what the scan codes, the dummy blocks included.
inline void histogram(const thmr_png_item& it, int32_t quality, int32_t sub, int32_t* hist) {
    const jpegem::Frame f = jpegem::frame_of(image_of(it), sub == THMR_JPEG_420);
    uint16_t q[128];
    quant_tables(quality, q);
    memset(hist, 0, sizeof(int32_t) * 2 * jpegem::TABLE_WORDS);
    for_each_block(f, it.pixels, q, [&](int cls, bool dummy, const int16_t* zz, int diff) {
        auto count = [&](int slot, uint32_t, int) { ++hist[cls * jpegem::TABLE_WORDS + slot]; };
        if (dummy) jpegem::walk_dummy(count); else jpegem::walk_block(zz, diff, count);
    });
}

// One table on the CPU, the routine of the table kernel with its steps in order.  nhist: 16 (a DC slot) or 256.  slot: null, or where
// the table's code words go (zeroed before).
inline void optimal_table(const int32_t* hist, int nhist, jpegem::OptimalTable& out, uint32_t* slot = nullptr) {
    jpegem::OptimalWork w;
    jpegem::SerialPar par;
    memset(&out, 0, sizeof(out));
    jpegem::optimal_table(hist, nhist, w, par, &out);
    if (slot) jpegem::code_words(out, w, par, slot);
}

// The whole file on the CPU.  The item is already checked.  With THMR_JPEG_OPTIMIZE the blocks are walked twice (statistics, then the
// coding with the image's own tables: the transform runs again rather than keeping every coefficient); 0, or THMR_ERR_UNSUPPORTED
// for statistics that give a code of more than 32 bits before the limit (libjpeg refuses them too).
inline int encode(thmr_png_item& it, int32_t quality, int32_t sub, int32_t flags, std::string& err) {
    const jpegem::Frame f = jpegem::frame_of(image_of(it), sub == THMR_JPEG_420);
    uint16_t q[128];
    quant_tables(quality, q);
    const uint32_t* codes = code_tables().t;
    std::vector<uint32_t> own;
    jpegem::OptimalTable opt[4];
    if (flags & THMR_JPEG_OPTIMIZE) {
        std::vector<int32_t> hist(2 * jpegem::TABLE_WORDS);
        histogram(it, quality, sub, hist.data());
        own.assign(2 * jpegem::TABLE_WORDS, 0);
        for (int cls = 0; cls < (f.ncomp == 1 ? 1 : 2); ++cls)
            for (int ac = 0; ac < 2; ++ac) {
                jpegem::OptimalTable& t = opt[cls * 2 + ac];
                optimal_table(hist.data() + cls * jpegem::TABLE_WORDS + ac * 16, ac ? 256 : 16, t, own.data() + cls * jpegem::TABLE_WORDS + ac * 16);
                if (t.nsym < 0) { err = "unsupported: the image's statistics give a Huffman code of more than 32 bits before the limit"; return THMR_ERR_UNSUPPORTED; }
            }
        codes = own.data();
    }
    BitWriter bw{it.out + write_header(it.out, f, q, (flags & THMR_JPEG_OPTIMIZE) ? opt : nullptr)};
    for_each_block(f, it.pixels, q, [&](int cls, bool dummy, const int16_t* zz, int diff) {
        if (dummy) jpegem::code_dummy(codes + cls * jpegem::TABLE_WORDS, bw); else jpegem::code_block(zz, diff, codes + cls * jpegem::TABLE_WORDS, bw);
    });
    bw.pad();
    *bw.p++ = 0xFF; *bw.p++ = 0xD9;
    it.written = bw.p - it.out;
    return 0;
}
inline void encode(thmr_png_item& it, int32_t quality, int32_t sub) {
    std::string err;
    encode(it, quality, sub, 0, err);
}

}  // namespace jpegeh
