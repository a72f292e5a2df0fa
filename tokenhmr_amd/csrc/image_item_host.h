// What the PNG and the JPEG encoder do with a thmr_png_item (include/tokenhmr_hip.h) before they differ: the image it describes, and
// the head and the tail of its argument check.  Each encoder's check_item puts its own tests (sizes, limits, modes) between the two, so
// an item with two faults is refused for the same one by both as far as they share it.  Host only, no HIP call.
#pragma once
#include <stdint.h>

#include <string>

#include "../../include/tokenhmr_hip.h"
#include "image_source.h"

namespace imgitem {

static_assert(sizeof(thmr_png_item) == 88, "tokenhmr_amd/_cabi.py mirrors this layout");

inline imgsrc::Image image_of(const thmr_png_item& it) {
    return imgsrc::Image{it.dtype, it.width, it.height, it.channels, it.stride_y, it.stride_x, it.stride_c, it.scale, it.rounding, it.swap_rb ? 1 : 0};
}

// The head of a check: dtype, then channels.  0, or the status with the reason in err.  verb: what the encoder does with 1, 3 or 4
// channels ("writes" them, "reads" them).
inline int check_source(const thmr_png_item& it, const char* verb, std::string& err) {
    if (it.dtype == THMR_PNG_U16) { err = "unsupported: 16-bit samples (dtype THMR_PNG_U16); the encoder writes 8-bit files"; return THMR_ERR_UNSUPPORTED; }
    if (it.dtype != THMR_PNG_U8 && it.dtype != THMR_PNG_F32) { err = "dtype must be THMR_PNG_U8 or THMR_PNG_F32"; return THMR_ERR_INVALID; }
    if (it.channels == 2) { err = std::string("unsupported: 2 channels (grey + alpha); the encoder ") + verb + " 1, 3 or 4"; return THMR_ERR_UNSUPPORTED; }
    if (it.channels != 1 && it.channels != 3 && it.channels != 4) { err = "channels must be 1, 3 or 4, got " + std::to_string(it.channels); return THMR_ERR_INVALID; }
    return 0;
}

// The tail: the pointers, then the capacity against `need`, the value of the entry point `bound_name`.
inline int check_buffers(const thmr_png_item& it, int64_t need, const char* bound_name, std::string& err) {
    if (!it.pixels) { err = "null pixels"; return THMR_ERR_INVALID; }
    if (!it.out) { err = "null out"; return THMR_ERR_INVALID; }
    if (it.capacity < need) {
        err = "capacity " + std::to_string(it.capacity) + " is below " + bound_name + " = " + std::to_string(need);
        return THMR_ERR_INVALID;
    }
    return 0;
}

}  // namespace imgitem
