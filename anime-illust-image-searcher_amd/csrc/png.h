// png.h -- what png.hip offers the batch entry in jpeg.hip (hipts_decode_batch_u8): header checks and the launch of the unfilter kernel
// over images whose slots already lie in device memory.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "png_slot.h"

namespace hipts {

constexpr int PNG_CHUNK = 64;            // images per launch: their descriptors travel in the kernel arguments
constexpr size_t PNG_STAGE_PAD = 32;     // bytes the kernel may read past a slot's last scanline (whole aligned words of the last pixel group)

struct PngImage {
    const uint8_t* src;                  // device: the slot's scanlines (behind the header), height rows of 1 + width * channels bytes
    uint8_t* rgb;                        // device: uint8 [height][width][3]
    int32_t width, height, channels, pad;
};

// checks a slot header against the slot's size; fills the descriptor but for its device pointers
int png_describe(const hipts_png_header* hd, int64_t slot_bytes, PngImage* im);

// one workgroup per image; all work on `s`, nothing is synchronised
int png_launch(const PngImage* ims, int n, hipStream_t s);

}  // namespace hipts
