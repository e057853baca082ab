// The hand-over between the host half and the device half of the hybrid PNG decode (jpeg_slot.h is its JPEG twin).
//
//   host   (hiptagsearch/png_host.py, pure Python: struct + zlib + numpy, in the decode worker PROCESSES) checks the chunk stream of a
//          completely regular 8-bit non-interlaced grey / grey + alpha / RGB / RGBA file and inflates its IDAT stream -- the part of a PNG
//          decoder that is a serial bit stream -- straight into the ring slot;
//   device (png.hip, in libhip_tagsearch.so) undoes the scanline filters (PNG specification, section 9), replicates grey to three channels
//          and composites alpha over white as Predictor.prepare_image does (reference tagging.py:103-106), then the tagger's pad + resize.
//
// A slot is a ring-buffer slot of hiptagsearch/pipeline.py: this header, then height rows of (1 filter byte + width * channels bytes),
// exactly what zlib returned.  What the reference does at this point is PIL's Image.open(...).load() plus the white composite: the
// device half reproduces those bytes exactly (tests/test_gpu_png.py compares with Pillow).
#pragma once
#include <stdint.h>

#define HIPTS_PNG_MAGIC 0x20474e50        /* "PNG " */
#define HIPTS_PNG_HEADER_BYTES 1024       /* scanlines start here */
#define HIPTS_PNG_MAX_WIDTH 8192          /* two LDS row buffers of 4 * width bytes (png.hip); the host half refuses wider files */

typedef struct {
    int32_t magic;                /* HIPTS_PNG_MAGIC */
    int32_t kind;                 /* 2: filtered scanlines follow */
    int32_t width, height;        /* image size in pixels */
    int32_t channels;             /* 1 grey, 2 grey + alpha, 3 RGB, 4 RGBA; one byte each */
    int32_t reserved[3];
    int64_t total_bytes;          /* header + height * (1 + width * channels) */
} hipts_png_header;
