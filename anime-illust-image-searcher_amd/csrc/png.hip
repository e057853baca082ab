// png.hip -- device half of the hybrid PNG decode (png_slot.h describes the split).  The reference decodes with PIL's Image.open and
// composites alpha over white (tagging.py:100-120, gen_cfeatures.py:285-295); the serial part -- the chunk stream and inflate -- stays on
// the host (hiptagsearch/png_host.py, in the decode worker processes); what is per scanline and per pixel runs here:
//   png_unfilter_kernel   reconstruction of the five PNG filter types (Recon(x) = Filt(x) + pred(a, b, c) mod 256; a = the pixel to the
//                         left, b = above, c = above left, zeros outside the image), grey -> three channels, alpha over white with
//                         Pillow's rounding -> uint8 [h][w][3]
// then resize.hip's pad + Pillow-exact resize.
//
// One image is one workgroup, and every dependency is resolved inside it by __syncthreads() and lane exchange: no flag in global memory,
// no spin, no wait for another workgroup.  No address depends on scanline content.
//
//   band    64 consecutive rows, one lane each, of one wave.  Lane l runs GROUPS of four pixels skewed by one group per lane: in group
//           step G it reconstructs pixels 4 (G - l) .. 4 (G - l) + 3 of its row.  `b` of those four pixels is what lane l - 1 produced
//           in step G - 1 (four __shfl_up), `c` is the previous `b`, `a` the lane's own last result.  A pixel is packed in 32 bits.
//   hand-on the last row of band k is `b` of the first row of band k + 1: lane 63 leaves it in an LDS row buffer (two buffers of
//           4 * width bytes, by band parity), lane 0 of the next band reads it.
//   chunk   the bands are dealt to the four waves of the workgroup (band k on wave k % 4) and a band advances in chunks of 64 group
//           steps, one barrier per round.  Chunk t of band k + 1 reads pixels up to 4 (64 t + 63) + 3 of the row above, which band k
//           has written once its chunk t + 1 is over (its lane 63 is 63 groups behind), so band k + 1 follows two chunks behind band k.
//           The schedule depends on the image's size only: every thread steps the same four counters in registers.
#include <algorithm>
#include <cstddef>
#include <mutex>
#include <vector>

#include "common.h"
#include "png.h"

#include "../../include/hip_tagsearch.h"

namespace hipts {
namespace {

constexpr int PNG_WAVES = 4;
constexpr int BAND = 64;          // rows per band = lanes per wave
constexpr int CHUNK = 64;         // group steps per round

struct PngBatch {
    PngImage im[PNG_CHUNK];
};

// Pillow's alpha blend over white (Paste.c / ImagingPaste with a mask, MULDIV255): exact for all 65 536 (alpha, v)
__device__ __forceinline__ unsigned over_white(unsigned v, unsigned alpha) {
    const unsigned t = 255u * (255u - alpha) + v * alpha + 128u;
    return ((t >> 8) + t) >> 8;
}

template <int BPP>
__device__ __forceinline__ unsigned recon(unsigned f, unsigned a, unsigned b, unsigned c, int ft) {
    unsigned r = 0;
#pragma unroll
    for (int ch = 0; ch < BPP; ++ch) {
        const int fa = (f >> (8 * ch)) & 255, aa = (a >> (8 * ch)) & 255, bb = (b >> (8 * ch)) & 255, cc = (c >> (8 * ch)) & 255;
        const int pa = abs(bb - cc), pb = abs(aa - cc), pc = abs(aa + bb - 2 * cc);
        const int paeth = (pa <= pb && pa <= pc) ? aa : (pb <= pc ? bb : cc);      // the order of the ties is the specification's
        const int pred = ft == 1 ? aa : ft == 2 ? bb : ft == 3 ? ((aa + bb) >> 1) : ft == 4 ? paeth : 0;
        r |= (unsigned)((fa + pred) & 255) << (8 * ch);
    }
    return r;
}

// the 4 * BPP bytes of pixel group g of a row as BPP words: whole aligned words, shifted together (the row starts at any byte)
template <int BPP>
__device__ __forceinline__ void load_group(const uint8_t* __restrict__ row, int g, unsigned (&d)[BPP]) {
    const uint8_t* p = row + (size_t)g * (4 * BPP);
    const unsigned sh = ((unsigned)(uintptr_t)p & 3u) * 8u;
    const unsigned* q = reinterpret_cast<const unsigned*>((uintptr_t)p & ~(uintptr_t)3);
    unsigned raw[BPP + 1];
#pragma unroll
    for (int i = 0; i <= BPP; ++i) raw[i] = q[i];
#pragma unroll
    for (int i = 0; i < BPP; ++i) d[i] = (unsigned)((((unsigned long long)raw[i + 1] << 32) | raw[i]) >> sh);
}

template <int BPP>
__device__ __forceinline__ unsigned pixel_of(const unsigned (&d)[BPP], int j) {
    unsigned p = 0;
#pragma unroll
    for (int ch = 0; ch < BPP; ++ch) {
        const int byte = j * BPP + ch;
        p |= ((d[byte >> 2] >> (8 * (byte & 3))) & 255u) << (8 * ch);
    }
    return p;
}

template <int BPP>
__device__ __forceinline__ void rgb_of(unsigned p, unsigned (&o)[3]) {
    if (BPP == 1) {
        o[0] = o[1] = o[2] = p & 255u;
    } else if (BPP == 2) {
        o[0] = o[1] = o[2] = over_white(p & 255u, (p >> 8) & 255u);
    } else if (BPP == 3) {
        o[0] = p & 255u;
        o[1] = (p >> 8) & 255u;
        o[2] = (p >> 16) & 255u;
    } else {
        const unsigned al = p >> 24;
        o[0] = over_white(p & 255u, al);
        o[1] = over_white((p >> 8) & 255u, al);
        o[2] = over_white((p >> 16) & 255u, al);
    }
}

template <int BPP>
__device__ void png_unfilter_image(const PngImage& im, unsigned* __restrict__ rows) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int w = im.width, h = im.height;
    const int ng = (w + 3) >> 2;                          // pixel groups per row
    const int wp = ng * 4;                                // words per LDS row buffer
    const int steps = ng + BAND - 1;                      // group steps of a band (the skew)
    const int nt = (steps + CHUNK - 1) / CHUNK;           // chunks per band
    const int nb = (h + BAND - 1) / BAND;
    const size_t stride = (size_t)w * BPP + 1;
    const bool words_out = (w & 3) == 0 && ((uintptr_t)im.rgb & 3) == 0;      // every row of the output starts on a word

    int cnt[PNG_WAVES], total[PNG_WAVES];
#pragma unroll
    for (int u = 0; u < PNG_WAVES; ++u) {
        cnt[u] = 0;
        total[u] = nb > u ? ((nb - u + PNG_WAVES - 1) / PNG_WAVES) * nt : 0;
    }
    // the band this wave is in: carried from chunk to chunk
    unsigned res[4] = {0, 0, 0, 0};                       // the lane's last four pixels
    unsigned cprev = 0;                                   // b of the pixel left of the next group
    int ft = 0, y = 0;
    const uint8_t* row = im.src;

    for (;;) {
        bool all_done = true, go_mine = false;
        int my_item = 0;
        bool go[PNG_WAVES];
#pragma unroll
        for (int u = 0; u < PNG_WAVES; ++u) {
            go[u] = false;
            if (cnt[u] < total[u]) {
                all_done = false;
                const int m = cnt[u] / nt, t = cnt[u] - m * nt;
                if (m == 0 && u == 0) {
                    go[u] = true;                          // the first band has nothing above it
                } else {
                    const int pu = u ? u - 1 : PNG_WAVES - 1, pm = u ? m : m - 1;
                    go[u] = cnt[pu] >= pm * nt + min(t + 1, nt - 1) + 1;
                }
            }
            if (u == wave) {
                go_mine = go[u];
                my_item = cnt[u];
            }
        }
        if (all_done) break;
        if (go_mine) {
            const int m = my_item / nt, t = my_item - m * nt;
            const int k = m * PNG_WAVES + wave;
            if (t == 0) {
                y = k * BAND + lane;
                const int yc = min(y, h - 1);
                const uint8_t* line = im.src + (size_t)yc * stride;
                ft = line[0];
                if (ft > 4) ft = 0;                        // (the host half has refused such a file)
                row = line + 1;
            }
            const unsigned* above = rows + ((k - 1) & 1) * wp;
            unsigned* mine = rows + (k & 1) * wp;
            const int g_end = min(t * CHUNK + CHUNK, steps);
            unsigned d[BPP], nd[BPP];
            load_group<BPP>(row, min(max(t * CHUNK - lane, 0), ng - 1), d);
            for (int G = t * CHUNK; G < g_end; ++G) {
                const int gl = G - lane;
                load_group<BPP>(row, min(max(gl + 1, 0), ng - 1), nd);       // the next group's bytes, under this group's arithmetic
                unsigned bv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) bv[j] = __shfl_up(res[j], 1);
                if (lane == 0) {
                    if (k > 0) {
                        const uint4 v = *reinterpret_cast<const uint4*>(above + 4 * min(G, ng - 1));
                        bv[0] = v.x;
                        bv[1] = v.y;
                        bv[2] = v.z;
                        bv[3] = v.w;
                    } else {
                        bv[0] = bv[1] = bv[2] = bv[3] = 0;
                    }
                }
                unsigned a = res[3];
                if (gl <= 0) a = cprev = 0;                // left of the row
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    a = recon<BPP>(pixel_of<BPP>(d, j), a, bv[j], j ? bv[j - 1] : cprev, ft);
                    res[j] = a;
                }
                cprev = bv[3];
                const bool in_row = gl >= 0 && gl < ng;
                if (lane == BAND - 1 && in_row) *reinterpret_cast<uint4*>(mine + 4 * gl) = make_uint4(res[0], res[1], res[2], res[3]);
                if (in_row && y < h) {
                    unsigned o[4][3];
#pragma unroll
                    for (int j = 0; j < 4; ++j) rgb_of<BPP>(res[j], o[j]);
                    uint8_t* op = im.rgb + ((size_t)y * w + 4 * gl) * 3;
                    if (words_out) {
                        unsigned* ow = reinterpret_cast<unsigned*>(op);
                        ow[0] = o[0][0] | (o[0][1] << 8) | (o[0][2] << 16) | (o[1][0] << 24);
                        ow[1] = o[1][1] | (o[1][2] << 8) | (o[2][0] << 16) | (o[2][1] << 24);
                        ow[2] = o[2][2] | (o[3][0] << 8) | (o[3][1] << 16) | (o[3][2] << 24);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            if (4 * gl + j < w) {
                                op[3 * j] = (uint8_t)o[j][0];
                                op[3 * j + 1] = (uint8_t)o[j][1];
                                op[3 * j + 2] = (uint8_t)o[j][2];
                            }
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < BPP; ++i) d[i] = nd[i];
            }
        }
#pragma unroll
        for (int u = 0; u < PNG_WAVES; ++u) cnt[u] += go[u] ? 1 : 0;
        __syncthreads();
    }
}

__global__ __launch_bounds__(PNG_WAVES * 64) void png_unfilter_kernel(const PngBatch b) {
    extern __shared__ __align__(16) unsigned png_rows[];
    const PngImage& im = b.im[blockIdx.x];
    switch (im.channels) {          // uniform per workgroup
        case 1: png_unfilter_image<1>(im, png_rows); break;
        case 2: png_unfilter_image<2>(im, png_rows); break;
        case 3: png_unfilter_image<3>(im, png_rows); break;
        default: png_unfilter_image<4>(im, png_rows); break;
    }
}

struct PngState {
    std::mutex mu;
    DevBuf stage[64], rgb[64];      // per device: the slot, the decoded image (host output)
    hipEvent_t last[64] = {};
};
PngState& pstate() {
    static PngState* s = new PngState;      // never destroyed: see scratch_buf() in query.hip
    return *s;
}

}  // namespace

int png_describe(const hipts_png_header* hd, int64_t slot_bytes, PngImage* im) {
    HIPTS_REQUIRE(hd->magic == HIPTS_PNG_MAGIC && hd->kind == 2, "png: the slot does not hold scanlines");
    HIPTS_REQUIRE(hd->channels >= 1 && hd->channels <= 4 && hd->width >= 1 && hd->width <= HIPTS_PNG_MAX_WIDTH && hd->height >= 1,
                  "png: unsupported geometry in the slot header");
    const int64_t want = HIPTS_PNG_HEADER_BYTES + (int64_t)hd->height * (1 + (int64_t)hd->width * hd->channels);
    HIPTS_REQUIRE(hd->total_bytes == want && hd->total_bytes <= slot_bytes, "png: slot of %lld bytes, header says %lld, %d x %d x %d needs %lld",
                  (long long)slot_bytes, (long long)hd->total_bytes, hd->height, hd->width, hd->channels, (long long)want);
    im->src = nullptr;
    im->rgb = nullptr;
    im->width = hd->width;
    im->height = hd->height;
    im->channels = hd->channels;
    im->pad = 0;
    return HIPTS_OK;
}

int png_launch(const PngImage* ims, int n, hipStream_t s) {
    for (int first = 0; first < n; first += PNG_CHUNK) {
        const int nb = std::min(PNG_CHUNK, n - first);
        PngBatch b{};
        int max_w = 1;
        for (int i = 0; i < nb; ++i) {
            b.im[i] = ims[first + i];
            max_w = std::max(max_w, b.im[i].width);
        }
        const size_t lds = (size_t)2 * ((max_w + 3) / 4 * 4) * sizeof(unsigned);      // <= 64 KB: HIPTS_PNG_MAX_WIDTH
        png_unfilter_kernel<<<nb, PNG_WAVES * 64, lds, s>>>(b);
        HIPTS_LAUNCH_CHECK();
    }
    return HIPTS_OK;
}

}  // namespace hipts

using namespace hipts;

extern "C" int hipts_png_decode_rgb(const void* slot, int64_t slot_bytes, uint8_t* rgb_out, int out_memspace, int64_t out_capacity, int device,
                                    void* stream) {
    HIPTS_REQUIRE(slot && rgb_out && slot_bytes >= HIPTS_PNG_HEADER_BYTES, "hipts_png_decode_rgb: bad arguments");
    HIPTS_REQUIRE(device >= 0 && device < 64, "hipts_png_decode_rgb: device index");
    const hipts_png_header* hd = static_cast<const hipts_png_header*>(slot);
    PngImage im{};
    HIPTS_TRY(png_describe(hd, slot_bytes, &im));
    const size_t rgb_bytes = (size_t)hd->width * hd->height * 3;
    HIPTS_REQUIRE((int64_t)rgb_bytes <= out_capacity, "hipts_png_decode_rgb: %d x %d needs %zu bytes, the output holds %lld", hd->height, hd->width,
                  rgb_bytes, (long long)out_capacity);
    HIPTS_TRY(use_device(device));
    hipStream_t s = (hipStream_t)stream;
    PngState& st = pstate();
    std::lock_guard<std::mutex> lock(st.mu);
    if (st.last[device]) HIPTS_HIP(hipStreamWaitEvent(s, st.last[device], 0));
    else HIPTS_HIP(hipEventCreateWithFlags(&st.last[device], hipEventDisableTiming));
    HIPTS_TRY(st.stage[device].reserve((size_t)hd->total_bytes + PNG_STAGE_PAD));
    uint8_t* out = rgb_out;
    if (out_memspace != HIPTS_DEVICE) {
        HIPTS_TRY(st.rgb[device].reserve(rgb_bytes));
        out = st.rgb[device].as<uint8_t>();
    }
    HIPTS_HIP(hipMemcpyAsync(st.stage[device].p, slot, (size_t)hd->total_bytes, hipMemcpyHostToDevice, s));
    im.src = st.stage[device].as<uint8_t>() + HIPTS_PNG_HEADER_BYTES;
    im.rgb = out;
    HIPTS_TRY(png_launch(&im, 1, s));
    if (out_memspace != HIPTS_DEVICE) HIPTS_HIP(hipMemcpyAsync(rgb_out, out, rgb_bytes, hipMemcpyDeviceToHost, s));
    HIPTS_HIP(hipEventRecord(st.last[device], s));
    HIPTS_HIP(hipStreamSynchronize(s));       // the caller's slot and (host) output are its own again
    return HIPTS_OK;
}
