// jpegenc.hip -- device half of the hybrid JPEG encode (hipts_jpeg_encode_batch_u8): the mirror image of jpeg.hip, for thumbnails and
// contact sheets (hiptagsearch/thumbs.py).  The reference shows what a query found by opening every full-size original per page view
// (webui.py display_images); this project wrote no picture at all.  The bar is the file PIL.Image.save(..., "JPEG", quality=Q) writes --
// libjpeg-turbo with its defaults: three components, 4:2:0, baseline tables -- byte for byte.  What is per pixel and per block runs
// here, all of it libjpeg's integer arithmetic (tests/jpegenc_ref.py is the numpy statement, pinned against Pillow's own files):
//   tables    jcparam.c jpeg_set_quality: s = 5000 / Q below 50, else 200 - 2 Q; clip((std s + 50) / 100, 1, 255) of the Annex K tables
//   colour    jccolor.c rgb_ycc_convert, 16 fractional bits
//   edges     jcprepct.c / jcsample.c: the last column is replicated to the right up to whole MCUs at full resolution; Y's last row
//             downwards; chroma gets one replicated row when the height is odd, is downsampled, and the DOWNSAMPLED rows are replicated
//             down to whole blocks
//   chroma    jcsample.c h2v2_downsample: (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2, ... along the output columns
//   DCT       jfdctint.c jpeg_fdct_islow on samples - 128: rows, then columns (CONST_BITS 13, PASS1_BITS 2)
//   quantise  jcdctmgr.c: d = 8 q, t = |c| + d / 2, sign(c) (t / d) -- a true integer division, nothing to prove about a reciprocal
//   filler    jccoefct.c: a luminance block wholly beyond ceil(w / 8) columns or ceil(h / 8) rows has no AC and the DC of the block before
//             it in the MCU's coding order (top-left, top-right, bottom-left, bottom-right)
// The output is the slot of jpeg_slot.h, header included -- what hipts_jpeg_entropy_decode writes for a 4:2:0 file -- so the host coder
// (jpeg_host.c hipts_jpeg_entropy_encode) and the decoder (hipts_jpeg_decode_rgb) read it as it stands.
//
//   jpeg_encode_kernel   a workgroup takes ENC_G MCUs of one MCU row: 16 rows x 64 pixels.  The RGB bytes come in as whole dwords,
//                        consecutive lanes on consecutive dwords of a row (byte loads where the row is not dword aligned, or crosses the
//                        right edge), and go to LDS; Y, Cb and Cr go to LDS as 16-bit; eight lanes per 8 x 8 block run the row pass
//                        (chroma is downsampled as it is read), hand over through LDS, run the column pass and quantise; the blocks
//                        leave as 16-byte stores, a row of a block per lane.
// Algorithmic traffic per pixel: 3 bytes read, 3 bytes of coefficients written.
#include <algorithm>

#include "common.h"
#include "jpeg_slot.h"

using namespace hipts;

namespace {

constexpr int ENC_G = 4;                      // MCUs per workgroup
constexpr int ENC_W = 16 * ENC_G;             // pixels per workgroup row
constexpr int ENC_ROW_DWORDS = ENC_W * 3 / 4;
constexpr int ENC_THREADS = 256;
constexpr int ENC_BLOCKS = 6 * ENC_G;         // 2 x 2 G luminance blocks, then G of Cb, then G of Cr
constexpr int ENC_MIN = 16, ENC_MAX = 8192;
static_assert(ENC_BLOCKS * 8 <= ENC_THREADS && 16 * ENC_W == 4 * ENC_THREADS, "eight lanes per block, four pixels per thread");

// T.81 Annex K.1 and K.2, natural order
__constant__ uint8_t STD_QUANT[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

struct EncParams {
    const uint8_t* images;      // device: uint8 [n][height][width][3]
    uint8_t* slots;             // device, 16-byte aligned
    int64_t slot_stride;        // a multiple of 16
    int width, height;
    int scale;                  // jpeg_quality_scaling(quality)
    int dword_rows;             // every row of every image starts on a dword
};

// one pass of jfdctint.c over d[0..7]
template <bool FIRST>
__device__ __forceinline__ void fdct_1d(int (&d)[8]) {
    constexpr int F0_298631336 = 2446, F0_390180644 = 3196, F0_541196100 = 4433, F0_765366865 = 6270, F0_899976223 = 7373, F1_175875602 = 9633,
                  F1_501321110 = 12299, F1_847759065 = 15137, F1_961570560 = 16069, F2_053119869 = 16819, F2_562915447 = 20995,
                  F3_072711026 = 25172;
    constexpr int N = FIRST ? 11 : 15, R = 1 << (N - 1);      // CONST_BITS -+ PASS1_BITS
    int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    if (FIRST) {
        d[0] = (tmp10 + tmp11) << 2;
        d[4] = (tmp10 - tmp11) << 2;
    } else {
        d[0] = (tmp10 + tmp11 + 2) >> 2;
        d[4] = (tmp10 - tmp11 + 2) >> 2;
    }
    int z1 = (tmp12 + tmp13) * F0_541196100;
    d[2] = (z1 + tmp13 * F0_765366865 + R) >> N;
    d[6] = (z1 + tmp12 * (-F1_847759065) + R) >> N;
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * F1_175875602;
    tmp4 *= F0_298631336;
    tmp5 *= F2_053119869;
    tmp6 *= F3_072711026;
    tmp7 *= F1_501321110;
    z1 *= -F0_899976223;
    z2 *= -F2_562915447;
    z3 = z3 * (-F1_961570560) + z5;
    z4 = z4 * (-F0_390180644) + z5;
    d[7] = (tmp4 + z1 + z3 + R) >> N;
    d[5] = (tmp5 + z2 + z4 + R) >> N;
    d[3] = (tmp6 + z2 + z3 + R) >> N;
    d[1] = (tmp7 + z1 + z4 + R) >> N;
}

__global__ __launch_bounds__(ENC_THREADS) void jpeg_encode_kernel(const EncParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[16][ENC_W * 3];
    __shared__ int16_t ycc[3][16][ENC_W];
    __shared__ int ws[ENC_BLOCKS][72];                                       // a block's rows padded to nine words
    __shared__ __attribute__((aligned(16))) int16_t qs[ENC_BLOCKS][64];
    __shared__ uint16_t qt[2][64];
    const int t = threadIdx.x;
    const int W = P.width, H = P.height;
    const int mcux = (W + 15) >> 4, mcuy = (H + 15) >> 4;
    const int gx = blockIdx.x, my = blockIdx.y;
    const int x0 = gx * ENC_W, y0 = my * 16;
    const uint8_t* __restrict__ src = P.images + (int64_t)blockIdx.z * H * W * 3;
    uint8_t* __restrict__ slot = P.slots + (int64_t)blockIdx.z * P.slot_stride;
    const int chroma_blocks = mcux * mcuy;                                   // per chroma component; luminance has four times as many

    if (t < 128) {
        const int q = ((int)STD_QUANT[t >> 6][t & 63] * P.scale + 50) / 100;
        qt[t >> 6][t & 63] = (uint16_t)(q < 1 ? 1 : q > 255 ? 255 : q);
    }
    // ---- the RGB bytes of 16 rows x 64 pixels; rows past the last one repeat it
    for (int i = t; i < 16 * ENC_ROW_DWORDS; i += ENC_THREADS) {
        const int r = i / ENC_ROW_DWORDS, dw = i - r * ENC_ROW_DWORDS;
        const uint8_t* __restrict__ rowp = src + (int64_t)min(y0 + r, H - 1) * W * 3;
        const int b0 = x0 * 3 + dw * 4;
        uint32_t v = 0;
        if (P.dword_rows && b0 + 4 <= W * 3) {
            v = *reinterpret_cast<const uint32_t*>(rowp + b0);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int b = b0 + q, px = b / 3, ch = b - px * 3;
                v |= (uint32_t)rowp[min(px, W - 1) * 3 + ch] << (8 * q);     // pixels past the last column repeat it
            }
        }
        *reinterpret_cast<uint32_t*>(&raw[r][dw * 4]) = v;
    }
    __syncthreads();
    // the slot's header, by the image's first workgroup: a dword per thread (jpeg_slot.h; the quantisers are ready in qt)
    if (gx == 0 && my == 0) {
        uint32_t v = 0;
        if (t < 8) {
            const int head[8] = {HIPTS_JPEG_MAGIC, 1, W, H, 3, 2, 2, 0};
            v = (uint32_t)head[t];
        } else if (t < 32) {
            const int c = (t - 8) >> 3, f = c == 0 ? 2 : 1;
            const int comp[8] = {f, f, mcux * f, mcuy * f, c == 0 ? W : (W + 1) >> 1, c == 0 ? H : (H + 1) >> 1,
                                 c == 0 ? 0 : chroma_blocks * 64 * (3 + c), 0};
            v = (uint32_t)comp[t & 7];
        } else if (t < 128) {
            const int c = (t - 32) >> 5, k = ((t - 32) & 31) * 2;
            v = (uint32_t)qt[c > 0][k] | ((uint32_t)qt[c > 0][k + 1] << 16);
        } else if (t == 128) {
            v = (uint32_t)(HIPTS_JPEG_HEADER_BYTES + chroma_blocks * 6 * 128);   // total_bytes: below 2^31 for every size the call takes
        }
        reinterpret_cast<uint32_t*>(slot)[t] = v;
    }
    // ---- colour: four pixels per thread
    {
        const int r = t >> 4, c0 = (t & 15) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int R = raw[r][(c0 + k) * 3], G = raw[r][(c0 + k) * 3 + 1], B = raw[r][(c0 + k) * 3 + 2];
            ycc[0][r][c0 + k] = (int16_t)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
            ycc[1][r][c0 + k] = (int16_t)((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16);
            ycc[2][r][c0 + k] = (int16_t)((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16);
        }
    }
    __syncthreads();
    // ---- eight lanes per block: lane l8 takes row l8, then column l8
    const int blk = t >> 3, l8 = t & 7;
    const bool dct = blk < ENC_BLOCKS;
    const int comp = blk < 4 * ENC_G ? 0 : 1 + (blk - 4 * ENC_G) / ENC_G;
    const int br = comp == 0 ? blk / (2 * ENC_G) : 0;                         // block row and column inside the workgroup's strip
    const int bc = comp == 0 ? blk % (2 * ENC_G) : (blk - 4 * ENC_G) % ENC_G;
    int d[8];
    if (dct) {
        if (comp == 0) {
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = (int)ycc[0][br * 8 + l8][bc * 8 + k] - 128;
        } else {
            // downsampled rows past the last real one, (H + 1) / 2 - 1, repeat IT (not the full-resolution row): it lies in this MCU row
            const int lr = 2 * (min(my * 8 + l8, ((H + 1) >> 1) - 1) - my * 8);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int cx = (bc * 8 + k) * 2;
                const int s = (int)ycc[comp][lr][cx] + ycc[comp][lr][cx + 1] + ycc[comp][lr + 1][cx] + ycc[comp][lr + 1][cx + 1] + 1 + (k & 1);
                d[k] = (s >> 2) - 128;
            }
        }
        fdct_1d<true>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) ws[blk][l8 * 9 + k] = d[k];
    }
    __syncthreads();
    if (dct) {
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = ws[blk][k * 9 + l8];
        fdct_1d<false>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const unsigned div = 8u * qt[comp > 0][k * 8 + l8];
            const unsigned a = (unsigned)(d[k] < 0 ? -d[k] : d[k]) + (div >> 1);
            const int q = (int)(a / div);                                   // (below div: 0, as jcdctmgr.c's test says)
            qs[blk][k * 8 + l8] = (int16_t)(d[k] < 0 ? -q : q);
        }
    }
    __syncthreads();
    if (!dct) return;
    // ---- lane l8 stores row l8 of its block
    int16_t* __restrict__ coef = reinterpret_cast<int16_t*>(slot + HIPTS_JPEG_HEADER_BYTES);
    uint4 v = *reinterpret_cast<const uint4*>(&qs[blk][l8 * 8]);
    if (comp == 0) {
        const int by = my * 2 + br, bx = gx * 2 * ENC_G + bc;
        if (bx >= 2 * mcux) return;                                          // an MCU past the last one of the row
        const int real_w = (W + 7) >> 3, real_h = (H + 7) >> 3;
        int sr = br, sc = bc;                                                // the block whose DC a filler block repeats
        while (my * 2 + sr >= real_h || gx * 2 * ENC_G + sc >= real_w) {     // (ends at the MCU's top-left block, which holds real pixels)
            if (sc & 1) {
                sc -= 1;
            } else {
                sr -= 1;
                sc += 1;
            }
        }
        if (sr != br || sc != bc) v = make_uint4(l8 == 0 ? (uint32_t)(uint16_t)qs[sr * 2 * ENC_G + sc][0] : 0u, 0u, 0u, 0u);
        *reinterpret_cast<uint4*>(coef + ((int64_t)by * (2 * mcux) + bx) * 64 + l8 * 8) = v;
    } else {
        const int bx = gx * ENC_G + bc;
        if (bx >= mcux) return;
        *reinterpret_cast<uint4*>(coef + (int64_t)chroma_blocks * 64 * (3 + comp) + ((int64_t)my * mcux + bx) * 64 + l8 * 8) = v;
    }
}

// Handle-less entry point: the staging buffers are kept per device and shared by every caller, ordered by an event (as imghash.hip's)
struct EncState {
    std::mutex mu;
    DevBuf in[64], out[64];
    hipEvent_t last[64] = {};
};
EncState& state() {
    static EncState* s = new EncState;          // never destroyed: the runtime may be gone before static destructors run
    return *s;
}

}  // namespace

extern "C" int hipts_jpeg_encode_batch_u8(const uint8_t* images, int images_memspace, int n, int height, int width, int quality,
                                          uint8_t* slots_out, int out_memspace, int64_t slot_stride, int device, void* stream) {
    HIPTS_REQUIRE(images && slots_out, "hipts_jpeg_encode_batch_u8: null argument");
    HIPTS_REQUIRE(n >= 1 && n <= 65535, "hipts_jpeg_encode_batch_u8: batch must be in [1, 65535], got %d", n);
    HIPTS_REQUIRE(height >= ENC_MIN && height <= ENC_MAX && width >= ENC_MIN && width <= ENC_MAX,
                  "hipts_jpeg_encode_batch_u8: size must be in [%d, %d] either way, got %d x %d", ENC_MIN, ENC_MAX, height, width);
    HIPTS_REQUIRE(quality >= 1 && quality <= 100, "hipts_jpeg_encode_batch_u8: quality must be in [1, 100], got %d", quality);
    HIPTS_REQUIRE(slot_stride >= hipts_jpeg_slot_bytes(width, height), "hipts_jpeg_encode_batch_u8: slot_stride %lld, a %d x %d image needs %lld",
                  (long long)slot_stride, height, width, (long long)hipts_jpeg_slot_bytes(width, height));
    HIPTS_REQUIRE(device >= 0 && device < 64, "hipts_jpeg_encode_batch_u8: device index");
    HIPTS_TRY(use_device(device));
    hipStream_t s = (hipStream_t)stream;
    const int mcux = (width + 15) / 16, mcuy = (height + 15) / 16;
    const size_t image_bytes = (size_t)height * width * 3;
    const size_t total_bytes = HIPTS_JPEG_HEADER_BYTES + (size_t)mcux * mcuy * 6 * 128;          // (a multiple of 16)
    const bool host_in = images_memspace != HIPTS_DEVICE, host_out = out_memspace != HIPTS_DEVICE;
    // the kernel stores 16-byte vectors: a destination that is not aligned for them (or is host memory) gets its slots by copies
    const bool direct = !host_out && (reinterpret_cast<uintptr_t>(slots_out) & 15) == 0 && (slot_stride & 15) == 0;
    EncState& st = state();
    std::lock_guard<std::mutex> lock(st.mu);
    if (st.last[device]) HIPTS_HIP(hipStreamWaitEvent(s, st.last[device], 0));
    else HIPTS_HIP(hipEventCreateWithFlags(&st.last[device], hipEventDisableTiming));
    EncParams P{};
    P.images = images;
    if (host_in) {
        HIPTS_TRY(st.in[device].reserve((size_t)n * image_bytes));
        HIPTS_HIP(hipMemcpyAsync(st.in[device].p, images, (size_t)n * image_bytes, hipMemcpyHostToDevice, s));
        P.images = st.in[device].as<uint8_t>();
    }
    P.slots = slots_out;
    P.slot_stride = slot_stride;
    if (!direct) {
        HIPTS_TRY(st.out[device].reserve((size_t)n * total_bytes));
        P.slots = st.out[device].as<uint8_t>();
        P.slot_stride = (int64_t)total_bytes;
    }
    P.width = width;
    P.height = height;
    P.scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    P.dword_rows = (reinterpret_cast<uintptr_t>(P.images) & 3) == 0 && width % 4 == 0;
    jpeg_encode_kernel<<<dim3((unsigned)((mcux + ENC_G - 1) / ENC_G), (unsigned)mcuy, (unsigned)n), ENC_THREADS, 0, s>>>(P);
    HIPTS_LAUNCH_CHECK();
    if (!direct)
        for (int i = 0; i < n; ++i)
            HIPTS_HIP(hipMemcpyAsync(slots_out + (size_t)i * slot_stride, P.slots + (size_t)i * total_bytes, total_bytes,
                                     host_out ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
    HIPTS_HIP(hipEventRecord(st.last[device], s));
    return HIPTS_OK;
}
