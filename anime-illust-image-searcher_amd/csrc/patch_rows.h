// patch_rows.h -- the "one thread per (token, ky) gathers a patch row" kernels in front of the five forwards' first GEMM (vit.hip, eva.hip
// and ccip.hip directly; convnext.hip and swinv2.hip through convnet.h).  Device code only.  Everything lives in an anonymous namespace,
// so each including object gets its own copy under the same symbol names.
//
// patch_gather_kernel writes the patch matrix as hi | lo halves of the normalised pixel (split_hilo, against [W | W]): what differs
// between its uses is a compile-time policy -- where a pixel comes from and how it is normalised, and the window's geometry.  The
// LDS-tiled throughput kernels of the uint8 entries (vit.hip: patchify_u8_p16_kernel, ccip.hip: stem_im2col_u8_kernel) are not part of it.
#pragma once
#include "vit_internal.h"
#include "row_ln.h"

namespace {

using namespace hipts;

// ---- pixels: operator()(image b, memory channel c (RGB), iy, ix, side S) = the normalised value.  The BGR order of the taggers lives
// in the weight permutation (model_host.h: stem_weight_hilo), so a float32 input that is already BGR is read at plane 2 - c.
struct PixelU8Affine {                  // uint8 NHWC; ToTensor (/255) and Normalize ((x - .5) / .5) in float32 like the reference
    const uint8_t* img;
    __device__ float operator()(int64_t b, int c, int iy, int ix, int S) const {
        const float u = (float)img[((b * S + iy) * S + ix) * 3 + c];
        return (u / 255.0f - 0.5f) / 0.5f;
    }
};

struct PixelU8Table {                   // uint8 NHWC through lut[c][u] in global memory (model_host.h: norm_lut)
    const uint8_t* img;
    const float* lut;
    __device__ float operator()(int64_t b, int c, int iy, int ix, int S) const { return lut[c * 256 + img[((b * S + iy) * S + ix) * 3 + c]]; }
};

template <bool FLIP>
struct PixelF32Planes {                 // float32 [B][3][S][S], already normalised; FLIP: plane 2 - c holds memory channel c
    const float* x;
    __device__ float operator()(int64_t b, int c, int iy, int ix, int S) const {
        return x[((b * 3 + (FLIP ? 2 - c : c)) * S + iy) * (int64_t)S + ix];
    }
};

// ---- windows: SIZE x SIZE taps (0: size() at run time), output (oy, ox) starts at input origin(oy), origin(ox); a row of the patch
// matrix is 2 half() wide, tap (ky, kx) of channel c at column (ky * size() + kx) * 3 + c of each half.  BORDER: taps outside the
// image are zero.  ZERO_PAD: the ky == 0 thread zeroes the pad columns 3 size()^2 .. half() of both halves; the others leave them to
// the allocation (eva.hip and ccip.hip zero a0 once).
struct WindowPatch {                    // P x P stride P
    static constexpr int SIZE = 0;
    static constexpr bool BORDER = false, ZERO_PAD = false;
    int P, KH;
    __device__ int size() const { return P; }
    __device__ int half() const { return KH; }
    __device__ int origin(int o) const { return o * P; }
};

struct Window4x4 {                      // 4 x 4 stride 4: 48 taps padded to 64
    static constexpr int SIZE = 4;
    static constexpr bool BORDER = false, ZERO_PAD = true;
    __device__ static constexpr int size() { return 4; }
    __device__ static constexpr int half() { return 64; }
    __device__ static constexpr int origin(int o) { return 4 * o; }
};

struct Window7x7 {                      // 7 x 7 stride 4 pad 2: 147 taps padded to 160 (Conv2d padding pads the NORMALISED input)
    static constexpr int SIZE = 7;
    static constexpr bool BORDER = true, ZERO_PAD = false;
    __device__ static constexpr int size() { return 7; }
    __device__ static constexpr int half() { return 160; }
    __device__ static constexpr int origin(int o) { return 4 * o - 2; }
};

// a0[m][...] for the total = images * G * G * size() (token m, ky) pairs of G x G tokens per image.  One thread per pair: 3 size() values.
template <bool F16, class Pixel, class Window>
__global__ __launch_bounds__(256) void patch_gather_kernel(Pixel pixel, Window win, bf16_t* __restrict__ a0, int64_t total, int S, int G) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ks = win.size(), KH = win.half();
    const int ky = (int)(idx % ks);
    const int64_t m = idx / ks;
    const int ox = (int)(m % G), oy = (int)((m / G) % G);
    const int64_t b = m / ((int64_t)G * G);
    bf16_t* row = a0 + m * (int64_t)(2 * KH);
    bf16_t* dst = row + ky * ks * 3;
    const int iy = win.origin(oy) + ky;
    const bool iny = !Window::BORDER || (iy >= 0 && iy < S);
    auto taps = [&](int kx) {
        const int ix = win.origin(ox) + kx;
        const bool in = !Window::BORDER || (iny && ix >= 0 && ix < S);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = in ? pixel(b, c, iy, ix, S) : 0.f;
            split_hilo<F16>(v, dst[kx * 3 + c], dst[KH + kx * 3 + c]);
        }
    };
    if constexpr (Window::SIZE > 0) {
#pragma unroll
        for (int kx = 0; kx < Window::SIZE; ++kx) taps(kx);
    } else {
        for (int kx = 0; kx < ks; ++kx) taps(kx);
    }
    if constexpr (Window::ZERO_PAD) {
        if (ky == 0) {
#pragma unroll
            for (int k = 3 * Window::SIZE * Window::SIZE; k < KH; ++k) {
                row[k] = to_op<F16>(0.f);
                row[KH + k] = to_op<F16>(0.f);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The ViT's uint8 patch matrix: A0[m][(ky*P + kx)*3 + c] = 16bit(raw byte), c in memory (RGB) order -- one half, not hi | lo.
// One thread per (token, ky): reads P*3 contiguous bytes, writes P*3 contiguous 16-bit values.
// ---------------------------------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(256) void patchify_u8_kernel(const uint8_t* __restrict__ img, bf16_t* __restrict__ a0, int batch,
                                                          int size, int P, int grid) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)batch * grid * grid * P;
    if (idx >= total) return;
    const int ky = (int)(idx % P);
    const int64_t tok = idx / P;
    const int px = (int)(tok % grid), py = (int)((tok / grid) % grid), b = (int)(tok / ((int64_t)grid * grid));
    const uint8_t* src = img + (((int64_t)b * size + (py * P + ky)) * size + px * P) * 3;
    bf16_t* dst = a0 + tok * (int64_t)(P * P * 3) + ky * P * 3;
    // The pixel is stored as the exact integer 0..255 (exact in bf16).  ToTensor + Normalize,
    // x = (u/255 - .5)/.5 = u*(2/255) - 1, is affine, so it is applied to the fp32 accumulator in the
    // GEMM epilogue: W.x = (2/255) W.u - rowsum(W).  Rounding x itself to bf16 would put the same
    // 256 rounding errors on every token -- a systematic error that mean-pooling does not average out.
    if (P == 16) {          // 48 contiguous bytes in, 96 contiguous bytes out: three 16-B loads, six 16-B stores
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
        uint4* d4 = reinterpret_cast<uint4*>(dst);
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const uint4 in = s4[v];
            const uint32_t w[4] = {in.x, in.y, in.z, in.w};
            bf16x8 lo, hi;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                lo[e] = to_op<F16>((float)((w[e >> 2] >> (8 * (e & 3))) & 0xffu));
                hi[e] = to_op<F16>((float)((w[2 + (e >> 2)] >> (8 * (e & 3))) & 0xffu));
            }
            d4[2 * v] = *reinterpret_cast<const uint4*>(&lo);
            d4[2 * v + 1] = *reinterpret_cast<const uint4*>(&hi);
        }
        return;
    }
    for (int i = 0; i < P * 3; ++i) dst[i] = to_op<F16>((float)src[i]);
}

}  // namespace
