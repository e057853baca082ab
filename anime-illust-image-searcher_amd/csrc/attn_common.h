// attn_common.h -- what the attention kernels of attn.hip (head_dim 32 / 64, V transposed) and attn2.hip + attn3.h (head_dim 64, LDS-DMA)
// must agree on, stated once: the head room of the half-operand reference exponent, the accumulator's register -> key row map, the
// reference exponent itself, the window a fast pass's row sum has to stay in, and the switch that sends every workgroup down the
// classic pass.  Device functions are __forceinline__ and carry no state.
#pragma once
#include "vit_internal.h"

// Head room of the half-operand fast path's reference exponent (round 4): m_ref = (the row's maximum over its first 32 keys) + this many
// bits, so P = 2^(S - m_ref) overflows half only when a later score exceeds that maximum by 15 + MARGIN bits, and the row sum's window is
// [2^(-1 - MARGIN), 2^15); keys more than 14 - MARGIN bits below the reference become half subnormals (their P keeps an absolute
// precision of 2^-24, against a row sum of at least 2^-MARGIN).  With 0 a padded picture (prepare_image's white bars are the first keys of every row, tagging.py:100-120) sent most
// query blocks through the fast pass AND the classic one: 4.6 k images/s where noise runs at 5.3 k (tools/vit_content_bench.py).
#ifndef HIPTS_ATTN_REF_MARGIN
#define HIPTS_ATTN_REF_MARGIN 10     // measured (r4_margin.sh, the round-4 margin sweep), padded picture: 0 / 4 / 8 / 10 / 12 bits -> 4667 / 4979 / 5199-5298 / 5261 / 5311 images/s (noise 5340-5435 at every setting); EVA02-L 1129 / 1158 / 1164 at 8 / 10 / 12 (noise 1176); at 12 an attention test fails (the reference keys' P sits two bits above the half subnormals), at 10 the oracle check of the structured images is unchanged
#endif
namespace hipts {

// HIPTS_ATTN_CLASSIC=1: the per-tile running maximum everywhere (A/B runs; the fallback's own test).  Read once per process.
inline int attn_classic_switch() {
    static const int classic = (getenv("HIPTS_ATTN_CLASSIC") && atoi(getenv("HIPTS_ATTN_CLASSIC"))) ? 1 : 0;
    return classic;
}

namespace {

// key row (of 32) that register `reg` of a 32 x 32 accumulator holds in the lane half h
__device__ __forceinline__ int crow(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// The half-operand reference exponent of a query row (the lane and its partner lane + 32 hold the row's scores): the maximum over the
// GH 32-key score blocks s[0 .. GH) plus the head room.  Finite: the first tile holds at least one unmasked key.
template <int GH>
__device__ __forceinline__ float ref_exponent(const f32x16* s) {
    float mx = s[0][0];
#pragma unroll
    for (int g = 0; g < GH; ++g)
#pragma unroll
        for (int i = (g == 0 ? 1 : 0); i < 16; ++i) mx = fmaxf(mx, s[g][i]);
    return fmaxf(mx, __shfl_xor(mx, 32)) + (float)HIPTS_ATTN_REF_MARGIN;
}

// True when a fast pass's row sum left its window: 2^(-1 - MARGIN) <= l < 2^15 (half) / 2^-100 <= l < 2^100 (bf16), tested on the bit
// pattern: positive floats order like their bits, a negative value or a NaN (>= 0x7f800001, or sign bit set) falls outside whatever the
// compiler assumes about NaNs (-fno-honor-nans).
template <bool F16>
__device__ __forceinline__ bool row_sum_left_window(float l_tot) {
    const uint32_t lb = __float_as_uint(l_tot);
    constexpr uint32_t LO = F16 ? 0x3f000000u - ((uint32_t)HIPTS_ATTN_REF_MARGIN << 23) : 0x0d800000u, HI = F16 ? 0x47000000u : 0x71800000u;
    return !(lb >= LO && lb < HI);
}

}  // namespace
}  // namespace hipts
