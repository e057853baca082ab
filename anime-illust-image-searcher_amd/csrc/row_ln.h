// row_ln.h -- the "one wave per row" LayerNorm of the five forwards (vit.hip, eva.hip and ccip.hip through launch_layernorm; ccip.hip,
// convnext.hip, swinv2.hip directly), the wave reduction and row statistics it is built from, the hi | lo operand split, and the pooled
// LayerNorm head (pool_ln_kernel, at the end).  Device code only.  Everything lives in an anonymous namespace, so each including object gets its own copy under the same symbol names.
//
// Batch invariance and the parity bounds of the models rest on every LayerNorm rounding alike: there is ONE body, row_ln_kernel, and
// what differs between its uses is a compile-time policy -- where the row comes from, which affine is applied, where the result goes.
// The build uses -ffp-contract=off: (v - mean) * rstd * g + b is three roundings in that order wherever it is written below.
#pragma once
#include <type_traits>

#include "vit_internal.h"

namespace {

using namespace hipts;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---------------------------------------------------------------------------------------------
// The hi | lo operand split: a float32 value as two 16-bit halves, hi = 16bit(v), lo = 16bit((v - hi) * lo_scale), multiplied against
// [W | W / lo_scale] by the consumer (22 significant bits of an IEEE-half operand, 16 of a bf16 one).
// ---------------------------------------------------------------------------------------------
template <bool F16>
__device__ __forceinline__ void split_hilo(float v, bf16_t& hi, bf16_t& lo) {
    hi = to_op<F16>(v);
    lo = to_op<F16>(v - from_op<F16>(hi));
}
template <bool F16>
__device__ __forceinline__ void split_hilo(float v, bf16_t& hi, bf16_t& lo, float lo_scale) {
    hi = to_op<F16>(v);
    lo = to_op<F16>((v - from_op<F16>(hi)) * lo_scale);
}
template <bool F16>
__device__ __forceinline__ void split_hilo4(float4 v, bf16x4& hi, bf16x4& lo) {
    hi = pack4<F16>(v.x, v.y, v.z, v.w);
    lo = pack4<F16>(v.x - from_op<F16>(hi[0]), v.y - from_op<F16>(hi[1]), v.z - from_op<F16>(hi[2]), v.w - from_op<F16>(hi[3]));
}

// ---------------------------------------------------------------------------------------------
// Row statistics of one row held by a wave as up to four float4 per lane (D <= 1024, D % 4 == 0; the lanes beyond the row hold zeros):
// two passes in registers, eps inside the sqrt, biased variance (torch F.layer_norm).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void row_mean_rstd(const float4 (&v)[4], int lane, int D, float eps, float& mean, float& rstd) {
    const int nvec = D >> 2;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    mean = wave_sum(s) / (float)D;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (lane + 64 * i < nvec) {
            const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
            ss += (a * a + b * b) + (c * c + d * d);
        }
    rstd = 1.0f / sqrtf(wave_sum(ss) / (float)D + eps);
}

// ---------------------------------------------------------------------------------------------
// row_ln_kernel<F16>(src, affine, sink, rows, D, eps): sink[row] = affine((src[row] - mean) * rstd).  256 threads = four rows per
// workgroup, one wave per row, up to four float4 per lane; D % 4 == 0, D <= 1024.  F16 is the 16-bit operand type of the policies that
// read or write one (HIPTS_LAUNCH_F16); the others ignore it and are launched as <false>.
//
// A source or sink is passed by value: seek(row, D) moves it to its row once, then load<F16>(c) / store<F16>(c, o) handle float4 c of the
// row.  A source of plain float32 returns f32x4, not float4: the kernel chooses between the loaded value and zeros on that type, and
// only a choice between whole 16-byte vectors keeps each load in one register quad -- all loads of a row in flight, one wait.  Chosen
// member by member (float4), the compiler shuffles registers behind every load and waits for each in turn.
// ---------------------------------------------------------------------------------------------

// ---- sources
__device__ __forceinline__ float4 as_float4(float4 v) { return v; }
__device__ __forceinline__ float4 as_float4(f32x4 v) { return make_float4(v[0], v[1], v[2], v[3]); }

struct FromF32 {                        // float32 rows, row-major
    const float* x;
    __device__ void seek(int64_t row, int D) { x += row * D; }
    template <bool F16>
    __device__ f32x4 load(int c) const { return reinterpret_cast<const f32x4*>(x)[c]; }
};

// Element offsets of the fp32 residual stream stored as 16 x 16 blocks of 1 KB, [m / 16][n / 16][m % 16][n % 16] (gemm_epi.h::x_off):
// of a row's first element, and of its float4 c from there
__device__ __forceinline__ int64_t x_blk_row(int64_t row, int D) { return (((row >> 4) * (int64_t)(D >> 4)) << 8) + (row & 15) * 16; }
__device__ __forceinline__ int x_blk_vec(int c) { return ((c >> 2) << 8) + (c & 3) * 4; }

struct FromF32Blocked {                 // float32 rows of the blocked stream
    const float* x;
    __device__ void seek(int64_t row, int D) { x += x_blk_row(row, D); }
    template <bool F16>
    __device__ f32x4 load(int c) const { return *reinterpret_cast<const f32x4*>(x + x_blk_vec(c)); }
};

// float32 rows normalised where they are (sink: BackToSource), row-major or (blk, a launch's choice) blocked.  The address is formed
// whole at every access from the row seek() noted, block index first: 40 VGPRs, against 42 with a row pointer moved by seek().
struct F32InPlace {
    float* x;
    int blk;
    int64_t row = 0;                    // set by seek()
    int D = 0;
    __device__ void seek(int64_t row_, int D_) { row = row_; D = D_; }
    __device__ float* at(int c) const {
        if (blk) return x + ((((row >> 4) * (int64_t)(D >> 4)) + (c >> 2)) << 8) + (row & 15) * 16 + (c & 3) * 4;      // = x_blk_row + x_blk_vec
        return x + row * D + 4 * c;
    }
    template <bool F16>
    __device__ f32x4 load(int c) const { return *reinterpret_cast<const f32x4*>(at(c)); }
    template <bool F16>
    __device__ void store(int c, float4 o) const { *reinterpret_cast<float4*>(at(c)) = o; }
};

struct From16Bias {                     // 16-bit rows plus a float32 bias per column, added in float32 before the statistics
    const bf16_t* h;
    const float* bias;
    __device__ void seek(int64_t row, int D) { h += row * D; }
    template <bool F16>
    __device__ float4 load(int c) const {
        const bf16x4 q = reinterpret_cast<const bf16x4*>(h)[c];
        const float4 bb = reinterpret_cast<const float4*>(bias)[c];
        return make_float4(from_op<F16>(q[0]) + bb.x, from_op<F16>(q[1]) + bb.y, from_op<F16>(q[2]) + bb.z, from_op<F16>(q[3]) + bb.w);
    }
};

// ---- affines.  A bias-free norm exists in two forms that differ in the sign of zero, and each user keeps its own: + 0.f turns a -0
// product into +0 (LnGammaOptBeta without beta, LnGamma<true>), no addition keeps it (LnGamma<false>).
__device__ __forceinline__ float4 ln_apply(float4 v, float mean, float rstd, float4 g, float4 b) {
    return make_float4((v.x - mean) * rstd * g.x + b.x, (v.y - mean) * rstd * g.y + b.y, (v.z - mean) * rstd * g.z + b.z,
                       (v.w - mean) * rstd * g.w + b.w);
}

struct LnGammaBeta {
    const float* g;
    const float* b;
    __device__ float4 operator()(float4 v, float mean, float rstd, int c) const {
        return ln_apply(v, mean, rstd, reinterpret_cast<const float4*>(g)[c], reinterpret_cast<const float4*>(b)[c]);
    }
};

struct LnGammaOptBeta {                 // b may be null (a launch's choice): zeros are added then
    const float* g;
    const float* b;
    __device__ float4 operator()(float4 v, float mean, float rstd, int c) const {
        return ln_apply(v, mean, rstd, reinterpret_cast<const float4*>(g)[c],
                        b ? reinterpret_cast<const float4*>(b)[c] : make_float4(0.f, 0.f, 0.f, 0.f));
    }
};

template <bool ADD_ZERO>
struct LnGamma {
    const float* g;
    __device__ float4 operator()(float4 v, float mean, float rstd, int c) const {
        const float4 gg = reinterpret_cast<const float4*>(g)[c];
        if constexpr (ADD_ZERO) return ln_apply(v, mean, rstd, gg, make_float4(0.f, 0.f, 0.f, 0.f));
        else return make_float4((v.x - mean) * rstd * gg.x, (v.y - mean) * rstd * gg.y, (v.z - mean) * rstd * gg.z, (v.w - mean) * rstd * gg.w);
    }
};

// ---- sinks
struct BackToSource {                   // in place: the kernel stores through the source's own store<F16>(c, o) (one row address, not two)
    __device__ void seek(int64_t, int) {}
};

struct To16 {                           // 16-bit rows, row-major
    bf16_t* out;
    __device__ void seek(int64_t row, int D) { out += row * D; }
    template <bool F16>
    __device__ void store(int c, float4 o) const { reinterpret_cast<bf16x4*>(out)[c] = pack4<F16>(o.x, o.y, o.z, o.w); }
};

struct ToE4m3 {                         // e4m3 bytes (the A operand of an op8 GEMM)
    uint8_t* out;
    __device__ void seek(int64_t row, int D) { out += row * D; }
    template <bool F16>
    __device__ void store(int c, float4 o) const { reinterpret_cast<uint32_t*>(out)[c] = pack4_e4m3(o.x, o.y, o.z, o.w); }
};

struct ToF32 {                          // float32 rows of another buffer
    float* y;
    __device__ void seek(int64_t row, int D) { y += row * D; }
    template <bool F16>
    __device__ void store(int c, float4 o) const { reinterpret_cast<float4*>(y)[c] = o; }
};

struct ToF32And16 {                     // float32 rows (x may be the source: in place) and their 16-bit copy, rounded from the value stored
    float* x;
    bf16_t* xh;
    __device__ void seek(int64_t row, int D) { x += row * D; xh += row * D; }
    template <bool F16>
    __device__ void store(int c, float4 o) const {
        reinterpret_cast<float4*>(x)[c] = o;
        reinterpret_cast<bf16x4*>(xh)[c] = pack4<F16>(o.x, o.y, o.z, o.w);
    }
};

struct ToPatch2x2 {                     // input token (b, iy, ix) of an H x H map into its place in the 2 x 2 s2 patch matrix:
    bf16_t* col;                        // col[(b, iy / 2, ix / 2)][((iy & 1) * 2 + (ix & 1)) * D + c].  The patches do not overlap.
    int H;
    __device__ void seek(int64_t row, int D) {
        const int ix = (int)(row % H), iy = (int)((row / H) % H);
        const int64_t b = row / ((int64_t)H * H);
        const int Ho = H >> 1;
        col += (((b * Ho + (iy >> 1)) * Ho + (ix >> 1)) * 4 + ((iy & 1) * 2 + (ix & 1))) * (int64_t)D;
    }
    template <bool F16>
    __device__ void store(int c, float4 o) const { reinterpret_cast<bf16x4*>(col)[c] = pack4<F16>(o.x, o.y, o.z, o.w); }
};

struct AddToStreamHiLo {                // post-norm residual: x += o, then the hi | lo halves of the NEW x into rows of 2 D:
    float* x;                           // hi = the rows' base, lo = hi + D
    bf16_t* hi;
    bf16_t* lo;
    __device__ void seek(int64_t row, int D) { x += row * D; hi += row * 2 * D; lo += row * 2 * D; }
    template <bool F16>
    __device__ void store(int c, float4 o) const {
        float4 n = reinterpret_cast<float4*>(x)[c];
        n.x += o.x; n.y += o.y; n.z += o.z; n.w += o.w;
        reinterpret_cast<float4*>(x)[c] = n;
        split_hilo4<F16>(n, reinterpret_cast<bf16x4*>(hi)[c], reinterpret_cast<bf16x4*>(lo)[c]);
    }
};

template <bool F16, class Src, class Affine, class Sink>
__global__ __launch_bounds__(256) void row_ln_kernel(Src src, Affine affine, Sink sink, int64_t rows, int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nvec = D >> 2;
    src.seek(row, D);
    using Loaded = decltype(src.template load<F16>(0));
    Loaded r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        r[i] = c < nvec ? src.template load<F16>(c) : Loaded{};
    }
    float4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = as_float4(r[i]);
    float mean, rstd;
    row_mean_rstd(v, lane, D, eps, mean, rstd);
    sink.seek(row, D);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        if (c < nvec) {
            const float4 o = affine(v[i], mean, rstd, c);
            if constexpr (std::is_same<Sink, BackToSource>::value) src.template store<F16>(c, o);
            else sink.template store<F16>(c, o);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The pooled LayerNorm head of ccip.hip, convnext.hip and eva.hip (one workgroup per image), and where a pooled feature goes (also
// swinv2.hip's token mean): store<F16>(image b, width C, column c, value).  F16 is the operand type of the 16-bit sink; the float32
// one ignores it and is launched as <false>.
// ---------------------------------------------------------------------------------------------
struct PooledF32 {                      // float32 rows
    float* out;
    template <bool F16>
    __device__ void store(int64_t b, int C, int c, float f) const { out[b * C + c] = f; }
};

struct PooledHiLo {                     // hi | lo halves, the A operand of a head GEMM with K = 2 C against [W | W]: [b][c] = hi, [b][C + c] = lo
    bf16_t* out;
    template <bool F16>
    __device__ void store(int64_t b, int C, int c, float f) const { split_hilo<F16>(f, out[b * 2 * C + c], out[b * 2 * C + C + c]); }
};

// Head: sink[b][:] = LN((sum over the T rows of x[b]) / count)  (with bias): count = T for the mean over an image's tokens, or the
// tokens behind T partial row sums (eva.hip).  One 1024-thread workgroup per image:
// four row groups x 256 channel threads sum a quarter of the rows each (the loop is load-latency bound,
// so more rows in flight is what matters), partial sums meet in LDS, the first 256 threads normalise.
template <bool F16, class Sink>
__global__ __launch_bounds__(1024) void pool_ln_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ bta,
                                                       Sink sink, int T, int C, float eps, int blk, int count) {
    __shared__ float part[4][1024];
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x & 255, rg = threadIdx.x >> 8;
    const float* xb = x + (int64_t)b * T * C;
    float m[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int r = rg; r < T; r += 4)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = tid + 256 * u;
            if (c < C) m[u] += blk ? xb[((((int64_t)(r >> 4) * (C >> 4)) + (c >> 4)) << 8) + (r & 15) * 16 + (c & 15)] : xb[(int64_t)r * C + c];
        }
#pragma unroll
    for (int u = 0; u < 4; ++u) part[rg][tid + 256 * u] = m[u];
    __syncthreads();
    // (every thread keeps walking to the barriers; only row group 0 does the arithmetic)
    float s = 0.f;
    if (rg == 0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = tid + 256 * u;
            m[u] = ((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) / (float)count;
            if (c < C) s += m[u];
        }
        s = wave_sum(s);
        if ((tid & 63) == 0) red[tid >> 6] = s;
    }
    __syncthreads();
    const float mean = (red[0] + red[1] + red[2] + red[3]) / (float)C;
    __syncthreads();
    if (rg == 0) {
        float ss = 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (tid + 256 * u < C) ss += (m[u] - mean) * (m[u] - mean);
        ss = wave_sum(ss);
        if ((tid & 63) == 0) red[tid >> 6] = ss;
    }
    __syncthreads();
    if (rg != 0) return;
    const float rstd = 1.0f / sqrtf((red[0] + red[1] + red[2] + red[3]) / (float)C + eps);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = tid + 256 * u;
        if (c < C) sink.template store<F16>(b, C, c, (m[u] - mean) * rstd * g[c] + bta[c]);
    }
}

}  // namespace
