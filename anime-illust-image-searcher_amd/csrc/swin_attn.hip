// swin_attn.hip -- SwinV2 window attention (timm `swin_transformer_v2.py` WindowAttention + the block's roll / partition) for head_dim 32.
//
// For every (image, window, head): the window's T = w * w tokens attend to each other with
//   score(p, p') = cos(q_p, k_p') * exp(min(logit_scale[h], ln 100)) + cpb[h][rel(p, p')] + (region(p) != region(p') ? -100 : 0)
// where cos is the product of F.normalize-d vectors (divide by max(|.|_2, 1e-12)), cpb the compact [(2w - 1)^2] table of
// 16 sigmoid(cpb_mlp(.)) per head (swinv2.hip computes it once per checkpoint), and -100 -- literally, not -inf -- the mask of the
// shifted windows between tokens from different roll regions.
//
// Shift and partition are index math only: token (py, px) of window (wy, wx) is raster token ((wy w + py + s) mod H, (wx w + px + s) mod H)
// of the image, in `qkv` (float32 [B * H * H][3 C], the q | k | v GEMM output with its bias) and in `out` (16-bit [B * H * H][C], head h at
// columns 32 h).  The region of a token is taken from its rolled coordinates, (hr < H - w ? 0 : hr < H - s ? 1 : 2) per axis, as timm's
// attn_mask slices the rolled image.
//
// One workgroup (4 waves) per (image, window, head).  Precision: q and k are normalised in float32 at load and rounded once, as hi | lo
// 16-bit pairs of 16 x the unit vector with the low half scaled by 2^11 (normal even in IEEE half); the cosine is
// (hi.hi + 2^-11 (lo.hi + hi.lo)) / 256, three MFMAs in two accumulators -- the scale of up to 100 multiplies every rounding of the unit
// vectors.  V and the softmax numerators (256 exp(s - max), in the normal range of half) are single 16-bit roundings, as in the other
// attention kernels; the row sum adds the rounded numerators.
//   S^T = K Q^T   v_mfma_f32_16x16x32: A = 16 keys x 32 dims from LDS, B = 16 queries held in registers; the accumulator has the query on
//                 the lane (l % 16) and keys 4 (l / 16) + r in its four registers, so a row's maximum and sum are one register walk plus two
//                 cross-lane steps.
//   O^T = V^T P^T the score registers of two key tiles are directly the B operand (k order 8 g + j -> key 4 g + j, 16 + 4 g + j - 4); V^T is
//                 read from LDS in that order (two 8-byte reads).  O^T keeps the query on the lane: the final 1 / l is lane-local.
// The whole row (<= 256 keys, padded to a multiple of 32, padded keys masked) sits in registers: the softmax is exact two-pass.
#include "vit_internal.h"
#include "row_ln.h"

namespace hipts {
namespace {

constexpr int SW_MAXT = 256;            // window tokens
constexpr int SW_KS = 40;               // LDS elements per K row (80 B: conflict-free 16-byte fragment reads)
constexpr int SW_VS = SW_MAXT + 4;      // LDS elements per V^T row
constexpr int SW_MAXB = 31 * 31;        // (2 w - 1)^2 for w <= 16
constexpr float SW_LO = 2048.0f;        // scale of the low halves
constexpr float SW_U = 16.0f;           // scale of the unit vectors (both halves): IEEE half keeps components down to 2^-18 normal
constexpr float SW_P = 256.0f;          // scale of the softmax numerators: the 16-bit rounding keeps p down to 2^-22 of the row maximum normal
constexpr float SW_LN100 = 4.605170185988091f;

struct SwMeta { short py, px; int region; };      // per window token: position, roll region (-1: padding)

template <bool F16, int NC>
__global__ __launch_bounds__(256) void swin_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ logit_scale,
                                                        const float* __restrict__ cpb, bf16_t* __restrict__ out, int H, int w, int shift,
                                                        int heads) {
    constexpr int TP = 32 * NC;         // padded window tokens
    __shared__ __attribute__((aligned(16))) bf16_t khi[TP * SW_KS];
    __shared__ __attribute__((aligned(16))) bf16_t klo[TP * SW_KS];
    __shared__ __attribute__((aligned(16))) bf16_t vt[32 * SW_VS];
    __shared__ float bias_l[SW_MAXB];
    __shared__ SwMeta meta[TP];
    __shared__ int rows[TP];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = heads * 32, ld = 3 * C;
    const int nwx = H / w, T = w * w, nb = (2 * w - 1) * (2 * w - 1);
    int bid = blockIdx.x;
    const int h = bid % heads;
    bid /= heads;
    const int win = bid % (nwx * nwx);
    const int64_t b = bid / (nwx * nwx);
    const int wy = win / nwx, wx = win - wy * nwx;

    for (int i = tid; i < nb; i += 256) bias_l[i] = cpb[(size_t)h * nb + i];
    for (int t = tid; t < TP; t += 256) {
        SwMeta m{0, 0, -1};
        int row = 0;
        if (t < T) {
            const int py = t / w, px = t - (t / w) * w;
            const int hr = wy * w + py, wr = wx * w + px;
            int oy = hr + shift, ox = wr + shift;
            if (oy >= H) oy -= H;
            if (ox >= H) ox -= H;
            row = oy * H + ox;
            int reg = 0;
            if (shift > 0) reg = 3 * (hr < H - w ? 0 : hr < H - shift ? 1 : 2) + (wr < H - w ? 0 : wr < H - shift ? 1 : 2);
            m = SwMeta{(short)py, (short)px, reg};
        }
        meta[t] = m;
        rows[t] = row;
    }
    __syncthreads();

    // K (normalised, hi | lo) and V^T into LDS: 8 threads per token, 4 dims each
    const float* base = qkv + (size_t)b * H * H * ld;
    for (int t0 = 0; t0 < TP; t0 += 32) {
        const int t = t0 + (tid >> 3), d0 = 4 * (tid & 7);
        float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
        if (t < T) {
            const float* r = base + (size_t)rows[t] * ld + h * 32 + d0;
            kv = *reinterpret_cast<const float4*>(r + C);
            vv = *reinterpret_cast<const float4*>(r + 2 * C);
        }
        float ss = (kv.x * kv.x + kv.y * kv.y) + (kv.z * kv.z + kv.w * kv.w);
        ss += __shfl_xor(ss, 1);
        ss += __shfl_xor(ss, 2);
        ss += __shfl_xor(ss, 4);
        const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
        const float kn[4] = {kv.x * inv * SW_U, kv.y * inv * SW_U, kv.z * inv * SW_U, kv.w * inv * SW_U};
        const float vn[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            split_hilo<F16>(kn[i], khi[t * SW_KS + d0 + i], klo[t * SW_KS + d0 + i], SW_LO);
            vt[(d0 + i) * SW_VS + t] = to_op<F16>(vn[i]);
        }
    }
    __syncthreads();

    const float scale = expf(fminf(logit_scale[h], SW_LN100));
    const int ql = lane & 15, g = lane >> 4;
    const int nqt = (T + 15) >> 4;
    for (int qt = wave; qt < nqt; qt += 4) {
        const int qi = qt * 16 + ql;
        const bool qv = qi < T;
        // this lane's 8 dims of its query, normalised across the 4 lanes that share it
        float qf[8];
        {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = a;
            if (qv) {
                const float* r = base + (size_t)rows[qi] * ld + h * 32 + 8 * g;
                a = *reinterpret_cast<const float4*>(r);
                c = *reinterpret_cast<const float4*>(r + 4);
            }
            qf[0] = a.x; qf[1] = a.y; qf[2] = a.z; qf[3] = a.w; qf[4] = c.x; qf[5] = c.y; qf[6] = c.z; qf[7] = c.w;
        }
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < 8; i += 2) ss += qf[i] * qf[i] + qf[i + 1] * qf[i + 1];
        ss += __shfl_xor(ss, 16);
        ss += __shfl_xor(ss, 32);
        const float qinv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
        bf16x8 qhi, qlo;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            bf16_t hb, lb;
            split_hilo<F16>(qf[i] * qinv * SW_U, hb, lb, SW_LO);
            qhi[i] = hb;
            qlo[i] = lb;
        }
        const SwMeta mq = meta[qi < TP ? qi : 0];
        const int boff = (mq.py + w - 1) * (2 * w - 1) + (mq.px + w - 1);

        // scores of this lane's query against keys 16 kt + 4 g + r
        f32x4 s[2 * NC];
        float mx = -3.0e38f;
#pragma unroll
        for (int kt = 0; kt < 2 * NC; ++kt) {
            const int kr = kt * 16 + ql;
            const bf16x8 ahi = *reinterpret_cast<const bf16x8*>(khi + kr * SW_KS + 8 * g);
            const bf16x8 alo = *reinterpret_cast<const bf16x8*>(klo + kr * SW_KS + 8 * g);
            f32x4 hh = mfma_16x16x32<F16>(ahi, qhi, f32x4{0.f, 0.f, 0.f, 0.f});
            f32x4 x = mfma_16x16x32<F16>(alo, qhi, f32x4{0.f, 0.f, 0.f, 0.f});
            x = mfma_16x16x32<F16>(ahi, qlo, x);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kt * 16 + 4 * g + r;
                const SwMeta mk = meta[key];
                float v;
                if (mk.region < 0) {
                    v = -3.0e38f;
                } else {
                    v = (hh[r] + x[r] * (1.0f / SW_LO)) * (1.0f / (SW_U * SW_U)) * scale + bias_l[boff - mk.py * (2 * w - 1) - mk.px];
                    if (mk.region != mq.region) v += -100.0f;
                }
                s[kt][r] = v;
                mx = fmaxf(mx, v);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));

        // numerators (16-bit), their sum, and O^T = V^T P^T per 32-key chunk
        float l = 0.f;
        f32x4 o0{0.f, 0.f, 0.f, 0.f}, o1{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            bf16x8 p;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float e = __expf(s[2 * c + (j >> 2)][j & 3] - mx) * SW_P;
                const bf16_t pb = to_op<F16>(e);
                p[j] = pb;
                l += from_op<F16>(pb);
            }
            const int k0 = 32 * c + 4 * g;
            bf16x8 v0, v1;
            const bf16x4 a0 = *reinterpret_cast<const bf16x4*>(vt + ql * SW_VS + k0);
            const bf16x4 a1 = *reinterpret_cast<const bf16x4*>(vt + ql * SW_VS + k0 + 16);
            const bf16x4 b0 = *reinterpret_cast<const bf16x4*>(vt + (ql + 16) * SW_VS + k0);
            const bf16x4 b1 = *reinterpret_cast<const bf16x4*>(vt + (ql + 16) * SW_VS + k0 + 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v0[j] = a0[j]; v0[4 + j] = a1[j];
                v1[j] = b0[j]; v1[4 + j] = b1[j];
            }
            o0 = mfma_16x16x32<F16>(v0, p, o0);
            o1 = mfma_16x16x32<F16>(v1, p, o1);
        }
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        if (qv) {
            const float il = 1.0f / l;
            bf16_t* orow = out + ((size_t)b * H * H + rows[qi]) * C + h * 32 + 4 * g;
            *reinterpret_cast<bf16x4*>(orow) = pack4<F16>(o0[0] * il, o0[1] * il, o0[2] * il, o0[3] * il);
            *reinterpret_cast<bf16x4*>(orow + 16) = pack4<F16>(o1[0] * il, o1[1] * il, o1[2] * il, o1[3] * il);
        }
    }
}

template <bool F16>
int launch_nc(int nc, const float* qkv, const float* ls, const float* cpb, bf16_t* out, int grid, int H, int w, int shift, int heads,
              hipStream_t s) {
    switch (nc) {
#define SW_CASE(N) \
        case N: swin_attn_kernel<F16, N><<<grid, 256, 0, s>>>(qkv, ls, cpb, out, H, w, shift, heads); break;
        SW_CASE(1) SW_CASE(2) SW_CASE(3) SW_CASE(4) SW_CASE(5) SW_CASE(6) SW_CASE(7) SW_CASE(8)
#undef SW_CASE
        default: return set_error(HIPTS_ERR_INVALID, "swin attention: %d key chunks", nc);
    }
    HIPTS_LAUNCH_CHECK();
    return HIPTS_OK;
}

}  // namespace

int launch_swin_attention(const float* qkv, const float* logit_scale, const float* cpb, bf16_t* out, int batch, int side, int window,
                          int shift, int heads, bool f16, hipStream_t s) {
    HIPTS_REQUIRE(qkv && logit_scale && cpb && out && batch >= 1 && heads >= 1, "swin attention: bad arguments");
    HIPTS_REQUIRE(window >= 2 && window * window <= SW_MAXT && side % window == 0, "swin attention: window %d (<= 16) must divide side %d",
                  window, side);
    HIPTS_REQUIRE(shift >= 0 && shift < window && (shift == 0 || side > window), "swin attention: shift %d for window %d, side %d", shift,
                  window, side);
    const int nw = side / window;
    const int64_t grid = (int64_t)batch * nw * nw * heads;
    HIPTS_REQUIRE(grid < (1ll << 31), "swin attention: grid too large");
    const int nc = (window * window + 31) / 32;
    return f16 ? launch_nc<true>(nc, qkv, logit_scale, cpb, out, (int)grid, side, window, shift, heads, s)
               : launch_nc<false>(nc, qkv, logit_scale, cpb, out, (int)grid, side, window, shift, heads, s);
}

}  // namespace hipts
