// swinv2.hip -- SwinV2 tagger forward (wd-swinv2-tagger-v3 = timm `swinv2_base_window8_256` built with img_size 448, window_size 14)
// behind hipts_swinv2_*.
//
// Layer algebra (timm `models/swin_transformer_v2.py`, >= 0.9 layout):
//   stem      x = LN(Conv2d(3, C0, k = 4, s = 4)(img) + b)
//   stage i   (i > 0) patch merging: x = LN(Linear(4 C_{i-1} -> C_i, no bias)(cat of the 2 x 2 neighbours, (dy, dx) = (0,0) (1,0) (0,1) (1,1)))
//             blocks (shift s = 0 for even j, window / 2 for odd j; a stage whose side is <= window attends over the whole map, unshifted):
//               x = x + LN1(proj(WindowAttn(x)))          x = x + LN2(fc2(GELU(fc1(x))))          (post-norm; qkv and fc1 read x)
//   head      logits = fc(mean over tokens of LN(x)), probs = sigmoid(logits)
//
// Data layout as in the ConvNeXt forward: token-major NHWC, the residual stream x float32 [B*H*W][C], its hi | lo 16-bit halves xh2
// [B*H*W][2 C] the A operand of q | k | v and fc1.  Every Linear is the shared persistent MFMA GEMM (gemm.hip):
//   stem          patch_rows.h's patch_gather_kernel (hi | lo halves, Window4x4) -> EPI_BIAS -> row_ln.h's row_ln_kernel (LayerNorm with bias in
//                 place, the ToF32And16 sink the ConvNeXt stem uses; its 16-bit copy xh is not read here) -> sw_split_x_kernel (xh2)
//   merging       sw_merge_kernel (2 x 2 gather in timm's order as hi | lo halves of the fp32 stream) -> EPI_BIAS (K = 8 C, zero bias)
//                 -> row_ln_kernel in place, as the stem
//   q | k | v     EPI_BIAS into float32 [M][3 C] (bias [q_bias | 0 | v_bias]) from the hi | lo halves of x (xh2, K = 2 C against
//                 [W | W]).  The cosine multiplies q and k by up to 100 after normalisation: a single 16-bit rounding of x moves a score
//                 by ~2e-2 (measured: 0.6 max |dlogit| on the trained-like checkpoint).  q and k reach the attention in float32, which
//                 normalises them before its own hi | lo rounding (swin_attn.hip)
//   attention     launch_swin_attention: windows, shift, cosine, position bias and the -100 mask as index math; 16-bit output
//   proj, fc2     EPI_BIAS into the float32 branch buffer, then row_ln_kernel with the AddToStreamHiLo sink (one wave per row):
//                 x += LN(branch) (weight, bias) and xh2 = the hi | lo halves of the new x, the operand of fc1 / of the next block's q | k | v.  One form for every stage: which kernels run
//                 depends on the configuration only, never on the batch or its split.
//   fc1           EPI_GELU from xh2 (K = 2 C against [W | W]; gelu_tanh from the configuration, 0 = the erf form).  The hi | lo operands
//                 of merging, q | k | v and fc1 are what brings a flat picture's logits within 1e-3 of float64: its tokens share every
//                 rounding error, which the mean over tokens then cannot average out
//   head          row_ln_kernel with the ToF32 sink (per-token LayerNorm, float32) -> sw_mean_kernel (hi | lo, the PooledHiLo sink) -> EPI_HEAD
// Tested one launch at a time: sw_merge_kernel, sw_split_x_kernel and sw_mean_kernel through hiptsdbg_swinv2_merge / _split_x / _mean
// below (tests/test_gpu_tokens.py: bit for bit against the reshape / permute, exact-answer means, float64), the row_ln_kernel sinks and
// the patch gather through csrc/rows_dbg.hip (tests/test_gpu_rows.py), the window attention through hiptsdbg_swinv2_window_attention and
// the whole forward against swinv2_ref (tests/test_gpu_swinv2.py).  Each launch_sw_* helper is the one launch shape the forward and its
// entry share.
// The position-bias tables 16 sigmoid(cpb_mlp(table)) depend on the weights only: computed on the host (double, stored float32) at the
// first forward after the last cpb_mlp tensor was set, [heads][(2 w - 1)^2] per block.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "vit_internal.h"
#include "dbg_buf.h"
#include "model_host.h"
#include "convnet.h"

using namespace hipts;

namespace {

constexpr int SW_CPB_HIDDEN = 512;               // timm's cpb_mlp: Linear(2, 512) -> ReLU -> Linear(512, heads, no bias)

struct SwBlock {
    int shift = 0;
    DevBuf qkv2, qkv_b, proj, proj_b, n1_w, n1_b, fc1, fc1_b, fc2, fc2_b, n2_w, n2_b, ls, cpb;
    std::vector<float> qkv_bh;                   // host [q_bias | 0 | v_bias]
    std::vector<float> cpb_w1, cpb_b1, cpb_w2;   // host copies of cpb_mlp.{0.weight, 0.bias, 2.weight}
};

struct SwStage {
    int C = 0, H = 0, T = 0, heads = 0, win = 0, hid = 0;
    DevBuf ds_w, ds_b, ds_nw, ds_nb;             // patch merging (stage > 0): reduction [C][4 Cprev] (timm's column order), zero bias, LN
    std::vector<SwBlock> blocks;
};

}  // namespace

struct hipts_swinv2 {
    int device = 0;
    hipts_swinv2_config_t cfg{};
    SwStage st[4];
    DevBuf stem_w, stem_b, stem_nw, stem_nb, head_nw, head_nb, head_w, head_b, lut;
    TensorLedger ledger;
    bool cpb_ready = false;
    // workspace (sized for cfg.max_batch), carved per image with the stride of the largest stage
    DevBuf img_in, a0, x, xh, xh2, qkv, ao, br, m1, col, feat2, logits, probs;
    size_t px = 0, p3c = 0, phid = 0, pcol = 0;
    SubStreams<2> streams;
    double flops_per_image = 0.0;
};

namespace {

// Patch merging gather as hi | lo halves: col[(b, oy, ox)][q * C + c] = hi and [4 C + q * C + c] = lo of x[b][2 oy + dy][2 ox + dx][c] with
// q = 2 dx + dy -- timm's reshape(B, H/2, 2, W/2, 2, C).permute(0, 1, 3, 4, 2, 5) order, so the reduction weight is used as it is (twice:
// [W | W]).  One thread per float4 of the hi half.
template <bool F16>
__global__ __launch_bounds__(256) void sw_merge_kernel(const float* __restrict__ x, bf16_t* __restrict__ col, int64_t total4, int H, int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int c4 = C >> 2;
    const int c = (int)(i % c4) * 4;
    int64_t r = i / c4;
    const int q = (int)(r & 3);
    r >>= 2;
    const int Ho = H >> 1;
    const int ox = (int)(r % Ho), oy = (int)((r / Ho) % Ho);
    const int64_t b = r / ((int64_t)Ho * Ho);
    const int dy = q & 1, dx = q >> 1;
    const float4 v = *reinterpret_cast<const float4*>(x + ((b * H + 2 * oy + dy) * H + 2 * ox + dx) * C + c);
    bf16_t* dst = col + r * 8 * C + q * C + c;
    split_hilo4<F16>(v, *reinterpret_cast<bf16x4*>(dst), *reinterpret_cast<bf16x4*>(dst + 4 * C));
}

// x as hi | lo halves, xh2[m] = [16bit(x[m]) | 16bit(x[m] - hi)] (behind the stem and merging LayerNorms).  One thread per float4.
template <bool F16>
__global__ __launch_bounds__(256) void sw_split_x_kernel(const float* __restrict__ x, bf16_t* __restrict__ xh2, int64_t n4, int D) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int64_t row = i / (D >> 2);
    const int c = (int)(i - row * (D >> 2)) * 4;
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    split_hilo4<F16>(v, *reinterpret_cast<bf16x4*>(xh2 + row * 2 * D + c), *reinterpret_cast<bf16x4*>(xh2 + row * 2 * D + D + c));
}

// Mean over an image's T tokens, tokens summed in order (one workgroup per image), into a sink of the pooled head (row_ln.h).
template <bool F16, class Sink>
__global__ __launch_bounds__(256) void sw_mean_kernel(const float* __restrict__ y, Sink sink, int T, int C) {
    const int64_t b = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 256) {
        float s = 0.f;
        for (int t = 0; t < T; ++t) s += y[(b * T + t) * C + c];
        sink.template store<F16>(b, C, c, s / (float)T);
    }
}

// The three kernels' launch shapes, shared by the forward and the debug entries (hiptsdbg_swinv2_merge, _split_x, _mean).
// rows_out: the merged rows, batch * (H / 2)^2, of 4 C values each
int launch_sw_merge(bool f16, const float* x, bf16_t* col, int64_t rows_out, int H, int C, hipStream_t s) {
    const int64_t total4 = rows_out * C;               // rows_out rows of 4 C, in float4
    HIPTS_LAUNCH_F16(f16, sw_merge_kernel, ceil_div(total4, 256), 256, 0, s, x, col, total4, H, C);
    return HIPTS_OK;
}

int launch_sw_split_x(bool f16, const float* x, bf16_t* xh2, int64_t rows, int D, hipStream_t s) {
    const int64_t n4 = rows * D / 4;
    HIPTS_LAUNCH_F16(f16, sw_split_x_kernel, ceil_div(n4, 256), 256, 0, s, x, xh2, n4, D);
    return HIPTS_OK;
}

int launch_sw_mean(bool f16, const float* y, bf16_t* feat2, int batch, int T, int C, hipStream_t s) {
    HIPTS_LAUNCH_F16(f16, sw_mean_kernel, batch, 256, 0, s, y, PooledHiLo{feat2}, T, C);
    return HIPTS_OK;
}

// 16 sigmoid(cpb_mlp(table)) for one block: [heads][(2 w - 1)^2], table entry (dy, dx) = sign(t) log2(1 + |t|) / log2(8) with
// t = 8 offset / (pw - 1) per axis (pw = the window, or cpb_pretrained_window when set).
std::vector<float> sw_cpb_table(const SwBlock& B, int w, int pw, int heads) {
    const int n = 2 * w - 1;
    std::vector<float> out((size_t)heads * n * n);
    std::vector<double> hid(SW_CPB_HIDDEN);
    auto coord = [&](int o) {
        const double t = 8.0 * o / (double)(pw - 1);
        return (t > 0 ? 1.0 : t < 0 ? -1.0 : 0.0) * std::log2(1.0 + std::fabs(t)) / 3.0;
    };
    for (int a = 0; a < n; ++a)
        for (int c = 0; c < n; ++c) {
            const double t0 = coord(a - (w - 1)), t1 = coord(c - (w - 1));
            for (int u = 0; u < SW_CPB_HIDDEN; ++u) {
                const double v = (double)B.cpb_w1[2 * u] * t0 + (double)B.cpb_w1[2 * u + 1] * t1 + (double)B.cpb_b1[u];
                hid[u] = v > 0.0 ? v : 0.0;
            }
            for (int hh = 0; hh < heads; ++hh) {
                const float* w2 = B.cpb_w2.data() + (size_t)hh * SW_CPB_HIDDEN;
                double acc = 0.0;
                for (int u = 0; u < SW_CPB_HIDDEN; ++u) acc += (double)w2[u] * hid[u];
                out[(size_t)hh * n * n + a * n + c] = (float)(16.0 / (1.0 + std::exp(-acc)));
            }
        }
    return out;
}

int sw_prepare_cpb(hipts_swinv2* h) {
    if (h->cpb_ready) return HIPTS_OK;
    const int pw_cfg = h->cfg.cpb_pretrained_window;
    for (SwStage& St : h->st)
        for (SwBlock& B : St.blocks) {
            const std::vector<float> t = sw_cpb_table(B, St.win, pw_cfg > 0 ? pw_cfg : St.win, St.heads);
            HIPTS_TRY(upload_f32(B.cpb, t.data(), t.size()));
        }
    h->cpb_ready = true;
    return HIPTS_OK;
}

// The kernel sequence for images [i0, i0 + batch) on stream s.  stop_stage >= 0 (debug entry): return after that stage's last block,
// x holding its residual stream.
int sw_run_images(hipts_swinv2* h, const void* in_dev, bool is_u8, int i0, int batch, float* lg, float* pr, hipStream_t s, bool shared_chip,
                  int stop_stage) {
    const auto& c = h->cfg;
    const int S = c.image_size;
    const bool f16 = (c.operand_f16 & 1) != 0;
    const size_t img_bytes = (size_t)S * S * 3 * (is_u8 ? 1 : 4);
    in_dev = (const char*)in_dev + (size_t)i0 * img_bytes;
    float* x = h->x.as<float>() + (size_t)i0 * h->px;
    bf16_t* xh = h->xh.as<bf16_t>() + (size_t)i0 * h->px;
    bf16_t* xh2 = h->xh2.as<bf16_t>() + (size_t)i0 * 2 * h->px;
    float* qkv = h->qkv.as<float>() + (size_t)i0 * h->p3c;
    bf16_t* ao = h->ao.as<bf16_t>() + (size_t)i0 * h->px;
    float* br = h->br.as<float>() + (size_t)i0 * h->px;
    bf16_t* m1 = h->m1.as<bf16_t>() + (size_t)i0 * h->phid;
    bf16_t* col = h->col.as<bf16_t>() + (size_t)i0 * h->pcol;
    bf16_t* a0 = h->a0.as<bf16_t>() + (size_t)i0 * h->st[0].T * CNX_STEM_K;

    // ---- stem: conv 4x4 s4 (+bias) -> LayerNorm (weight, bias) = the residual stream of stage 0
    {
        const SwStage& S0 = h->st[0];
        const int64_t M = (int64_t)batch * S0.T;
        const int blocks = ceil_div(M * 4, 256);
        const PixelU8Table from_u8{(const uint8_t*)in_dev, h->lut.as<float>()};
        const PixelF32Planes<true> from_f32{(const float*)in_dev};
        HIPTS_LAUNCH_U8_F16(is_u8, f16, patch_gather_kernel, blocks, 256, 0, s, from_u8, from_f32, Window4x4{}, a0, M * 4, S, S0.H);
        GemmArgs g = gemm_args(f16, shared_chip);
        g.A = a0; g.W = h->stem_w.as<bf16_t>(); g.M = (int)M; g.N = S0.C; g.K = CNX_STEM_K;
        g.bias = h->stem_b.as<float>(); g.out_f32 = x;
        HIPTS_TRY(launch_gemm(EPI_BIAS, g, s));
        const LnGammaBeta norm{h->stem_nw.as<float>(), h->stem_nb.as<float>()};
        HIPTS_LAUNCH_F16(f16, row_ln_kernel, ceil_div(M, 4), 256, 0, s, FromF32{x}, norm, ToF32And16{x, xh}, M, S0.C, c.ln_eps);
        HIPTS_TRY(launch_sw_split_x(f16, x, xh2, M, S0.C, s));
    }

    for (int si = 0; si < 4; ++si) {
        SwStage& St = h->st[si];
        const int C = St.C, H = St.H;
        const int M = batch * St.T;
        if (si > 0) {
            // patch merging: 2x2 gather -> reduction GEMM -> LayerNorm (weight, bias) in place, with the 16-bit copy
            const SwStage& Pv = h->st[si - 1];
            HIPTS_TRY(launch_sw_merge(f16, x, col, M, Pv.H, Pv.C, s));
            GemmArgs g = gemm_args(f16, shared_chip);
            g.A = col; g.W = St.ds_w.as<bf16_t>(); g.M = M; g.N = C; g.K = 8 * Pv.C;
            g.bias = St.ds_b.as<float>(); g.out_f32 = x;
            HIPTS_TRY(launch_gemm(EPI_BIAS, g, s));
            const LnGammaBeta norm{St.ds_nw.as<float>(), St.ds_nb.as<float>()};
            HIPTS_LAUNCH_F16(f16, row_ln_kernel, ceil_div(M, 4), 256, 0, s, FromF32{x}, norm, ToF32And16{x, xh}, (int64_t)M, C, c.ln_eps);
            HIPTS_TRY(launch_sw_split_x(f16, x, xh2, M, C, s));
        }
        const AddToStreamHiLo to_stream{x, xh2, xh2 + C};       // x += LN(branch); xh2 = [hi | lo] of the new x
        for (SwBlock& B : St.blocks) {
            GemmArgs g = gemm_args(f16, shared_chip);
            g.A = xh2; g.W = B.qkv2.as<bf16_t>(); g.M = M; g.N = 3 * C; g.K = 2 * C; g.bias = B.qkv_b.as<float>(); g.out_f32 = qkv;
            HIPTS_TRY(launch_gemm(EPI_BIAS, g, s));
            HIPTS_TRY(launch_swin_attention(qkv, B.ls.as<float>(), B.cpb.as<float>(), ao, batch, H, St.win, B.shift, St.heads, f16, s));
            g = gemm_args(f16, shared_chip);
            g.A = ao; g.W = B.proj.as<bf16_t>(); g.M = M; g.N = C; g.K = C; g.bias = B.proj_b.as<float>(); g.out_f32 = br;
            HIPTS_TRY(launch_gemm(EPI_BIAS, g, s));
            const LnGammaBeta norm1{B.n1_w.as<float>(), B.n1_b.as<float>()};
            HIPTS_LAUNCH_F16(f16, row_ln_kernel, ceil_div(M, 4), 256, 0, s, FromF32{br}, norm1, to_stream, (int64_t)M, C, c.ln_eps);
            g = gemm_args(f16, shared_chip);
            g.A = xh2; g.W = B.fc1.as<bf16_t>(); g.M = M; g.N = St.hid; g.K = 2 * C; g.bias = B.fc1_b.as<float>();
            g.out_bf16 = m1; g.gelu_tanh = c.gelu_tanh;
            HIPTS_TRY(launch_gemm(EPI_GELU, g, s));
            g = gemm_args(f16, shared_chip);
            g.A = m1; g.W = B.fc2.as<bf16_t>(); g.M = M; g.N = C; g.K = St.hid; g.bias = B.fc2_b.as<float>(); g.out_f32 = br;
            HIPTS_TRY(launch_gemm(EPI_BIAS, g, s));
            const LnGammaBeta norm2{B.n2_w.as<float>(), B.n2_b.as<float>()};
            HIPTS_LAUNCH_F16(f16, row_ln_kernel, ceil_div(M, 4), 256, 0, s, FromF32{br}, norm2, to_stream, (int64_t)M, C, c.ln_eps);
        }
        if (si == stop_stage) return HIPTS_OK;
    }
    // ---- head: LayerNorm per token -> mean over tokens -> hi | lo -> fc (+bias) with sigmoid
    const SwStage& L = h->st[3];
    const int64_t ML = (int64_t)batch * L.T;
    bf16_t* feat2 = h->feat2.as<bf16_t>() + (size_t)i0 * 2 * L.C;
    const LnGammaBeta head_norm{h->head_nw.as<float>(), h->head_nb.as<float>()};
    row_ln_kernel<false><<<ceil_div(ML, 4), 256, 0, s>>>(FromF32{x}, head_norm, ToF32{br}, ML, L.C, c.ln_eps);
    HIPTS_LAUNCH_CHECK();
    HIPTS_TRY(launch_sw_mean(f16, br, feat2, batch, L.T, L.C, s));
    GemmArgs g = gemm_args(f16, shared_chip);
    g.A = feat2; g.W = h->head_w.as<bf16_t>(); g.M = batch; g.N = c.num_classes; g.K = 2 * L.C;
    g.bias = h->head_b.as<float>(); g.out_f32 = lg ? lg + (size_t)i0 * c.num_classes : nullptr;
    g.out2_f32 = pr ? pr + (size_t)i0 * c.num_classes : nullptr;
    HIPTS_TRY(launch_gemm(EPI_HEAD, g, s));
    return HIPTS_OK;
}

int sw_forward_impl(hipts_swinv2* h, const void* input, int in_memspace, bool is_u8, int batch, float* logits_out, float* probs_out,
                    int out_memspace, hipStream_t s, int stop_stage = -1) {
    HIPTS_REQUIRE(h && input && batch >= 1, "hipts_swinv2_forward: bad arguments");
    HIPTS_REQUIRE(batch <= h->cfg.max_batch, "batch %d exceeds max_batch %d", batch, h->cfg.max_batch);
    HIPTS_TRY(h->ledger.require_complete("hipts_swinv2_forward"));
    HIPTS_TRY(use_device(h->device));
    HIPTS_TRY(sw_prepare_cpb(h));
    const auto& c = h->cfg;
    const int S = c.image_size, NC = c.num_classes;
    const void* in_dev = nullptr;
    HIPTS_TRY(stage_input(h->img_in, input, in_memspace, (size_t)batch * S * S * 3 * (is_u8 ? 1 : 4), s, &in_dev));
    const bool dev_out = out_memspace == HIPTS_DEVICE;
    // deliberate: an output the caller does not ask for stays null and EPI_HEAD skips it (the ViT / EVA02 forwards always compute logits)
    float* lg = dev_out ? logits_out : (logits_out ? h->logits.as<float>() : nullptr);
    float* pr = dev_out ? probs_out : (probs_out ? h->probs.as<float>() : nullptr);
    // Two sub-batches on two internal streams from 32 images on (as the other forwards); the split changes which images share a
    // launch, never an image's arithmetic.
    // The debug entry (stop_stage >= 0) never splits and reads nothing back: its caller copies the residual stream itself.
    const int ns = (stop_stage < 0 && batch >= 32) ? 2 : 1;
    HIPTS_TRY(run_split(h->streams, s, batch, ns, [&](int i0, int nb, hipStream_t st, bool shared_chip, int) {
        return sw_run_images(h, in_dev, is_u8, i0, nb, lg, pr, st, shared_chip, stop_stage);
    }));
    if (stop_stage < 0 && !dev_out) HIPTS_TRY(read_back(s, (size_t)batch * NC * 4, logits_out, lg, probs_out, pr));
    return HIPTS_OK;
}

}  // namespace

extern "C" {

int hipts_swinv2_create(const hipts_swinv2_config_t* cfg, int device, hipts_swinv2_t** out) {
    HIPTS_REQUIRE(cfg && out, "hipts_swinv2_create: null argument");
    HIPTS_REQUIRE(cfg->patch == 4, "patch = %d: only 4 is built", cfg->patch);
    HIPTS_REQUIRE(cfg->image_size >= 32 && cfg->image_size % 32 == 0, "image_size %d must be a positive multiple of 32", cfg->image_size);
    HIPTS_REQUIRE(cfg->max_batch >= 1, "max_batch must be >= 1");
    HIPTS_REQUIRE(cfg->num_classes >= 1, "num_classes must be >= 1");
    HIPTS_REQUIRE(cfg->operand_f16 == 0 || cfg->operand_f16 == 1, "operand_f16 = %d: 0 (bf16) or 1 (IEEE half)", cfg->operand_f16);
    HIPTS_REQUIRE(cfg->ln_eps > 0.f, "ln_eps must be positive");
    HIPTS_REQUIRE(cfg->gelu_tanh == 0 || cfg->gelu_tanh == 1, "gelu_tanh = %d: 0 (erf) or 1 (tanh)", cfg->gelu_tanh);
    HIPTS_REQUIRE(cfg->mlp_ratio >= 1 && cfg->mlp_ratio <= 16, "mlp_ratio = %d must be in [1, 16]", cfg->mlp_ratio);
    HIPTS_REQUIRE(cfg->cpb_pretrained_window == 0 || cfg->cpb_pretrained_window >= 2, "cpb_pretrained_window = %d: 0 or >= 2",
                  cfg->cpb_pretrained_window);
    HIPTS_REQUIRE(cfg->window >= 2, "window = %d must be >= 2", cfg->window);
    for (int i = 0; i < 3; ++i)
        HIPTS_REQUIRE(cfg->norm_std[i] > 0.f && std::isfinite(cfg->norm_std[i]) && std::isfinite(cfg->norm_mean[i]), "norm_std[%d] must be positive", i);
    int H = cfg->image_size / 4;
    for (int s = 0; s < 4; ++s, H /= 2) {
        HIPTS_REQUIRE(cfg->dims[s] >= 64 && cfg->dims[s] % 64 == 0 && cfg->dims[s] <= 1024, "dims[%d] = %d must be a multiple of 64, at most 1024",
                      s, cfg->dims[s]);
        HIPTS_REQUIRE(cfg->heads[s] >= 1 && cfg->dims[s] == 32 * cfg->heads[s], "stage %d: dims %d / heads %d: head_dim must be 32", s,
                      cfg->dims[s], cfg->heads[s]);
        HIPTS_REQUIRE(cfg->depths[s] >= 1, "depths[%d] must be >= 1", s);
        const int w = std::min(H, cfg->window);
        HIPTS_REQUIRE(w >= 2 && H % w == 0, "stage %d: window %d does not divide the side %d", s, w, H);
        HIPTS_REQUIRE(w * w <= 256, "stage %d: window %d has %d tokens (at most 256)", s, w, w * w);
    }
    HIPTS_TRY(use_device(device));
    auto* h = new hipts_swinv2();
    h->device = device;
    h->cfg = *cfg;
    const int B = cfg->max_batch;
    double flops = 0.0;
    H = cfg->image_size / 4;
    flops += 2.0 * H * H * cfg->dims[0] * 48.0;
    for (int s = 0; s < 4; ++s) {
        SwStage& St = h->st[s];
        if (s > 0) H /= 2;
        St.C = cfg->dims[s];
        St.H = H;
        St.T = H * H;
        St.heads = cfg->heads[s];
        St.win = std::min(H, cfg->window);
        St.hid = cfg->mlp_ratio * St.C;
        St.blocks.resize(cfg->depths[s]);
        for (int j = 0; j < cfg->depths[s]; ++j) St.blocks[j].shift = (j % 2 == 1 && H > cfg->window) ? cfg->window / 2 : 0;
        const double T = St.T, C = St.C;
        if (s > 0) {
            flops += 2.0 * T * C * 4.0 * cfg->dims[s - 1];
            h->pcol = std::max(h->pcol, (size_t)St.T * 8 * cfg->dims[s - 1]);
        }
        // q | k | v, proj, fc1, fc2; Q K^T and P V over the window's tokens
        flops += cfg->depths[s] * (2.0 * T * C * (3.0 * C + C + 2.0 * St.hid) + 4.0 * T * (double)(St.win * St.win) * C);
        h->px = std::max(h->px, (size_t)St.T * St.C);
        h->p3c = std::max(h->p3c, (size_t)St.T * 3 * St.C);
        h->phid = std::max(h->phid, (size_t)St.T * St.hid);
    }
    flops += 2.0 * cfg->dims[3] * (double)cfg->num_classes;
    h->flops_per_image = flops;
    const int C3 = cfg->dims[3];
    const std::vector<float> lut = norm_lut(cfg->norm_mean, cfg->norm_std);
    int st = 0;
    if ((st = upload_f32(h->lut, lut.data(), lut.size())) || (st = h->a0.alloc((size_t)B * h->st[0].T * CNX_STEM_K * 2)) ||
        (st = h->x.alloc((size_t)B * h->px * 4)) || (st = h->xh.alloc((size_t)B * h->px * 2)) || (st = h->xh2.alloc((size_t)B * h->px * 4)) || (st = h->qkv.alloc((size_t)B * h->p3c * 4)) ||
        (st = h->ao.alloc((size_t)B * h->px * 2)) || (st = h->br.alloc((size_t)B * h->px * 4)) || (st = h->m1.alloc((size_t)B * h->phid * 2)) ||
        (st = h->col.alloc((size_t)B * h->pcol * 2)) || (st = h->feat2.alloc((size_t)B * 2 * C3 * 2)) ||
        (st = h->logits.alloc((size_t)B * cfg->num_classes * 4)) || (st = h->probs.alloc((size_t)B * cfg->num_classes * 4))) {
        delete h;
        return st;
    }
    for (int s = 1; s < 4; ++s) {
        const std::vector<float> zero(h->st[s].C, 0.f);
        if ((st = upload_f32(h->st[s].ds_b, zero.data(), zero.size()))) {
            delete h;
            return st;
        }
    }
    auto need = [&](const std::string& k) { h->ledger.need(k); };
    need("patch_embed.proj.weight"); need("patch_embed.proj.bias"); need("patch_embed.norm.weight"); need("patch_embed.norm.bias");
    for (int s = 0; s < 4; ++s) {
        const std::string sp = "layers." + std::to_string(s) + ".";
        if (s > 0) {
            need(sp + "downsample.reduction.weight"); need(sp + "downsample.norm.weight"); need(sp + "downsample.norm.bias");
        }
        for (int i = 0; i < cfg->depths[s]; ++i) {
            const std::string p = sp + "blocks." + std::to_string(i) + ".";
            for (const char* k : {"attn.qkv.weight", "attn.q_bias", "attn.v_bias", "attn.logit_scale", "attn.cpb_mlp.0.weight", "attn.cpb_mlp.0.bias",
                                  "attn.cpb_mlp.2.weight", "attn.proj.weight", "attn.proj.bias", "norm1.weight", "norm1.bias", "mlp.fc1.weight",
                                  "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias", "norm2.weight", "norm2.bias"})
                need(p + k);
        }
    }
    need("norm.weight"); need("norm.bias"); need("head.fc.weight"); need("head.fc.bias");
    *out = h;
    return HIPTS_OK;
}

int hipts_swinv2_destroy(hipts_swinv2_t* h) {
    if (h) {
        (void)hipSetDevice(h->device);
        (void)hipDeviceSynchronize();
        delete h;
    }
    return HIPTS_OK;
}

int hipts_swinv2_set_tensor(hipts_swinv2_t* h, const char* key_c, const float* data, int64_t numel) {
    HIPTS_REQUIRE(h && key_c && data, "hipts_swinv2_set_tensor: null argument");
    HIPTS_TRY(use_device(h->device));
    const std::string key(key_c);
    const auto& cf = h->cfg;
    const bool f16 = (cf.operand_f16 & 1) != 0;
    int st = HIPTS_OK;
    const int C0 = cf.dims[0], C3 = cf.dims[3], NC = cf.num_classes;
    int s = 0, bi = 0;
    std::string sub, t;
    if (key == "patch_embed.proj.weight") {
        EXPECT_NUMEL((int64_t)C0 * 48);
        const std::vector<float> w2 = stem_weight_hilo(data, C0, 16, CNX_STEM_KH, true);      // BGR; the hi | lo halves of patch_gather_kernel
        st = upload_matrix16(h->stem_w, w2.data(), C0, CNX_STEM_K, round_up(C0, 256), f16);
    } else if (key == "patch_embed.proj.bias") { EXPECT_NUMEL(C0); st = upload_f32(h->stem_b, data, C0); }
    else if (key == "patch_embed.norm.weight") { EXPECT_NUMEL(C0); st = upload_f32(h->stem_nw, data, C0); }
    else if (key == "patch_embed.norm.bias") { EXPECT_NUMEL(C0); st = upload_f32(h->stem_nb, data, C0); }
    else if (key == "norm.weight") { EXPECT_NUMEL(C3); st = upload_f32(h->head_nw, data, C3); }
    else if (key == "norm.bias") { EXPECT_NUMEL(C3); st = upload_f32(h->head_nb, data, C3); }
    else if (key == "head.fc.bias") { EXPECT_NUMEL(NC); st = upload_f32(h->head_b, data, NC); }
    else if (key == "head.fc.weight") {
        EXPECT_NUMEL((int64_t)NC * C3);
        st = upload_matrix16_dup(h->head_w, data, NC, C3, round_up(NC, 256), f16);
    } else if (parse_indexed(key, "layers.", &s, &sub)) {
        if (s < 0 || s > 3) return set_error(HIPTS_ERR_INVALID, "tensor %s: stage out of range", key_c);
        SwStage& St = h->st[s];
        const int C = St.C;
        if (sub.rfind("downsample.", 0) == 0) {
            if (s == 0) return set_error(HIPTS_ERR_INVALID, "tensor %s: stage 0 has no downsample", key_c);
            const int Cp = cf.dims[s - 1];
            if (sub == "downsample.norm.weight") { EXPECT_NUMEL(C); st = upload_f32(St.ds_nw, data, C); }
            else if (sub == "downsample.norm.bias") { EXPECT_NUMEL(C); st = upload_f32(St.ds_nb, data, C); }
            else if (sub == "downsample.reduction.weight") {
                EXPECT_NUMEL((int64_t)C * 4 * Cp);            // columns in timm's (dx, dy, c) order: the order sw_merge_kernel writes; [W | W]
                st = upload_matrix16_dup(St.ds_w, data, C, 4 * Cp, round_up(C, 256), f16);
            } else return set_error(HIPTS_ERR_INVALID, "unknown tensor key %s", key_c);
        } else if (parse_indexed(sub, "blocks.", &bi, &t)) {
            if (bi < 0 || bi >= (int)St.blocks.size()) return set_error(HIPTS_ERR_INVALID, "tensor %s: block out of range", key_c);
            SwBlock& B = St.blocks[bi];
            const int nh = St.heads;
            if (t == "attn.qkv.weight") {
                EXPECT_NUMEL((int64_t)3 * C * C);
                st = upload_matrix16_dup(B.qkv2, data, 3 * C, C, round_up(3 * C, 256), f16);       // against [hi | lo] of x: [W | W]
            }
            else if (t == "attn.q_bias" || t == "attn.v_bias") {
                EXPECT_NUMEL(C);
                if (B.qkv_bh.empty()) B.qkv_bh.assign((size_t)3 * C, 0.f);        // [q_bias | 0 | v_bias]: timm's k bias is a zero buffer
                std::copy(data, data + C, B.qkv_bh.begin() + (t == "attn.q_bias" ? 0 : 2 * C));
                st = upload_f32(B.qkv_b, B.qkv_bh.data(), B.qkv_bh.size());
            }
            else if (t == "attn.logit_scale") { EXPECT_NUMEL(nh); st = upload_f32(B.ls, data, nh); }
            else if (t == "attn.cpb_mlp.0.weight") { EXPECT_NUMEL(2 * SW_CPB_HIDDEN); B.cpb_w1.assign(data, data + 2 * SW_CPB_HIDDEN); h->cpb_ready = false; }
            else if (t == "attn.cpb_mlp.0.bias") { EXPECT_NUMEL(SW_CPB_HIDDEN); B.cpb_b1.assign(data, data + SW_CPB_HIDDEN); h->cpb_ready = false; }
            else if (t == "attn.cpb_mlp.2.weight") {
                EXPECT_NUMEL((int64_t)nh * SW_CPB_HIDDEN);
                B.cpb_w2.assign(data, data + (size_t)nh * SW_CPB_HIDDEN);
                h->cpb_ready = false;
            }
            else if (t == "attn.proj.weight") { EXPECT_NUMEL((int64_t)C * C); st = upload_matrix16(B.proj, data, C, C, round_up(C, 256), f16); }
            else if (t == "attn.proj.bias") { EXPECT_NUMEL(C); st = upload_f32(B.proj_b, data, C); }
            else if (t == "norm1.weight") { EXPECT_NUMEL(C); st = upload_f32(B.n1_w, data, C); }
            else if (t == "norm1.bias") { EXPECT_NUMEL(C); st = upload_f32(B.n1_b, data, C); }
            else if (t == "norm2.weight") { EXPECT_NUMEL(C); st = upload_f32(B.n2_w, data, C); }
            else if (t == "norm2.bias") { EXPECT_NUMEL(C); st = upload_f32(B.n2_b, data, C); }
            else if (t == "mlp.fc1.weight") {
                EXPECT_NUMEL((int64_t)St.hid * C);
                st = upload_matrix16_dup(B.fc1, data, St.hid, C, round_up(St.hid, 256), f16);      // against [hi | lo] of x: [W | W]
            }
            else if (t == "mlp.fc1.bias") { EXPECT_NUMEL(St.hid); st = upload_f32(B.fc1_b, data, St.hid); }
            else if (t == "mlp.fc2.weight") { EXPECT_NUMEL((int64_t)St.hid * C); st = upload_matrix16(B.fc2, data, C, St.hid, round_up(C, 256), f16); }
            else if (t == "mlp.fc2.bias") { EXPECT_NUMEL(C); st = upload_f32(B.fc2_b, data, C); }
            else return set_error(HIPTS_ERR_INVALID, "unknown tensor key %s", key_c);
        } else return set_error(HIPTS_ERR_INVALID, "unknown tensor key %s", key_c);
    } else return set_error(HIPTS_ERR_INVALID, "unknown tensor key %s", key_c);
    if (st) return st;
    h->ledger.mark_set(key);
    return HIPTS_OK;
}

int hipts_swinv2_forward_u8(hipts_swinv2_t* h, const uint8_t* images, int images_memspace, int batch, float* logits_out, float* probs_out,
                            int out_memspace, void* stream) {
    return sw_forward_impl(h, images, images_memspace, true, batch, logits_out, probs_out, out_memspace, (hipStream_t)stream);
}

int hipts_swinv2_forward_f32(hipts_swinv2_t* h, const float* x, int x_memspace, int batch, float* logits_out, float* probs_out,
                             int out_memspace, void* stream) {
    return sw_forward_impl(h, x, x_memspace, false, batch, logits_out, probs_out, out_memspace, (hipStream_t)stream);
}

int hipts_swinv2_flops_per_image(const hipts_swinv2_t* h, double* flops) {
    HIPTS_REQUIRE(h && flops, "null argument");
    *flops = h->flops_per_image;
    return HIPTS_OK;
}

// Debug / test entry (include/hip_tagsearch_debug.h): the float32 residual stream [batch][H*H][dims[stage]] after the last block of
// `stage`, from host float32 input (the layout of hipts_swinv2_forward_f32).
int hiptsdbg_swinv2_stream(hipts_swinv2_t* h, const float* x_host, int batch, int stage, float* out_host) {
    HIPTS_REQUIRE(h && x_host && out_host && stage >= 0 && stage <= 3, "hiptsdbg_swinv2_stream: bad argument");
    HIPTS_TRY(sw_forward_impl(h, x_host, HIPTS_HOST, false, batch, nullptr, nullptr, HIPTS_HOST, nullptr, stage));
    HIPTS_HIP(hipDeviceSynchronize());
    HIPTS_HIP(hipMemcpy(out_host, h->x.p, (size_t)batch * h->st[stage].T * h->st[stage].C * 4, hipMemcpyDeviceToHost));
    return HIPTS_OK;
}

// Debug / test entry: the window attention kernel alone (include/hip_tagsearch_debug.h).
int hiptsdbg_swinv2_window_attention(const float* q, const float* k, const float* v, const float* logit_scale, const float* cpb, int batch,
                                     int heads, int side, int window, int shift, int operand_f16, float* out) {
    HIPTS_REQUIRE(q && k && v && logit_scale && cpb && out && batch >= 1 && heads >= 1 && side >= 1, "hiptsdbg_swinv2_window_attention: bad argument");
    HIPTS_REQUIRE(operand_f16 == 0 || operand_f16 == 1, "operand_f16 must be 0 or 1");
    HIPTS_REQUIRE(window >= 2 && window <= 16, "window %d out of range", window);
    const int C = 32 * heads;
    const size_t M = (size_t)batch * side * side, nb = (size_t)(2 * window - 1) * (2 * window - 1);
    std::vector<float> packed(M * 3 * C);
    for (size_t m = 0; m < M; ++m) {
        std::copy(q + m * C, q + (m + 1) * C, packed.begin() + m * 3 * C);
        std::copy(k + m * C, k + (m + 1) * C, packed.begin() + m * 3 * C + C);
        std::copy(v + m * C, v + (m + 1) * C, packed.begin() + m * 3 * C + 2 * C);
    }
    DevBuf dqkv, dls, dcpb, dout;
    HIPTS_TRY(upload_f32(dqkv, packed.data(), packed.size()));
    HIPTS_TRY(upload_f32(dls, logit_scale, heads));
    HIPTS_TRY(upload_f32(dcpb, cpb, (size_t)heads * nb));
    HIPTS_TRY(dout.alloc(M * C * 2));
    HIPTS_TRY(launch_swin_attention(dqkv.as<float>(), dls.as<float>(), dcpb.as<float>(), dout.as<bf16_t>(), batch, side, window, shift, heads,
                                    operand_f16 == 1, nullptr));
    HIPTS_HIP(hipDeviceSynchronize());
    std::vector<uint16_t> o16(M * C);
    HIPTS_HIP(hipMemcpy(o16.data(), dout.p, M * C * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < M * C; ++i) {
        if (operand_f16 == 1) out[i] = f16_bits_to_f32(o16[i]);
        else { const uint32_t bits = (uint32_t)o16[i] << 16; memcpy(&out[i], &bits, 4); }
    }
    return HIPTS_OK;
}

// Debug / test entries (tests/test_gpu_tokens.py): sw_merge_kernel, sw_split_x_kernel and sw_mean_kernel once each, launched as the
// forward launches them, the output filled with `fill` before and copied back whole.
int hiptsdbg_swinv2_merge(const float* x, uint64_t x_bytes, int batch, int H, int C, int f16, int fill, uint16_t* col, uint64_t col_bytes) {
    const char* who = "hiptsdbg_swinv2_merge";
    HIPTS_REQUIRE(x && col, "%s: null argument", who);
    HIPTS_REQUIRE(batch >= 1 && batch <= 4096 && H >= 2 && H <= 1024 && H % 2 == 0, "%s: H=%d must be even (batch %d)", who, H, batch);
    HIPTS_REQUIRE(C >= 4 && C % 4 == 0 && C <= 4096, "%s: C=%d must be a multiple of 4", who, C);
    HIPTS_REQUIRE(x_bytes >= (uint64_t)batch * H * H * C * 4, "%s: x does not cover the launch", who);
    HIPTS_TRY(use_device(0));
    const int64_t rows_out = (int64_t)batch * (H / 2) * (H / 2);
    DevBuf xd, cd;
    HIPTS_TRY(dbg_guarded(cd, col_bytes, (uint64_t)rows_out * 8 * C * 2, fill, who, "col"));
    HIPTS_TRY(dbg_put(xd, x, x_bytes));
    HIPTS_TRY(launch_sw_merge(f16 != 0, xd.as<float>(), cd.as<bf16_t>(), rows_out, H, C, nullptr));
    HIPTS_HIP(hipDeviceSynchronize());
    return dbg_fetch(col, cd, col_bytes, who);
}

int hiptsdbg_swinv2_split_x(const float* x, uint64_t x_bytes, int64_t rows, int D, int f16, int fill, uint16_t* xh2, uint64_t xh2_bytes) {
    const char* who = "hiptsdbg_swinv2_split_x";
    HIPTS_REQUIRE(x && xh2, "%s: null argument", who);
    HIPTS_REQUIRE(rows >= 1 && rows <= (1 << 22) && D >= 4 && D % 4 == 0 && D <= 4096, "%s: rows=%lld, D=%d (a multiple of 4)", who, (long long)rows, D);
    HIPTS_REQUIRE(x_bytes >= (uint64_t)rows * D * 4, "%s: x does not cover the launch", who);
    HIPTS_TRY(use_device(0));
    DevBuf xd, hd;
    HIPTS_TRY(dbg_guarded(hd, xh2_bytes, (uint64_t)rows * 2 * D * 2, fill, who, "hi | lo"));
    HIPTS_TRY(dbg_put(xd, x, x_bytes));
    HIPTS_TRY(launch_sw_split_x(f16 != 0, xd.as<float>(), hd.as<bf16_t>(), rows, D, nullptr));
    HIPTS_HIP(hipDeviceSynchronize());
    return dbg_fetch(xh2, hd, xh2_bytes, who);
}

int hiptsdbg_swinv2_mean(const float* y, uint64_t y_bytes, int batch, int T, int C, int f16, int fill, uint16_t* out, uint64_t out_bytes) {
    const char* who = "hiptsdbg_swinv2_mean";
    HIPTS_REQUIRE(y && out, "%s: null argument", who);
    HIPTS_REQUIRE(batch >= 1 && batch <= 4096 && T >= 1 && T <= (1 << 16) && C >= 1 && C <= 4096, "%s: unsupported shape", who);
    HIPTS_REQUIRE(y_bytes >= (uint64_t)batch * T * C * 4, "%s: y does not cover the launch", who);
    HIPTS_TRY(use_device(0));
    DevBuf yd, od;
    HIPTS_TRY(dbg_guarded(od, out_bytes, (uint64_t)batch * 2 * C * 2, fill, who, "hi | lo"));
    HIPTS_TRY(dbg_put(yd, y, y_bytes));
    HIPTS_TRY(launch_sw_mean(f16 != 0, yd.as<float>(), od.as<bf16_t>(), batch, T, C, nullptr));
    HIPTS_HIP(hipDeviceSynchronize());
    return dbg_fetch(out, od, out_bytes, who);
}

}  // extern "C"
