// convnext.hip -- ConvNeXt tagger forward (wd-convnext-tagger-v3 = timm `convnext_base` at 448 px) behind hipts_convnext_*.
//
// Layer algebra (timm `models/convnext.py`, conv_mlp = False, the layout of the checkpoint's keys):
//   stem      x = LN(Conv2d(3, C0, k = 4, s = 4)(img) + b)                        (channels-last LayerNorm, weight and bias)
//   stage i   (i > 0) x = Conv2d(C_{i-1}, C_i, k = 2, s = 2)(LN(x)) + b
//             blocks: x = x + gamma * fc2(GELU_erf(fc1(LN(dwconv7x7(x) + b_dw))))
//   head      logits = fc(LN(mean over tokens of x)), probs = sigmoid(logits)
//
// Data layout as in the CCIP encoder (ccip.hip): token-major NHWC, the residual stream x float32 [B*H*W][C] (row-major), GEMM
// operands 16-bit (bf16, or IEEE half with operand_f16 bit 0).  Every 1 x 1 convolution / Linear is the shared persistent MFMA
// GEMM (gemm.hip) with a fused epilogue:
//   stem 4x4 s4      patch gather (hi | lo halves against [W | W], K = 2 x 64)  -> EPI_BIAS, then LayerNorm with bias in place
//                    (patch_rows.h: patch_gather_kernel with Window4x4; row_ln.h: row_ln_kernel, whose ToF32And16 sink also writes the
//                    16-bit copy of x the first depthwise convolution reads)
//   downsample       LayerNorm fused with the 2 x 2 s2 gather (row_ln_kernel with the ToPatch2x2 sink writes the GEMM's A matrix: every
//                    token is normalised once and lands in one row) -> EPI_BIAS, 16-bit copy
//   depthwise 7x7    convnet.h: the matrix-core kernel (half operands, side >= 16) or the VALU kernel; then row_ln_kernel with the
//                    From16Bias source adds the depthwise bias in fp32 and applies the block's LayerNorm (weight, bias) into the 16-bit
//                    operand of fc1
//   fc1              EPI_GELU with gelu_tanh = 0 (erf GELU, the epilogue's rational approximation)
//   fc2              EPI_RESID_LS: x += gamma * (acc + b2) in fp32 -- the layer scale is NOT folded into W2 (timm initialises it at
//                    1e-6, and gamma W2 rounded to half lands in the subnormal range, which the MFMA reads as zero) -- and the 16-bit
//                    copy of the new x, the next block's depthwise input
//   head             pool_ln_kernel with the PooledHiLo sink (convnet.h) -> EPI_HEAD (logits and sigmoid)
// Every kernel choice is a function of the configuration and the stage only; an image's bits do not depend on the batch or the
// sub-batch split (tests/test_gpu_convnext.py).
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

struct CnxBlock {
    DevBuf dw;                     // depthwise weights as [49][C] float32 (VALU kernel)
    DevBuf dwz;                    // ... and as the Toeplitz lane images of dwconv7_mfma_kernel (half operands only)
    DevBuf dw_b, n_w, n_b;         // depthwise bias, LayerNorm weight and bias
    DevBuf fc1, fc1_b, fc2, fc2_b; // [4C][C], [4C], [C][4C], [C]
    DevBuf gamma;                  // layer scale [C], applied in fp32 by the fc2 epilogue
};

struct CnxStage {
    int C = 0, H = 0, T = 0;
    DevBuf ds_nw, ds_nb, ds_w, ds_b;       // downsample (stage > 0): LN weight / bias [Cprev], conv as [C][4 Cprev] ((ky, kx, c) order), bias [C]
    std::vector<CnxBlock> blocks;
};

}  // namespace

struct hipts_convnext {
    int device = 0;
    hipts_convnext_config_t cfg{};
    CnxStage st[4];
    DevBuf stem_w, stem_b, stem_nw, stem_nb, head_nw, head_nb, head_w, head_b, lut;
    TensorLedger ledger;
    // workspace (sized for cfg.max_batch), carved per image with the stride of the largest stage
    DevBuf img_in, a0, x, xh, dwo, xn, m1, col, feat2, logits, probs;
    size_t px = 0, p4c = 0, pcol = 0;
    SubStreams<2> streams;
    double flops_per_image = 0.0;
};

namespace {


// 16-bit copy of the fp32 stream (behind the downsample GEMM, whose EPI_BIAS epilogue writes fp32 only).  One thread per float4.
template <bool F16>
__global__ __launch_bounds__(256) void cnx_cast_kernel(const float* __restrict__ x, bf16_t* __restrict__ xh, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    reinterpret_cast<bf16x4*>(xh)[i] = pack4<F16>(v.x, v.y, v.z, v.w);
}

// its launch shape, shared by the forward and hiptsdbg_convnext_cast
int launch_cnx_cast(bool f16, const float* x, bf16_t* xh, int64_t n4, hipStream_t s) {
    HIPTS_LAUNCH_F16(f16, cnx_cast_kernel, ceil_div(n4, 256), 256, 0, s, x, xh, n4);
    return HIPTS_OK;
}

// The kernel sequence for images [i0, i0 + batch) on stream s.  stop_stage >= 0 (debug entry): return after that stage's last block,
// x holding its residual stream.
int cnx_run_images(hipts_convnext* h, const void* in_dev, bool is_u8, int i0, int batch, float* lg, float* pr, hipStream_t s, bool shared_chip,
                   int stop_stage) {
    const auto& c = h->cfg;
    const int S = c.image_size;
    const bool f16 = (c.operand_f16 & 1) != 0;
    const size_t img_bytes = (size_t)S * S * 3 * (is_u8 ? 1 : 4);
    in_dev = (const char*)in_dev + (size_t)i0 * img_bytes;
    float* x = h->x.as<float>() + (size_t)i0 * h->px;
    bf16_t* xh = h->xh.as<bf16_t>() + (size_t)i0 * h->px;
    bf16_t* dwo = h->dwo.as<bf16_t>() + (size_t)i0 * h->px;
    bf16_t* xn = h->xn.as<bf16_t>() + (size_t)i0 * h->px;
    bf16_t* m1 = h->m1.as<bf16_t>() + (size_t)i0 * h->p4c;
    bf16_t* col = h->col.as<bf16_t>() + (size_t)i0 * h->pcol;
    bf16_t* a0 = h->a0.as<bf16_t>() + (size_t)i0 * h->st[0].T * CNX_STEM_K;

    // ---- stem: conv 4x4 s4 (+bias) -> LayerNorm (weight, bias) = the residual stream of stage 0
    {
        const CnxStage& S0 = h->st[0];
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
    }

    for (int si = 0; si < 4; ++si) {
        CnxStage& St = h->st[si];
        const int C = St.C, H = St.H;
        const int M = batch * St.T;
        if (si > 0) {
            // downsample: LN(x) gathered into 2x2 s2 patches -> GEMM (+bias) -> x, then its 16-bit copy
            const CnxStage& Pv = h->st[si - 1];
            const int64_t rows_in = (int64_t)batch * Pv.T;
            const LnGammaBeta norm{St.ds_nw.as<float>(), St.ds_nb.as<float>()};
            HIPTS_LAUNCH_F16(f16, row_ln_kernel, ceil_div(rows_in, 4), 256, 0, s, FromF32{x}, norm, ToPatch2x2{col, Pv.H}, rows_in, Pv.C, c.ln_eps);
            GemmArgs g = gemm_args(f16, shared_chip);
            g.A = col; g.W = St.ds_w.as<bf16_t>(); g.M = M; g.N = C; g.K = 4 * Pv.C;
            g.bias = St.ds_b.as<float>(); g.out_f32 = x;
            HIPTS_TRY(launch_gemm(EPI_BIAS, g, s));
            const int64_t n4 = (int64_t)M * C / 4;
            HIPTS_TRY(launch_cnx_cast(f16, x, xh, n4, s));
        }
        for (CnxBlock& B : St.blocks) {
            // depthwise 7x7 (no bias) of the 16-bit copy of x
            if (f16 && H >= 16) {
                HIPTS_TRY(launch_dwconv7_mfma(xh, B.dwz.as<uint32_t>(), dwo, batch, H, C, 1, s));
            } else {
                const int tiles_x = ceil_div(H, DW_TW), tiles_y = ceil_div(H, DW_TH);
                const int dw_grid = batch * tiles_y * tiles_x * (C / DW_CS);
                HIPTS_LAUNCH_F16(f16, dwconv7_kernel, dw_grid, 256, DW_LDS_BYTES, s, xh, B.dw.as<float>(), dwo, H, C, tiles_x, tiles_y);
            }
            // + depthwise bias -> LayerNorm (weight, bias) -> the 16-bit operand of fc1
            const From16Bias dw{dwo, B.dw_b.as<float>()};
            const LnGammaBeta norm{B.n_w.as<float>(), B.n_b.as<float>()};
            HIPTS_LAUNCH_F16(f16, row_ln_kernel, ceil_div(M, 4), 256, 0, s, dw, norm, To16{xn}, (int64_t)M, C, c.ln_eps);
            GemmArgs g = gemm_args(f16, shared_chip);
            g.A = xn; g.W = B.fc1.as<bf16_t>(); g.M = M; g.N = 4 * C; g.K = C; g.bias = B.fc1_b.as<float>();
            g.out_bf16 = m1; g.gelu_tanh = 0;
            HIPTS_TRY(launch_gemm(EPI_GELU, g, s));
            g = gemm_args(f16, shared_chip);
            g.A = m1; g.W = B.fc2.as<bf16_t>(); g.M = M; g.N = C; g.K = 4 * C; g.bias = B.fc2_b.as<float>();
            g.out_f32 = x; g.res_scale = B.gamma.as<float>(); g.out_bf16 = xh;
            HIPTS_TRY(launch_gemm(EPI_RESID_LS, g, s));
        }
        if (si == stop_stage) return HIPTS_OK;
    }
    // ---- head: mean over tokens -> LayerNorm (weight, bias) -> hi | lo -> fc (+bias) with sigmoid
    const CnxStage& L = h->st[3];
    bf16_t* feat2 = h->feat2.as<bf16_t>() + (size_t)i0 * 2 * L.C;
    HIPTS_LAUNCH_F16(f16, pool_ln_kernel, batch, 1024, 0, s, x, h->head_nw.as<float>(), h->head_nb.as<float>(), PooledHiLo{feat2}, L.T, L.C, c.ln_eps, 0,
                     L.T);
    GemmArgs g = gemm_args(f16, shared_chip);
    g.A = feat2; g.W = h->head_w.as<bf16_t>(); g.M = batch; g.N = c.num_classes; g.K = 2 * L.C;
    g.bias = h->head_b.as<float>(); g.out_f32 = lg ? lg + (size_t)i0 * c.num_classes : nullptr;
    g.out2_f32 = pr ? pr + (size_t)i0 * c.num_classes : nullptr;
    HIPTS_TRY(launch_gemm(EPI_HEAD, g, s));
    return HIPTS_OK;
}

int cnx_forward_impl(hipts_convnext* h, const void* input, int in_memspace, bool is_u8, int batch, float* logits_out, float* probs_out,
                     int out_memspace, hipStream_t s, int stop_stage = -1) {
    HIPTS_REQUIRE(h && input && batch >= 1, "hipts_convnext_forward: bad arguments");
    HIPTS_REQUIRE(batch <= h->cfg.max_batch, "batch %d exceeds max_batch %d", batch, h->cfg.max_batch);
    HIPTS_TRY(h->ledger.require_complete("hipts_convnext_forward"));
    HIPTS_TRY(use_device(h->device));
    const auto& c = h->cfg;
    const int S = c.image_size, NC = c.num_classes;
    const void* in_dev = nullptr;
    HIPTS_TRY(stage_input(h->img_in, input, in_memspace, (size_t)batch * S * S * 3 * (is_u8 ? 1 : 4), s, &in_dev));
    const bool dev_out = out_memspace == HIPTS_DEVICE;
    // deliberate: an output the caller does not ask for stays null and EPI_HEAD skips it (the ViT / EVA02 forwards always compute logits)
    float* lg = dev_out ? logits_out : (logits_out ? h->logits.as<float>() : nullptr);
    float* pr = dev_out ? probs_out : (probs_out ? h->probs.as<float>() : nullptr);
    // Two sub-batches on two internal streams from 32 images on (as the CCIP and ViT forwards): the late stages have fewer output
    // tiles than the chip has CUs, and a kernel of one half fills the CUs the other half leaves idle.  The split changes which images
    // share a launch, never an image's arithmetic.
    // The debug entry (stop_stage >= 0) never splits and reads nothing back: its caller copies the residual stream itself.
    const int ns = (stop_stage < 0 && batch >= 32) ? 2 : 1;
    HIPTS_TRY(run_split(h->streams, s, batch, ns, [&](int i0, int nb, hipStream_t st, bool shared_chip, int) {
        return cnx_run_images(h, in_dev, is_u8, i0, nb, lg, pr, st, shared_chip, stop_stage);
    }));
    if (stop_stage < 0 && !dev_out) HIPTS_TRY(read_back(s, (size_t)batch * NC * 4, logits_out, lg, probs_out, pr));
    return HIPTS_OK;
}

}  // namespace

extern "C" {

int hipts_convnext_create(const hipts_convnext_config_t* cfg, int device, hipts_convnext_t** out) {
    HIPTS_REQUIRE(cfg && out, "hipts_convnext_create: null argument");
    HIPTS_REQUIRE(cfg->image_size >= 32 && cfg->image_size % 32 == 0, "image_size %d must be a positive multiple of 32", cfg->image_size);
    HIPTS_REQUIRE(cfg->max_batch >= 1, "max_batch must be >= 1");
    HIPTS_REQUIRE(cfg->num_classes >= 1, "num_classes must be >= 1");
    HIPTS_REQUIRE(cfg->operand_f16 == 0 || cfg->operand_f16 == 1, "operand_f16 = %d: 0 (bf16) or 1 (IEEE half)", cfg->operand_f16);
    HIPTS_REQUIRE(cfg->ln_eps > 0.f, "ln_eps must be positive");
    for (int i = 0; i < 3; ++i)
        HIPTS_REQUIRE(cfg->norm_std[i] > 0.f && std::isfinite(cfg->norm_std[i]) && std::isfinite(cfg->norm_mean[i]), "norm_std[%d] must be positive", i);
    for (int s = 0; s < 4; ++s) {
        // multiples of 64: the GEMMs' K (fc1 reads C columns) and the depthwise kernels' 64-channel slabs
        HIPTS_REQUIRE(cfg->dims[s] >= 64 && cfg->dims[s] % 64 == 0 && cfg->dims[s] <= 1024, "dims[%d] = %d must be a multiple of 64, at most 1024",
                      s, cfg->dims[s]);
        HIPTS_REQUIRE(cfg->depths[s] >= 1, "depths[%d] must be >= 1", s);
    }
    HIPTS_TRY(use_device(device));
    auto* h = new hipts_convnext();
    h->device = device;
    h->cfg = *cfg;
    const int B = cfg->max_batch;
    double flops = 0.0;
    int H = cfg->image_size / 4;
    flops += 2.0 * H * H * cfg->dims[0] * 48.0;
    for (int s = 0; s < 4; ++s) {
        CnxStage& St = h->st[s];
        if (s > 0) H /= 2;
        St.C = cfg->dims[s];
        St.H = H;
        St.T = H * H;
        St.blocks.resize(cfg->depths[s]);
        const double T = St.T, C = St.C;
        if (s > 0) {
            flops += 2.0 * T * C * 4.0 * cfg->dims[s - 1];
            h->pcol = std::max(h->pcol, (size_t)St.T * 4 * cfg->dims[s - 1]);
        }
        flops += cfg->depths[s] * (2.0 * 49.0 * T * C + 2.0 * T * 4 * C * C * 2);
        h->px = std::max(h->px, (size_t)St.T * St.C);
        h->p4c = std::max(h->p4c, (size_t)St.T * 4 * St.C);
    }
    flops += 2.0 * cfg->dims[3] * (double)cfg->num_classes;
    h->flops_per_image = flops;
    const int C3 = cfg->dims[3];
    const std::vector<float> lut = norm_lut(cfg->norm_mean, cfg->norm_std);
    int st = 0;
    if ((st = upload_f32(h->lut, lut.data(), lut.size())) || (st = h->a0.alloc((size_t)B * h->st[0].T * CNX_STEM_K * 2)) ||
        (st = h->x.alloc((size_t)B * h->px * 4)) || (st = h->xh.alloc((size_t)B * h->px * 2)) || (st = h->dwo.alloc((size_t)B * h->px * 2)) ||
        (st = h->xn.alloc((size_t)B * h->px * 2)) || (st = h->m1.alloc((size_t)B * h->p4c * 2)) || (st = h->col.alloc((size_t)B * h->pcol * 2)) ||
        (st = h->feat2.alloc((size_t)B * 2 * C3 * 2)) ||
        (st = h->logits.alloc((size_t)B * cfg->num_classes * 4)) || (st = h->probs.alloc((size_t)B * cfg->num_classes * 4))) {
        delete h;
        return st;
    }
    hipError_t e = hipFuncSetAttribute((const void*)dwconv7_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, DW_LDS_BYTES);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)dwconv7_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, DW_LDS_BYTES);
    if (e != hipSuccess) {
        delete h;
        return set_error(HIPTS_ERR_HIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    }
    auto need = [&](const std::string& k) { h->ledger.need(k); };
    need("stem.0.weight"); need("stem.0.bias"); need("stem.1.weight"); need("stem.1.bias");
    for (int s = 0; s < 4; ++s) {
        const std::string sp = "stages." + std::to_string(s) + ".";
        if (s > 0) {
            need(sp + "downsample.0.weight"); need(sp + "downsample.0.bias");
            need(sp + "downsample.1.weight"); need(sp + "downsample.1.bias");
        }
        for (int i = 0; i < cfg->depths[s]; ++i) {
            const std::string p = sp + "blocks." + std::to_string(i) + ".";
            need(p + "conv_dw.weight"); need(p + "conv_dw.bias"); need(p + "norm.weight"); need(p + "norm.bias");
            need(p + "mlp.fc1.weight"); need(p + "mlp.fc1.bias"); need(p + "mlp.fc2.weight"); need(p + "mlp.fc2.bias"); need(p + "gamma");
        }
    }
    need("head.norm.weight"); need("head.norm.bias"); need("head.fc.weight"); need("head.fc.bias");
    *out = h;
    return HIPTS_OK;
}

int hipts_convnext_destroy(hipts_convnext_t* h) {
    if (h) {
        (void)hipSetDevice(h->device);
        (void)hipDeviceSynchronize();
        delete h;
    }
    return HIPTS_OK;
}

int hipts_convnext_set_tensor(hipts_convnext_t* h, const char* key_c, const float* data, int64_t numel) {
    HIPTS_REQUIRE(h && key_c && data, "hipts_convnext_set_tensor: null argument");
    HIPTS_TRY(use_device(h->device));
    const std::string key(key_c);
    const auto& cf = h->cfg;
    const bool f16 = (cf.operand_f16 & 1) != 0;
    int st = HIPTS_OK;
    const int C0 = cf.dims[0], C3 = cf.dims[3], NC = cf.num_classes;
    int s = 0, bi = 0;
    std::string sub, t;
    if (key == "stem.0.weight") {
        EXPECT_NUMEL((int64_t)C0 * 48);
        const std::vector<float> w2 = stem_weight_hilo(data, C0, 16, CNX_STEM_KH, true);      // BGR; the hi | lo halves of patch_gather_kernel
        st = upload_matrix16(h->stem_w, w2.data(), C0, CNX_STEM_K, round_up(C0, 256), f16);
    } else if (key == "stem.0.bias") { EXPECT_NUMEL(C0); st = upload_f32(h->stem_b, data, C0); }
    else if (key == "stem.1.weight") { EXPECT_NUMEL(C0); st = upload_f32(h->stem_nw, data, C0); }
    else if (key == "stem.1.bias") { EXPECT_NUMEL(C0); st = upload_f32(h->stem_nb, data, C0); }
    else if (key == "head.norm.weight") { EXPECT_NUMEL(C3); st = upload_f32(h->head_nw, data, C3); }
    else if (key == "head.norm.bias") { EXPECT_NUMEL(C3); st = upload_f32(h->head_nb, data, C3); }
    else if (key == "head.fc.bias") { EXPECT_NUMEL(NC); st = upload_f32(h->head_b, data, NC); }
    else if (key == "head.fc.weight") {
        EXPECT_NUMEL((int64_t)NC * C3);
        st = upload_matrix16_dup(h->head_w, data, NC, C3, round_up(NC, 256), f16);
    } else if (parse_indexed(key, "stages.", &s, &sub)) {
        if (s < 0 || s > 3) return set_error(HIPTS_ERR_INVALID, "tensor %s: stage out of range", key_c);
        CnxStage& St = h->st[s];
        const int C = St.C;
        if (sub.rfind("downsample.", 0) == 0) {
            if (s == 0) return set_error(HIPTS_ERR_INVALID, "tensor %s: stage 0 has no downsample", key_c);
            const int Cp = cf.dims[s - 1];
            if (sub == "downsample.0.weight") { EXPECT_NUMEL(Cp); st = upload_f32(St.ds_nw, data, Cp); }
            else if (sub == "downsample.0.bias") { EXPECT_NUMEL(Cp); st = upload_f32(St.ds_nb, data, Cp); }
            else if (sub == "downsample.1.bias") { EXPECT_NUMEL(C); st = upload_f32(St.ds_b, data, C); }
            else if (sub == "downsample.1.weight") {
                EXPECT_NUMEL((int64_t)C * Cp * 4);
                std::vector<float> w2((size_t)C * 4 * Cp);          // [n][c][ky][kx] -> [n][(ky*2 + kx)*Cp + c], the gather's order
                for (int n = 0; n < C; ++n)
                    for (int cc = 0; cc < Cp; ++cc)
                        for (int t = 0; t < 4; ++t) w2[((size_t)n * 4 + t) * Cp + cc] = data[((size_t)n * Cp + cc) * 4 + t];
                st = upload_matrix16(St.ds_w, w2.data(), C, 4 * Cp, round_up(C, 256), f16);
            } else return set_error(HIPTS_ERR_INVALID, "unknown tensor key %s", key_c);
        } else if (parse_indexed(sub, "blocks.", &bi, &t)) {
            if (bi < 0 || bi >= (int)St.blocks.size()) return set_error(HIPTS_ERR_INVALID, "tensor %s: block out of range", key_c);
            CnxBlock& B = St.blocks[bi];
            if (t == "conv_dw.weight") {
                EXPECT_NUMEL((int64_t)C * 49);
                std::vector<float> w2((size_t)49 * C);          // [c][tap] -> [tap][c]
                for (int cc = 0; cc < C; ++cc)
                    for (int tp = 0; tp < 49; ++tp) w2[(size_t)tp * C + cc] = data[(size_t)cc * 49 + tp];
                st = upload_f32(B.dw, w2.data(), w2.size());
                if (st == HIPTS_OK && f16) {
                    const std::vector<uint32_t> tzv = dw_toeplitz_lanes(data, C);
                    st = upload_f32(B.dwz, reinterpret_cast<const float*>(tzv.data()), tzv.size());
                }
            }
            else if (t == "conv_dw.bias") { EXPECT_NUMEL(C); st = upload_f32(B.dw_b, data, C); }
            else if (t == "norm.weight") { EXPECT_NUMEL(C); st = upload_f32(B.n_w, data, C); }
            else if (t == "norm.bias") { EXPECT_NUMEL(C); st = upload_f32(B.n_b, data, C); }
            else if (t == "gamma") { EXPECT_NUMEL(C); st = upload_f32(B.gamma, data, C); }
            else if (t == "mlp.fc1.weight") { EXPECT_NUMEL((int64_t)4 * C * C); st = upload_matrix16(B.fc1, data, 4 * C, C, round_up(4 * C, 256), f16); }
            else if (t == "mlp.fc1.bias") { EXPECT_NUMEL((int64_t)4 * C); st = upload_f32(B.fc1_b, data, (size_t)4 * C); }
            else if (t == "mlp.fc2.weight") { EXPECT_NUMEL((int64_t)4 * C * C); st = upload_matrix16(B.fc2, data, C, 4 * C, round_up(C, 256), f16); }
            else if (t == "mlp.fc2.bias") { EXPECT_NUMEL(C); st = upload_f32(B.fc2_b, data, C); }
            else return set_error(HIPTS_ERR_INVALID, "unknown tensor key %s", key_c);
        } else return set_error(HIPTS_ERR_INVALID, "unknown tensor key %s", key_c);
    } else return set_error(HIPTS_ERR_INVALID, "unknown tensor key %s", key_c);
    if (st) return st;
    h->ledger.mark_set(key);
    return HIPTS_OK;
}

int hipts_convnext_forward_u8(hipts_convnext_t* h, const uint8_t* images, int images_memspace, int batch, float* logits_out, float* probs_out,
                              int out_memspace, void* stream) {
    return cnx_forward_impl(h, images, images_memspace, true, batch, logits_out, probs_out, out_memspace, (hipStream_t)stream);
}

int hipts_convnext_forward_f32(hipts_convnext_t* h, const float* x, int x_memspace, int batch, float* logits_out, float* probs_out,
                               int out_memspace, void* stream) {
    return cnx_forward_impl(h, x, x_memspace, false, batch, logits_out, probs_out, out_memspace, (hipStream_t)stream);
}

int hipts_convnext_flops_per_image(const hipts_convnext_t* h, double* flops) {
    HIPTS_REQUIRE(h && flops, "null argument");
    *flops = h->flops_per_image;
    return HIPTS_OK;
}

// Debug / test entry (include/hip_tagsearch_debug.h): the float32 residual stream [batch][H*H][dims[stage]] after the last block of
// `stage`, from host float32 input (the layout of hipts_convnext_forward_f32) -- places a parity failure in the network.
int hiptsdbg_convnext_stream(hipts_convnext_t* h, const float* x_host, int batch, int stage, float* out_host) {
    HIPTS_REQUIRE(h && x_host && out_host && stage >= 0 && stage <= 3, "hiptsdbg_convnext_stream: bad argument");
    HIPTS_TRY(cnx_forward_impl(h, x_host, HIPTS_HOST, false, batch, nullptr, nullptr, HIPTS_HOST, nullptr, stage));
    HIPTS_HIP(hipDeviceSynchronize());
    // (one run over all the images: their rows are contiguous, [batch * H * H][C])
    HIPTS_HIP(hipMemcpy(out_host, h->x.p, (size_t)batch * h->st[stage].T * h->st[stage].C * 4, hipMemcpyDeviceToHost));
    return HIPTS_OK;
}

// Debug / test entry (tests/test_gpu_tokens.py): cnx_cast_kernel once on n4 float4, launched as the forward launches it, xh filled with
// `fill` before and copied back whole.
int hiptsdbg_convnext_cast(const float* x, uint64_t x_bytes, int64_t n4, int f16, int fill, uint16_t* xh, uint64_t xh_bytes) {
    const char* who = "hiptsdbg_convnext_cast";
    HIPTS_REQUIRE(x && xh, "%s: null argument", who);
    HIPTS_REQUIRE(n4 >= 1 && n4 <= (1 << 26), "%s: n4=%lld", who, (long long)n4);
    HIPTS_REQUIRE(x_bytes >= (uint64_t)n4 * 16, "%s: x does not cover the launch", who);
    HIPTS_TRY(use_device(0));
    DevBuf xd, hd;
    HIPTS_TRY(dbg_guarded(hd, xh_bytes, (uint64_t)n4 * 8, fill, who, "16-bit"));
    HIPTS_TRY(dbg_put(xd, x, x_bytes));
    HIPTS_TRY(launch_cnx_cast(f16 != 0, xd.as<float>(), hd.as<bf16_t>(), n4, nullptr));
    HIPTS_HIP(hipDeviceSynchronize());
    return dbg_fetch(xh, hd, xh_bytes, who);
}

}  // extern "C"
