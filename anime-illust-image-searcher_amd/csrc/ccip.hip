// ccip.hip -- CCIP character-feature encoder (gen_cfeatures.py:112-118,133-159): a CAFormer (timm
// MetaFormer) forward behind hipts_ccip_*.
//
// Reference call being replaced: `self.embed_model.run(['output'], {'input': x})` with x float32
// [B,3,384,384] (gen_cfeatures.py:158).  The ONNX graph itself is not in /root/reference; the layer
// algebra below is timm 1.0.9 `models/metaformer.py` -- see oracle/ccip.py, which
// restates the same definition on the CPU and is what the parity tests compare against.
//
// Data layout: activations are token-major NHWC throughout -- the residual stream x is float32
// [B*H*W][C], GEMM operands are bf16 [rows][K] -- so every 1x1 convolution / Linear is the same
// persistent MFMA GEMM as in the ViT (gemm.hip) with a fused epilogue:
//   pwconv1 / fc1      -> EPI_STAR     bf16(s * relu(.)^2 + b)        (StarReLU)
//   pwconv2 / fc2 / proj -> EPI_RESID / EPI_RESCALE   x = rs * x + .  (float32 read-modify-write)
//   qkv                -> EPI_QK + EPI_VT with head_dim 32 layouts, then attn.hip<HD = 32>
//   stem 7x7 s4, downsample 3x3 s2 -> im2col kernel + GEMM with EPI_BIAS
// The stem's patch matrix is stored as bf16 hi | lo halves against [W | W] (K = 2 * 160), so the
// normalised pixels enter the MFMA with 16 mantissa bits (same device as the ViT float input path).
// Memory-bound pieces are plain HIP kernels here: depthwise 7x7 (NHWC, 8 channels = 16 B per thread),
// im2col gathers, bias-free LayerNorm, pooled LayerNorm head.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "gemm_plan.h"
#include "vit_internal.h"
#include "dbg_buf.h"
#include "model_host.h"
#include "convnet.h"

using namespace hipts;

namespace {

struct Block {
    bool attn = false;
    DevBuf n1, n2;                 // LayerNorm gammas (no beta)
    DevBuf w_in, w_out;            // SepConv: pwconv1 [2C,C], pwconv2 [C,2C]; attention: qkv [3C,C], proj [C,C]
    DevBuf dw;                     // SepConv: depthwise weights as [49][2C] float32
    DevBuf dwz;                    // ... and as the lane images of their Toeplitz operands, [2C][7][64] u32 (dwconv7_mfma_kernel)
    DevBuf fc1, fc2;               // [4C,C], [C,4C]
    DevBuf mlp_img;                // the two as the chunk images of the fused MLP kernel (mlp.hip; widths 128 / 256, half operands)
    std::vector<float> fc1_host, fc2_host;      // host copies (stages 0-1: 15 MB in all): the image is rebuilt whenever either tensor is set again
    DevBuf u_qk, u_v, u_fc1;       // attention blocks of the wide stages: W gamma per output column of q | k, v (norm1) and fc1 (norm2) -- the
                                   // LayerNorm folded into the consumer GEMM (round 5; EPI_RESID_XG prepares gamma * x and the row sums)
    DevBuf rs1, rs2;               // optional res_scale vectors
    bool has_rs1 = false, has_rs2 = false;
    float s1 = 1.f, b1 = 0.f;      // token-mixer StarReLU
    float s2 = 1.f, b2 = 0.f;      // MLP StarReLU
};

struct Stage {
    int C = 0, H = 0, T = 0, Tp = 0;       // width, spatial side, tokens = H*H, padded tokens
    DevBuf ds_norm, ds_w, ds_b;            // downsample (stage > 0): LN gamma [Cprev], conv as [C][9*Cprev], bias [C]
    std::vector<Block> blocks;
};

constexpr int STEM_KH = 160;               // 7*7*3 = 147 taps padded to 160; K = hi | lo = 320
constexpr int STEM_K = 2 * STEM_KH;

}  // namespace

struct hipts_ccip {
    int device = 0;
    hipts_ccip_config_t cfg{};
    Stage st[4];
    DevBuf stem_w, stem_b, stem_norm, head_g, head_b, zeros, lut;
    TensorLedger ledger;
    // workspace (sized for cfg.max_batch)
    DevBuf img_in, a0, x, xn, h1, h2, m1, col, q, k, vT, feat;
    DevBuf stat_part, fold_c;      // folded LayerNorms of the wide stages: per (256-column tile, row) partial (sum, sum of squares); scratch for W beta (unused: no beta)
    size_t pstat = 0;              // float2 per image of stat_part (largest wide stage)
    bool fold_dirty = true;        // a norm / qkv / fc1 tensor changed since the fold vectors were computed
    size_t px = 0, p2c = 0, p4c = 0, pcol = 0, pqk = 0;   // per-image element strides of the workspace buffers (largest stage)
    static constexpr int MAX_SUB = 4;
    SubStreams<MAX_SUB> streams;
    double flops_per_image = 0.0;
};

namespace {

// ---------------------------------------------------------------------------------------------
// Stem patch matrix.  A0[m][(ky*7 + kx)*3 + c] = hi, A0[m][160 + ...] = lo of the normalised pixel at
// (4 oy - 2 + ky, 4 ox - 2 + kx), zero outside the image (Conv2d padding = 2 pads the NORMALISED input).
// The float32 entry gathers it with patch_rows.h's patch_gather_kernel (Window7x7; the planes are read in
// memory order, no BGR flip; one thread per (token, ky): 21 values; the pad columns 147..159 stay zero as allocated).
// uint8 images (NHWC RGB): /255 in float32, (x - mean) / std in float64, cast (gen_cfeatures.py:100-110,156) --
// 3 x 256 possible values, tabulated once on the host with exactly that arithmetic.
// ---------------------------------------------------------------------------------------------
static_assert(Window7x7::half() == STEM_KH, "the stem weight's half width");

// The uint8 entry point's version: a workgroup owns 64 adjacent output pixels of one output row.  It loads
// the 7 x (64*4+3) x 3 input bytes they touch with coalesced byte loads into LDS, builds the 64 patch rows
// (hi | lo halves, zero pad columns included) in LDS through the normalisation table, and writes them out
// as ONE contiguous 40 KB block with 16 B stores (consecutive pixels are consecutive rows of A0).  The
// one-thread-per-kernel-row gather spends its time on scattered byte loads and 2-byte stores
// (628 us for 64 images).
template <bool F16>
__global__ __launch_bounds__(256) void stem_im2col_u8_kernel(const uint8_t* __restrict__ img, const float* __restrict__ lut,
                                                             bf16_t* __restrict__ a0, int S, int H0, int xtiles) {
    constexpr int TW = (64 * 4 + 3) * 3;        // 777 bytes per input row of the tile
    __shared__ float slut[3 * 256];
    __shared__ uint8_t tile[7][TW + 7];
    __shared__ __attribute__((aligned(16))) bf16_t orow[64][STEM_K];
    const int tid = threadIdx.x;
    int bid = blockIdx.x;
    const int xt = bid % xtiles;
    bid /= xtiles;
    const int oy = bid % H0;
    const int64_t b = bid / H0;
    const int ox0 = xt * 64, ix0 = 4 * ox0 - 2, iy0 = 4 * oy - 2;
    for (int i = tid; i < 3 * 256; i += 256) slut[i] = lut[i];
    for (int i = tid; i < 7 * TW; i += 256) {
        const int ry = i / TW, c = i - ry * TW;
        const int iy = iy0 + ry, ix = ix0 + c / 3;
        tile[ry][c] = (iy >= 0 && iy < S && ix >= 0 && ix < S) ? img[((b * S + iy) * S + ix0) * 3 + c] : (uint8_t)0;
    }
    for (int i = tid; i < 64 * 2 * (STEM_KH - 147); i += 256) {        // the pad columns of both halves
        const int t = i / (2 * (STEM_KH - 147)), r = i - t * (2 * (STEM_KH - 147));
        const int half = r / (STEM_KH - 147), c = r - half * (STEM_KH - 147);
        orow[t][half * STEM_KH + 147 + c] = to_op<F16>(0.f);
    }
    __syncthreads();
    const int tok = tid & 63, part = tid >> 6;
    const int ox = ox0 + tok;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int ky = part + 4 * kk;
        if (ky >= 7) break;
        const int iy = iy0 + ky;
        const bool iny = iy >= 0 && iy < S;
        bf16_t* row = &orow[tok][ky * 21];
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
            const int ix = 4 * ox - 2 + kx;
            const bool in = iny && ix >= 0 && ix < S;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = in ? slut[c * 256 + tile[ky][(tok * 4 + kx) * 3 + c]] : 0.f;
                split_hilo<F16>(v, row[kx * 3 + c], row[STEM_KH + kx * 3 + c]);
            }
        }
    }
    __syncthreads();
    const int ntok = H0 - ox0 < 64 ? H0 - ox0 : 64;
    const int64_t m0 = (b * H0 + oy) * H0 + ox0;
    const uint4* src = reinterpret_cast<const uint4*>(&orow[0][0]);
    uint4* dst = reinterpret_cast<uint4*>(a0 + m0 * STEM_K);
    for (int i = tid; i < ntok * (STEM_K * 2 / 16); i += 256) dst[i] = src[i];
}

// Downsampling patch matrix: col[m'][(ky*3 + kx)*C + c] = xn[b][2 oy - 1 + ky][2 ox - 1 + kx][c] (zero outside).
// One thread = one 16 B chunk.
__global__ __launch_bounds__(256) void ds_im2col_kernel(const bf16_t* __restrict__ xn, bf16_t* __restrict__ col, int batch, int H,
                                                        int C) {
    const int Ho = H >> 1, cg = C >> 3;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)batch * Ho * Ho * 9 * cg;
    if (idx >= total) return;
    const int g = (int)(idx % cg);
    const int tap = (int)((idx / cg) % 9);
    const int64_t m = idx / ((int64_t)cg * 9);
    const int ox = (int)(m % Ho), oy = (int)((m / Ho) % Ho);
    const int64_t b = m / ((int64_t)Ho * Ho);
    const int iy = 2 * oy - 1 + tap / 3, ix = 2 * ox - 1 + tap % 3;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (iy >= 0 && iy < H && ix >= 0 && ix < H) v = *reinterpret_cast<const uint4*>(xn + (((b * H + iy) * H + ix) * C + g * 8));
    *reinterpret_cast<uint4*>(col + (m * 9 + tap) * C + g * 8) = v;
}

// its launch shape, shared by the forward and hiptsdbg_ccip_ds_im2col.  M: the rows of col, batch * (H / 2)^2
int launch_ds_im2col(const bf16_t* xn, bf16_t* col, int batch, int M, int H, int C, hipStream_t s) {
    const int64_t chunks = (int64_t)M * 9 * (C / 8);
    ds_im2col_kernel<<<ceil_div(chunks, 256), 256, 0, s>>>(xn, col, batch, H, C);
    HIPTS_LAUNCH_CHECK();
    return HIPTS_OK;
}


// y = act(A W^T) helpers over the shared persistent GEMM
int gemm(GemmEpilogue epi, GemmArgs& g, hipStream_t s) { return launch_gemm(epi, g, s); }

// The whole kernel sequence for images [i0, i0 + nb) on stream s.  Every workspace buffer is carved per image
// with the stride of the LARGEST stage, so that sub-batches on different streams never share bytes even when
// they are in different stages at the same time.
int ccip_run_images(hipts_ccip* h, const void* in_dev, bool is_u8, int i0, int batch, float* f_dev, hipStream_t s, bool shared_chip) {
    const auto& c = h->cfg;
    const int S = c.image_size;
    const bool f16 = c.operand_f16 != 0;
    const float* zeros = h->zeros.as<float>();
    const size_t img_bytes = (size_t)S * S * 3 * (is_u8 ? 1 : 4);
    in_dev = (const char*)in_dev + (size_t)i0 * img_bytes;
    float* x = h->x.as<float>() + (size_t)i0 * h->px;
    bf16_t* xn = h->xn.as<bf16_t>() + (size_t)i0 * h->px;
    bf16_t* h1 = h->h1.as<bf16_t>() + (size_t)i0 * h->p2c;
    bf16_t* h2 = h->h2.as<bf16_t>() + (size_t)i0 * h->p2c;
    bf16_t* m1 = h->m1.as<bf16_t>() + (size_t)i0 * h->p4c;
    bf16_t* col = h->col.as<bf16_t>() + (size_t)i0 * h->pcol;
    bf16_t* qb = h->q.as<bf16_t>() + (size_t)i0 * h->pqk;
    bf16_t* kb = h->k.as<bf16_t>() + (size_t)i0 * h->pqk;
    bf16_t* vb = h->vT.as<bf16_t>() + (size_t)i0 * h->pqk;
    bf16_t* a0 = h->a0.as<bf16_t>() + (size_t)i0 * h->st[0].T * STEM_K;
    GemmArgs g;
    bool xn_ready = false;          // xn already holds the LayerNorm the next consumer needs
    // x = rs * x + A W^T, optionally followed in the same epilogue by xn = LN(x) * gamma
    // (The e4m3 operand mode of rounds 1-3 -- operand_f16 = 2, BASELINE.json configs[4]'s "fp8 MFMA" -- was withdrawn in round 4:
    // hipts_ccip_create refuses it.  DESIGN.md section 6 has the numbers: cosine 0.968 against the float32 oracle, 1 % slower than half
    // operands, and no scaling scheme the MFMA offers lifts e4m3's three mantissa bits above 0.995 through 36 blocks.)
    // depthwise 7x7: 0 = the VALU kernel, 1 = matrix cores with the tile shape chosen by the spatial side, 2 / 3 = 32- / 48-column tiles forced
    static const int dw_mfma = getenv("HIPTS_CCIP_DW_MFMA") ? atoi(getenv("HIPTS_CCIP_DW_MFMA")) : 1;
    static const bool fused_mlp = !(getenv("HIPTS_CCIP_FUSED_MLP") && atoi(getenv("HIPTS_CCIP_FUSED_MLP")) == 0);      // A/B: 0 = fc1 and fc2 as two GEMM launches
    // The fp32 residual stream of the narrow stages (C <= 256: SepConv blocks, fused MLP) in 16 x 16 blocks of 1 KB (round 5,
    // csrc/gemm_epi.h::x_off; the ViT forward has the measurements): the loads / stores of the residual epilogues and of the fused MLP
    // are lane = (row, 4 columns of a 16-column block) -- one contiguous kilobyte per instruction instead of sixteen half lines.  Every
    // stage's stream is produced afresh by its stem / downsample GEMM, so the layout is a per-stage choice: blocked where the readers are
    // the epilogues and the fused MLP (stages 0-1; their three elementwise readers -- stem norm, two downsample norms -- read blocks),
    // row-major for the wide stages (LayerNorm kernels, pool).  HIPTS_CCIP_X_BLOCKED=0: row-major everywhere (A/B).
    static const bool xblk_env = !(getenv("HIPTS_CCIP_X_BLOCKED") && atoi(getenv("HIPTS_CCIP_X_BLOCKED")) == 0);
    auto stage_blocked = [&](int si) {
        const Stage& Sg = h->st[si];
        return xblk_env && Sg.C <= 256 && Sg.C % 16 == 0 && Sg.T % 16 == 0;
    };
    bool xblk = false;          // layout of x right now (the stage being processed)
    // xn = 16bit(LN(x) * gamma): launch_layernorm without beta -- it adds + 0.f, so -0 becomes +0 -- or, where the stream is stored in
    // 16 x 16 blocks (two downsample norms per forward), the same row_ln_kernel reading blocks, with the same + 0.f
    auto layernorm_xn = [&](const float* gamma, int64_t rows, int D) -> int {
        if (xblk) {
            const LnGamma<true> norm{gamma};
            HIPTS_LAUNCH_F16(f16, row_ln_kernel, ceil_div(rows, 4), 256, 0, s, FromF32Blocked{x}, norm, To16{xn}, rows, D, c.ln_eps);
            return HIPTS_OK;
        }
        return launch_layernorm(x, gamma, nullptr, xn, rows, D, c.ln_eps, f16, s);
    };
    auto residual = [&](GemmArgs& ga, const float* rs, const float* gamma) -> int {
        ga.res_scale = rs;
        ga.x_blocked = xblk ? 1 : 0;
        if (gamma) {
            ga.ln_gamma = gamma;
            ga.ln_eps = c.ln_eps;
            ga.out_bf16 = xn;
            return launch_gemm(EPI_RESID_LN, ga, s);
        }
        return launch_gemm(rs ? EPI_RESCALE : EPI_RESID, ga, s);
    };

    // ---- stem: conv 7x7 s4 p2 (+bias) -> bias-free LN = residual stream of stage 0
    {
        const Stage& S0 = h->st[0];
        const int64_t M = (int64_t)batch * S0.T;
        const int blocks = ceil_div(M * 7, 256);
        if (is_u8) {
            const int xtiles = ceil_div(S0.H, 64);
            const int grid_u8 = batch * S0.H * xtiles;
            HIPTS_LAUNCH_F16(f16, stem_im2col_u8_kernel, grid_u8, 256, 0, s, (const uint8_t*)in_dev, h->lut.as<float>(), a0, S, S0.H, xtiles);
        } else {
            HIPTS_LAUNCH_F16(f16, patch_gather_kernel, blocks, 256, 0, s, PixelF32Planes<false>{(const float*)in_dev}, Window7x7{}, a0, M * 7, S, S0.H);
        }
        g = gemm_args(f16, shared_chip);
        g.A = a0; g.W = h->stem_w.as<bf16_t>(); g.M = (int)M; g.N = S0.C; g.K = STEM_K;
        g.bias = h->stem_b.as<float>(); g.out_f32 = x;
        xblk = stage_blocked(0);
        g.x_blocked = xblk ? 1 : 0;
        HIPTS_TRY(gemm(EPI_BIAS, g, s));
        // bias-free LayerNorm in place: its output IS the residual stream (no + 0.f here: a -0 product stays -0 in the fp32 stream)
        const F32InPlace stream{x, xblk ? 1 : 0};
        const LnGamma<false> norm{h->stem_norm.as<float>()};
        row_ln_kernel<false><<<ceil_div(M, 4), 256, 0, s>>>(stream, norm, BackToSource{}, M, S0.C, c.ln_eps);
        HIPTS_LAUNCH_CHECK();
    }

    for (int si = 0; si < 4; ++si) {
        Stage& St = h->st[si];
        const int C = St.C, H = St.H, T = St.T, Tp = St.Tp;
        const int M = batch * T;
        if (si > 0) {
            // downsample: LN(x) -> 3x3 s2 p1 conv (+bias) -> x
            const Stage& Pv = h->st[si - 1];
            if (!xn_ready) HIPTS_TRY(layernorm_xn(St.ds_norm.as<float>(), (int64_t)batch * Pv.T, Pv.C));
            xn_ready = false;
            HIPTS_TRY(launch_ds_im2col(xn, col, batch, M, Pv.H, Pv.C, s));
            g = gemm_args(f16, shared_chip);
            g.A = col; g.W = St.ds_w.as<bf16_t>(); g.M = M; g.N = C; g.K = 9 * Pv.C;
            g.bias = St.ds_b.as<float>(); g.out_f32 = x;
            xblk = stage_blocked(si);           // (the norm above read the previous stage's layout)
            g.x_blocked = xblk ? 1 : 0;
            HIPTS_TRY(gemm(EPI_BIAS, g, s));
        }
        if (si >= c.attn_from_stage && Tp != T) {
            // the padded token rows of this stage's q / k / v^T layouts must be zero (finite at least): the
            // same bytes held another stage's values before
            const size_t bytes = (size_t)batch * Tp * C * 2;
            HIPTS_HIP(hipMemsetAsync(qb, 0, bytes, s));
            HIPTS_HIP(hipMemsetAsync(kb, 0, bytes, s));
            HIPTS_HIP(hipMemsetAsync(vb, 0, bytes, s));
        }
        // A stage whose rows fit one 256-wide GEMM tile gets its LayerNorms from the epilogue of the residual GEMM
        // that produces the row (EPI_RESID_LN): the separate pass over the fp32 stream is the largest HBM
        // consumer of the wide early stages.
        const bool fuse_ln = C <= 256 && !getenv("HIPTS_CCIP_NO_LN_FUSION");
        // Wide stages (rows of more than one 256-column tile: C = 512, 768; round 5): the LayerNorms are folded as in the ViT -- the residual
        // GEMM that finishes a row (EPI_RESID_XG, here with the CAFormer's res_scale) also writes gamma * x as the consumer's 16-bit operand
        // and the row's partial sums; q | k, v and fc1 apply rstd / mean in their epilogues (col_u = W gamma; the CAFormer's norms have no
        // beta).  40 of a forward's 45 row_ln_kernel launches (5.2 % of its kernel time, each a pass over the fp32 stream) go; a stage's
        // first norm1 (its rows come from the downsample GEMM) and the downsample norms (their consumer is the im2col) stay.  Only when the
        // stage's residual launches are not the two-workgroups-per-CU kernel's anyway (that loop has no statistics epilogue): more tiles
        // than gemm_dw_size() takes (half the CUs by default).  HIPTS_CCIP_LN_FOLD=0: off (A/B).
        static const bool fold_env = !(getenv("HIPTS_CCIP_LN_FOLD") && atoi(getenv("HIPTS_CCIP_LN_FOLD")) == 0);
        const int sblocks = (C + 255) / 256;
        const bool fold23 = fold_env && !fuse_ln && si >= c.attn_from_stage && C % 256 == 0 && M % 256 == 0 && h->stat_part.p &&
                            !gemm_dw_size((long)((M + 255) / 256) * sblocks, current_device_cus(nullptr), gemm_knobs());
        float* stat_p = fold23 ? h->stat_part.as<float>() + 2 * (size_t)i0 * h->pstat : nullptr;
        bool xn_folded = false;         // xn holds gamma * x + stat_p the row sums (not the LayerNorm itself)
        auto folded = [&](GemmArgs& ga, const float* u) {
            ga.stat_in = stat_p; ga.stat_in_blocks = sblocks; ga.stat_in_stride = M; ga.ln_dim = C; ga.ln_eps = c.ln_eps;
            ga.col_u = u; ga.bias = zeros;
        };
        auto residual_xg = [&](GemmArgs& ga, const float* rs, const float* gamma) -> int {
            ga.res_scale = rs; ga.ln_gamma = gamma; ga.ln_eps = c.ln_eps; ga.out_bf16 = xn; ga.stat_part = stat_p; ga.stat_stride = M;
            ga.x_blocked = xblk ? 1 : 0;
            return launch_gemm(EPI_RESID_XG, ga, s);
        };
        for (size_t bi = 0; bi < St.blocks.size(); ++bi) {
            Block& B = St.blocks[bi];
            const bool in_folded = xn_ready && xn_folded;
            if (!xn_ready) HIPTS_TRY(layernorm_xn(B.n1.as<float>(), M, C));
            xn_ready = false;
            xn_folded = false;
            // LayerNorm that follows this block's MLP: the next block's norm1, or the next stage's downsample norm
            const float* next_gamma = bi + 1 < St.blocks.size() ? St.blocks[bi + 1].n1.as<float>()
                                      : (si < 3 ? h->st[si + 1].ds_norm.as<float>() : nullptr);
            if (!B.attn) {
                // SepConv: 1x1 (C -> 2C) + StarReLU -> depthwise 7x7 -> 1x1 (2C -> C) + residual
                g = gemm_args(f16, shared_chip);
                g.A = xn; g.W = B.w_in.as<bf16_t>(); g.M = M; g.N = 2 * C; g.K = C; g.bias = zeros;
                g.out_bf16 = h1; g.star_scale = B.s1; g.star_bias = B.b1;
                HIPTS_TRY(gemm(EPI_STAR, g, s));
                const int tiles_x = ceil_div(H, DW_TW), tiles_y = ceil_div(H, DW_TH);
                const int dw_grid = batch * tiles_y * tiles_x * (2 * C / DW_CS);
                if (f16 && H >= 16 && dw_mfma && B.dwz.p) HIPTS_TRY(launch_dwconv7_mfma(h1, B.dwz.as<uint32_t>(), h2, batch, H, 2 * C, dw_mfma, s));
                else HIPTS_LAUNCH_F16(f16, dwconv7_kernel, dw_grid, 256, DW_LDS_BYTES, s, h1, B.dw.as<float>(), h2, H, 2 * C, tiles_x, tiles_y);
                g = gemm_args(f16, shared_chip);
                g.A = h2; g.W = B.w_out.as<bf16_t>(); g.M = M; g.N = C; g.K = 2 * C; g.bias = zeros; g.out_f32 = x;
                HIPTS_TRY(residual(g, B.has_rs1 ? B.rs1.as<float>() : nullptr, fuse_ln ? B.n2.as<float>() : nullptr));
            } else {
                const int heads = C / c.head_dim;
                g = gemm_args(f16, shared_chip);
                g.A = xn; g.W = B.w_in.as<bf16_t>(); g.M = M; g.N = 2 * C; g.K = C; g.bias = zeros;
                g.out_bf16 = qb; g.out2_bf16 = kb;
                g.tokens = T; g.tokens_pad = Tp; g.heads = heads; g.dim = C; g.hd_log2 = 5;
                g.qscale = 0.17677669529663687f * 1.4426950408889634f;      // 32^-0.5 * log2(e): attention works in base 2
                if (in_folded) folded(g, B.u_qk.as<float>());
                HIPTS_TRY(gemm(EPI_QK, g, s));
                g = gemm_args(f16, shared_chip);
                g.A = xn; g.W = B.w_in.as<bf16_t>() + (size_t)2 * C * C; g.M = M; g.N = C; g.K = C; g.bias = zeros;
                g.out_bf16 = vb;
                g.tokens = T; g.tokens_pad = Tp; g.heads = heads; g.dim = C; g.hd_log2 = 5;
                if (in_folded) folded(g, B.u_v.as<float>());
                HIPTS_TRY(gemm(EPI_VT, g, s));
                HIPTS_TRY(launch_attention(qb, kb, vb, h1, batch, heads, T, Tp,
                                           f16, s, 32));
                g = gemm_args(f16, shared_chip);
                g.A = h1; g.W = B.w_out.as<bf16_t>(); g.M = M; g.N = C; g.K = C; g.bias = zeros; g.out_f32 = x;
                if (fold23) HIPTS_TRY(residual_xg(g, B.has_rs1 ? B.rs1.as<float>() : nullptr, B.n2.as<float>()));
                else HIPTS_TRY(residual(g, B.has_rs1 ? B.rs1.as<float>() : nullptr, fuse_ln ? B.n2.as<float>() : nullptr));
            }
            // MLP: fc1 + StarReLU, fc2 + residual
            const bool mlp_folded = fold23 && B.attn;
            if (!fuse_ln && !mlp_folded) HIPTS_TRY(layernorm_xn(B.n2.as<float>(), M, C));
            if (fused_mlp && fuse_ln && f16 && B.mlp_img.p) {
                // stages 0-1 (rows of <= 256 columns): one kernel, the hidden tensor stays in registers (mlp.hip)
                const bool fuse_next = next_gamma != nullptr;
                HIPTS_TRY(launch_mlp_fused(xn, B.mlp_img.p, x, B.has_rs2 ? B.rs2.as<float>() : nullptr, next_gamma, xn, M, C, B.s2, B.b2, c.ln_eps, s, 0,
                                           xblk ? 1 : 0));
                xn_ready = fuse_next;
                continue;
            }
            g = gemm_args(f16, shared_chip);
            g.A = xn; g.W = B.fc1.as<bf16_t>(); g.M = M; g.N = 4 * C; g.K = C; g.bias = zeros;
            g.out_bf16 = m1; g.star_scale = B.s2; g.star_bias = B.b2;
            if (mlp_folded) folded(g, B.u_fc1.as<float>());
            HIPTS_TRY(gemm(EPI_STAR, g, s));
            g = gemm_args(f16, shared_chip);
            g.A = m1; g.W = B.fc2.as<bf16_t>(); g.M = M; g.N = C; g.K = 4 * C; g.bias = zeros; g.out_f32 = x;
            const bool fuse_next = fuse_ln && next_gamma != nullptr;
            // folded: the next block's norm1 (same stage: an attention block too) is prepared here
            const bool xg_next = fold23 && bi + 1 < St.blocks.size() && St.blocks[bi + 1].attn;
            if (xg_next) HIPTS_TRY(residual_xg(g, B.has_rs2 ? B.rs2.as<float>() : nullptr, St.blocks[bi + 1].n1.as<float>()));
            else HIPTS_TRY(residual(g, B.has_rs2 ? B.rs2.as<float>() : nullptr, fuse_next ? next_gamma : nullptr));
            xn_ready = fuse_next || xg_next;
            xn_folded = xg_next;
        }
    }
    // ---- head: global average pool -> LayerNorm
    const Stage& L = h->st[3];
    pool_ln_kernel<false><<<batch, 1024, 0, s>>>(x, h->head_g.as<float>(), h->head_b.as<float>(), PooledF32{f_dev + (size_t)i0 * L.C}, L.T, L.C, c.ln_eps,
                                                 xblk ? 1 : 0, L.T);
    HIPTS_LAUNCH_CHECK();
    return HIPTS_OK;
}

int ccip_forward_impl(hipts_ccip* h, const void* input, int in_memspace, bool is_u8, int batch, float* out, int out_memspace,
                      hipStream_t s) {
    HIPTS_REQUIRE(h && input && out && batch >= 1, "hipts_ccip_forward: bad arguments");
    HIPTS_REQUIRE(batch <= h->cfg.max_batch, "batch %d exceeds max_batch %d", batch, h->cfg.max_batch);
    HIPTS_TRY(h->ledger.require_complete("hipts_ccip_forward"));
    HIPTS_TRY(use_device(h->device));
    const auto& c = h->cfg;
    const int S = c.image_size;
    const void* in_dev = nullptr;
    HIPTS_TRY(stage_input(h->img_in, input, in_memspace, (size_t)batch * S * S * 3 * (is_u8 ? 1 : 4), s, &in_dev));
    const bool dev_out = out_memspace == HIPTS_DEVICE;
    float* f_dev = dev_out ? out : h->feat.as<float>();
    if (h->fold_dirty) {        // W gamma of the wide stages' q | k, v and fc1 (folded LayerNorms): once per checkpoint
        const bool f16w = c.operand_f16 != 0;
        for (int si = c.attn_from_stage; si < 4; ++si) {
            Stage& St = h->st[si];
            const int C = St.C;
            if (C <= 256 || C % 256) continue;
            HIPTS_TRY(h->fold_c.reserve((size_t)4 * C * 4));
            for (Block& B : St.blocks) {
                if (!B.attn) continue;
                HIPTS_TRY(B.u_qk.reserve((size_t)2 * C * 4));
                HIPTS_TRY(B.u_v.reserve((size_t)C * 4));
                HIPTS_TRY(B.u_fc1.reserve((size_t)4 * C * 4));
                HIPTS_TRY(launch_fold_ln(B.w_in.as<bf16_t>(), f16w, B.n1.as<float>(), nullptr, nullptr, B.u_qk.as<float>(), h->fold_c.as<float>(), 2 * C, C, s));
                HIPTS_TRY(launch_fold_ln(B.w_in.as<bf16_t>() + (size_t)2 * C * C, f16w, B.n1.as<float>(), nullptr, nullptr, B.u_v.as<float>(),
                                         h->fold_c.as<float>(), C, C, s));
                HIPTS_TRY(launch_fold_ln(B.fc1.as<bf16_t>(), f16w, B.n2.as<float>(), nullptr, nullptr, B.u_fc1.as<float>(), h->fold_c.as<float>(), 4 * C, C, s));
            }
        }
        h->fold_dirty = false;
    }
    // Two sub-batches on two internal streams (as in the ViT forward): the late stages have fewer output
    // tiles than the chip has CUs, and a kernel of one half fills the CUs the other half leaves idle.
    static const int want_streams = getenv("HIPTS_CCIP_STREAMS") ? atoi(getenv("HIPTS_CCIP_STREAMS")) : 2;
    // (measured, B36 @384: batch 64 2567 -> 2809 images/s; at the reference's batch of 20 the halves are too small
    // to gain and the doubled launch count costs, so small batches stay on the caller's stream)
    static const int min_sub = getenv("HIPTS_CCIP_MINSUB") && atoi(getenv("HIPTS_CCIP_MINSUB")) > 0 ? atoi(getenv("HIPTS_CCIP_MINSUB")) : 16;      // images per sub-batch needed to split
    const int ns = std::min({want_streams, (int)hipts_ccip::MAX_SUB, batch / min_sub});      // (round 5, HIPTS_CCIP_STREAMS = 2 / 3 / 4 at batch 64: 3608 / 3458 / 2844 images/s -- two it stays)
    HIPTS_TRY(run_split(h->streams, s, batch, ns, [&](int i0, int nb, hipStream_t st, bool shared_chip, int) {
        return ccip_run_images(h, in_dev, is_u8, i0, nb, f_dev, st, shared_chip);
    }));
    if (!dev_out) HIPTS_TRY(read_back(s, (size_t)batch * h->st[3].C * 4, out, f_dev));      // a single output: the pooled features
    return HIPTS_OK;
}

}  // namespace

extern "C" {

int hipts_ccip_create(const hipts_ccip_config_t* cfg, int device, hipts_ccip_t** out) {
    HIPTS_REQUIRE(cfg && out, "hipts_ccip_create: null argument");
    HIPTS_REQUIRE(cfg->image_size >= 32 && cfg->image_size % 32 == 0, "image_size %d must be a multiple of 32", cfg->image_size);
    HIPTS_REQUIRE(cfg->head_dim == 32, "head_dim %d: only 32 is built", cfg->head_dim);
    HIPTS_REQUIRE(cfg->max_batch >= 1, "max_batch must be >= 1");
    HIPTS_REQUIRE(cfg->operand_f16 == 0 || cfg->operand_f16 == 1,
                  "operand_f16 = %d: 0 (bf16) or 1 (IEEE half); the e4m3 mode (2) was withdrawn in round 4 -- cosine 0.968 against the float32 "
                  "forward and no faster than half operands (DESIGN.md section 6)", cfg->operand_f16);
    HIPTS_REQUIRE(cfg->attn_from_stage >= 0 && cfg->attn_from_stage <= 4, "attn_from_stage must be 0 .. 4");
    for (int s = 0; s < 4; ++s) {
        HIPTS_REQUIRE(cfg->dims[s] >= 64 && cfg->dims[s] % 64 == 0 && cfg->dims[s] <= 1024, "dims[%d] = %d must be a multiple of 64, at most 1024",
                      s, cfg->dims[s]);
        HIPTS_REQUIRE(cfg->depths[s] >= 1, "depths[%d] must be >= 1", s);
    }
    HIPTS_TRY(use_device(device));
    auto* h = new hipts_ccip();
    h->device = device;
    h->cfg = *cfg;
    const int B = cfg->max_batch;
    size_t max_x = 0, max_2c = 0, max_4c = 0, max_col = 16, max_qk = 16;
    double flops = 0.0;
    int H = cfg->image_size / 4;
    flops += 2.0 * H * H * cfg->dims[0] * 147.0;
    for (int s = 0; s < 4; ++s) {
        Stage& St = h->st[s];
        if (s > 0) H /= 2;
        St.C = cfg->dims[s];
        St.H = H;
        St.T = H * H;
        St.Tp = round_up(St.T, 64);
        St.blocks.resize(cfg->depths[s]);
        const double T = St.T, C = St.C;
        if (s > 0) flops += 2.0 * T * C * 9.0 * cfg->dims[s - 1];
        for (int i = 0; i < cfg->depths[s]; ++i) {
            Block& Bk = St.blocks[i];
            Bk.attn = s >= cfg->attn_from_stage;
            if (Bk.attn) flops += 2.0 * T * 3 * C * C + 4.0 * T * T * C + 2.0 * T * C * C;
            else flops += 2.0 * T * 2 * C * C * 2 + 2.0 * 49.0 * T * 2 * C;
            flops += 2.0 * T * 4 * C * C * 2;
        }
        h->px = std::max(h->px, (size_t)St.T * St.C);
        if (St.C > 256 && St.C % 256 == 0) h->pstat = std::max(h->pstat, (size_t)(St.C / 256) * St.T);
        h->p2c = std::max(h->p2c, (size_t)St.T * 2 * St.C);
        h->p4c = std::max(h->p4c, (size_t)St.T * 4 * St.C);
        if (s > 0) h->pcol = std::max(h->pcol, (size_t)St.T * 9 * cfg->dims[s - 1]);
        if (s >= cfg->attn_from_stage) h->pqk = std::max(h->pqk, (size_t)St.Tp * St.C);
    }
    max_x = (size_t)B * h->px;
    max_2c = (size_t)B * h->p2c;
    max_4c = (size_t)B * h->p4c;
    max_col = std::max(max_col, (size_t)B * h->pcol);
    max_qk = std::max(max_qk, (size_t)B * h->pqk);
    h->flops_per_image = flops;
    int st = 0;
    std::vector<float> z(4096, 0.f);
    const double mean[3] = {0.48145466, 0.4578275, 0.40821073}, stdv[3] = {0.26862954, 0.26130258, 0.27577711};   // gen_cfeatures.py:103-104
    const std::vector<float> lut = norm_lut(mean, stdv);      // (x - mean) / std in float64, as the reference's numpy does
    if ((st = upload_f32(h->zeros, z.data(), z.size())) || (st = upload_f32(h->lut, lut.data(), lut.size())) || (st = h->a0.alloc((size_t)B * h->st[0].T * STEM_K * 2)) ||
        (st = h->x.alloc(max_x * 4)) || (st = h->xn.alloc(max_x * 2)) || (st = h->h1.alloc(max_2c * 2)) || (st = h->h2.alloc(max_2c * 2)) ||
        (st = h->m1.alloc(max_4c * 2)) || (st = h->col.alloc(max_col * 2)) || (st = h->q.alloc(max_qk * 2)) || (st = h->k.alloc(max_qk * 2)) ||
        (st = h->vT.alloc(max_qk * 2)) || (st = h->feat.alloc((size_t)B * cfg->dims[3] * 4)) ||
        (h->pstat && (st = h->stat_part.alloc((size_t)B * h->pstat * 8)))) {
        delete h;
        return st;
    }
    // pad columns of the stem patch matrix and the padded token rows of q / k / v^T stay zero for ever
    hipError_t e = hipMemset(h->a0.p, 0, h->a0.bytes);
    if (e == hipSuccess) e = hipMemset(h->q.p, 0, h->q.bytes);
    if (e == hipSuccess) e = hipMemset(h->k.p, 0, h->k.bytes);
    if (e == hipSuccess) e = hipMemset(h->vT.p, 0, h->vT.bytes);
    if (e != hipSuccess) {
        delete h;
        return set_error(HIPTS_ERR_HIP, "hipMemset failed: %s", hipGetErrorString(e));
    }
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)dwconv7_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, DW_LDS_BYTES);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)dwconv7_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, DW_LDS_BYTES);
    if (e != hipSuccess) {
        delete h;
        return set_error(HIPTS_ERR_HIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    }
    auto need = [&](const std::string& k) { h->ledger.need(k); };
    need("stem.conv.weight"); need("stem.conv.bias"); need("stem.norm.weight"); need("head.norm.weight"); need("head.norm.bias");
    for (int s = 0; s < 4; ++s) {
        const std::string sp = "stages." + std::to_string(s) + ".";
        if (s > 0) { need(sp + "downsample.norm.weight"); need(sp + "downsample.conv.weight"); need(sp + "downsample.conv.bias"); }
        for (int i = 0; i < cfg->depths[s]; ++i) {
            const std::string p = sp + "blocks." + std::to_string(i) + ".";
            need(p + "norm1.weight"); need(p + "norm2.weight");
            if (s >= cfg->attn_from_stage) { need(p + "token_mixer.qkv.weight"); need(p + "token_mixer.proj.weight"); }
            else {
                need(p + "token_mixer.pwconv1.weight"); need(p + "token_mixer.act1.scale"); need(p + "token_mixer.act1.bias");
                need(p + "token_mixer.dwconv.weight"); need(p + "token_mixer.pwconv2.weight");
            }
            need(p + "mlp.fc1.weight"); need(p + "mlp.act.scale"); need(p + "mlp.act.bias"); need(p + "mlp.fc2.weight");
        }
    }
    *out = h;
    return HIPTS_OK;
}

int hipts_ccip_destroy(hipts_ccip_t* h) {
    if (h) {
        (void)hipSetDevice(h->device);
        (void)hipDeviceSynchronize();
        delete h;
    }
    return HIPTS_OK;
}

int hipts_ccip_set_tensor(hipts_ccip_t* h, const char* key_c, const float* data, int64_t numel) {
    HIPTS_REQUIRE(h && key_c && data, "hipts_ccip_set_tensor: null argument");
    HIPTS_TRY(use_device(h->device));
    const std::string key(key_c);
    const bool f16 = h->cfg.operand_f16 != 0;
    int st = HIPTS_OK;
    const int C0 = h->cfg.dims[0], C3 = h->cfg.dims[3];
    int s = 0, bi = 0;
    std::string sub, t;
    if (key == "stem.conv.weight") {
        EXPECT_NUMEL((int64_t)C0 * 147);
        const std::vector<float> w2 = stem_weight_hilo(data, C0, 49, STEM_KH, false);      // the hi | lo halves of the stem patch matrix
        st = upload_matrix16(h->stem_w, w2.data(), C0, STEM_K, round_up(C0, 256), f16);
    } else if (key == "stem.conv.bias") { EXPECT_NUMEL(C0); st = upload_f32(h->stem_b, data, C0); }
    else if (key == "stem.norm.weight") { EXPECT_NUMEL(C0); st = upload_f32(h->stem_norm, data, C0); }
    else if (key == "head.norm.weight") { EXPECT_NUMEL(C3); st = upload_f32(h->head_g, data, C3); }
    else if (key == "head.norm.bias") { EXPECT_NUMEL(C3); st = upload_f32(h->head_b, data, C3); }
    else if (parse_indexed(key, "stages.", &s, &sub)) {
        if (s < 0 || s > 3) return set_error(HIPTS_ERR_INVALID, "tensor %s: stage out of range", key_c);
        Stage& St = h->st[s];
        const int C = St.C;
        if (sub.rfind("downsample.", 0) == 0) {
            if (s == 0) return set_error(HIPTS_ERR_INVALID, "tensor %s: stage 0 has no downsample", key_c);
            const int Cp = h->cfg.dims[s - 1];
            if (sub == "downsample.norm.weight") { EXPECT_NUMEL(Cp); st = upload_f32(St.ds_norm, data, Cp); }
            else if (sub == "downsample.conv.bias") { EXPECT_NUMEL(C); st = upload_f32(St.ds_b, data, C); }
            else if (sub == "downsample.conv.weight") {
                EXPECT_NUMEL((int64_t)C * Cp * 9);
                std::vector<float> w2((size_t)C * 9 * Cp);          // [n][c][tap] -> [n][tap*Cp + c]
                for (int n = 0; n < C; ++n)
                    for (int cc = 0; cc < Cp; ++cc)
                        for (int t = 0; t < 9; ++t) w2[((size_t)n * 9 + t) * Cp + cc] = data[((size_t)n * Cp + cc) * 9 + t];
                st = upload_matrix16(St.ds_w, w2.data(), C, 9 * Cp, round_up(C, 256), f16);
            } else return set_error(HIPTS_ERR_INVALID, "unknown tensor key %s", key_c);
        } else if (parse_indexed(sub, "blocks.", &bi, &t)) {
            if (bi < 0 || bi >= (int)St.blocks.size()) return set_error(HIPTS_ERR_INVALID, "tensor %s: block out of range", key_c);
            Block& B = St.blocks[bi];
            auto up = [&](DevBuf& buf, int rows, int cols, int rows_pad) -> int { return upload_matrix16(buf, data, rows, cols, rows_pad, f16); };
            if (t == "norm1.weight") { EXPECT_NUMEL(C); st = upload_f32(B.n1, data, C); }
            else if (t == "norm2.weight") { EXPECT_NUMEL(C); st = upload_f32(B.n2, data, C); }
            else if (t == "res_scale1.scale") { EXPECT_NUMEL(C); st = upload_f32(B.rs1, data, C); B.has_rs1 = true; }
            else if (t == "res_scale2.scale") { EXPECT_NUMEL(C); st = upload_f32(B.rs2, data, C); B.has_rs2 = true; }
            else if (t == "mlp.fc1.weight" || t == "mlp.fc2.weight") {
                EXPECT_NUMEL((int64_t)4 * C * C);
                const bool first = t == "mlp.fc1.weight";
                st = first ? up(B.fc1, 4 * C, C, round_up(4 * C, 256)) : up(B.fc2, C, 4 * C, round_up(C, 256));
                if (st == HIPTS_OK && f16 && mlp_fused_supports(C)) {
                    (first ? B.fc1_host : B.fc2_host).assign(data, data + (size_t)4 * C * C);
                    if (!B.fc1_host.empty() && !B.fc2_host.empty()) {
                        const std::vector<uint16_t> img = mlp_weight_image(B.fc1_host.data(), B.fc2_host.data(), C);
                        st = B.mlp_img.alloc(img.size() * 2);
                        if (st == HIPTS_OK) st = upload(B.mlp_img.p, img.data(), img.size() * 2);
                    }
                }
            }
            else if (t == "mlp.act.scale") { EXPECT_NUMEL(1); B.s2 = data[0]; }
            else if (t == "mlp.act.bias") { EXPECT_NUMEL(1); B.b2 = data[0]; }
            else if (!B.attn && t == "token_mixer.pwconv1.weight") { EXPECT_NUMEL((int64_t)2 * C * C); st = upload_matrix16(B.w_in, data, 2 * C, C, round_up(2 * C, 256), f16); }
            else if (!B.attn && t == "token_mixer.pwconv2.weight") { EXPECT_NUMEL((int64_t)2 * C * C); st = up(B.w_out, C, 2 * C, round_up(C, 256)); }
            else if (!B.attn && t == "token_mixer.act1.scale") { EXPECT_NUMEL(1); B.s1 = data[0]; }
            else if (!B.attn && t == "token_mixer.act1.bias") { EXPECT_NUMEL(1); B.b1 = data[0]; }
            else if (!B.attn && t == "token_mixer.dwconv.weight") {
                EXPECT_NUMEL((int64_t)2 * C * 49);
                std::vector<float> w2((size_t)49 * 2 * C);          // [c][tap] -> [tap][c]
                for (int cc = 0; cc < 2 * C; ++cc)
                    for (int tp = 0; tp < 49; ++tp) w2[(size_t)tp * 2 * C + cc] = data[(size_t)cc * 49 + tp];
                st = upload_f32(B.dw, w2.data(), w2.size());
                if (st == HIPTS_OK && f16) {
                    const std::vector<uint32_t> tzv = dw_toeplitz_lanes(data, 2 * C);
                    st = upload_f32(B.dwz, reinterpret_cast<const float*>(tzv.data()), tzv.size());
                }
            }
            else if (B.attn && t == "token_mixer.qkv.weight") {
                EXPECT_NUMEL((int64_t)3 * C * C);
                // q|k rows and the v rows are read by separate launches whose last tile may run past its
                // own rows: pad behind the v rows as well
                st = upload_matrix16(B.w_in, data, 3 * C, C, round_up(2 * C, 256) + round_up(C, 256) + 256, f16);
            }
            else if (B.attn && t == "token_mixer.proj.weight") { EXPECT_NUMEL((int64_t)C * C); st = upload_matrix16(B.w_out, data, C, C, round_up(C, 256), f16); }
            else return set_error(HIPTS_ERR_INVALID, "unknown tensor key %s", key_c);
        } else return set_error(HIPTS_ERR_INVALID, "unknown tensor key %s", key_c);
    } else return set_error(HIPTS_ERR_INVALID, "unknown tensor key %s", key_c);
    if (st) return st;
    h->fold_dirty = true;
    h->ledger.mark_set(key);
    return HIPTS_OK;
}

int hipts_ccip_forward_u8(hipts_ccip_t* h, const uint8_t* images, int images_memspace, int batch, float* features_out,
                          int out_memspace, void* stream) {
    return ccip_forward_impl(h, images, images_memspace, true, batch, features_out, out_memspace, (hipStream_t)stream);
}

int hipts_ccip_forward_f32(hipts_ccip_t* h, const float* x, int x_memspace, int batch, float* features_out, int out_memspace,
                           void* stream) {
    return ccip_forward_impl(h, x, x_memspace, false, batch, features_out, out_memspace, (hipStream_t)stream);
}

int hipts_ccip_flops_per_image(const hipts_ccip_t* h, double* flops) {
    HIPTS_REQUIRE(h && flops, "null argument");
    *flops = h->flops_per_image;
    return HIPTS_OK;
}

// Debug / test entry (include/hip_tagsearch_debug.h): the depthwise 7x7 of a SepConv block on its own.
int hiptsdbg_dwconv7(const uint16_t* in_f16, const float* w, uint16_t* out_f16, int batch, int H, int C, int mode, int iters, float* ms_out) {
    HIPTS_REQUIRE(in_f16 && w && out_f16 && batch >= 1 && H >= 1 && C >= 64 && C % 64 == 0 && mode >= 0 && mode <= 3, "hiptsdbg_dwconv7: bad argument");
    HIPTS_REQUIRE(mode == 0 || H >= 16, "hiptsdbg_dwconv7: the matrix-core kernel needs a side of 16 or more");
    const size_t n = (size_t)batch * H * H * C;
    DevBuf in, out, wv, tz;
    HIPTS_TRY(in.alloc(n * 2));
    HIPTS_TRY(out.alloc(n * 2));
    HIPTS_TRY(upload(in.p, in_f16, n * 2));
    std::vector<float> w2((size_t)49 * C);
    for (int cc = 0; cc < C; ++cc)
        for (int tp = 0; tp < 49; ++tp) w2[(size_t)tp * C + cc] = w[(size_t)cc * 49 + tp];
    HIPTS_TRY(upload_f32(wv, w2.data(), w2.size()));
    const std::vector<uint32_t> tzv = dw_toeplitz_lanes(w, C);
    HIPTS_TRY(upload_f32(tz, reinterpret_cast<const float*>(tzv.data()), tzv.size()));
    hipEvent_t e0, e1;
    HIPTS_HIP(hipEventCreate(&e0));
    HIPTS_HIP(hipEventCreate(&e1));
    const int tiles_x = ceil_div(H, DW_TW), tiles_y = ceil_div(H, DW_TH);
    for (int it = 0; it <= iters; ++it) {
        if (it == 1) HIPTS_HIP(hipEventRecord(e0, nullptr));
        if (mode == 0) {
            dwconv7_kernel<true><<<batch * tiles_y * tiles_x * (C / DW_CS), 256, DW_LDS_BYTES, nullptr>>>(in.as<bf16_t>(), wv.as<float>(), out.as<bf16_t>(), H, C, tiles_x, tiles_y);
            HIPTS_LAUNCH_CHECK();
        } else {
            HIPTS_TRY(launch_dwconv7_mfma(in.as<bf16_t>(), tz.as<uint32_t>(), out.as<bf16_t>(), batch, H, C, mode, nullptr));
        }
    }
    HIPTS_HIP(hipEventRecord(e1, nullptr));
    HIPTS_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    if (iters > 0) HIPTS_HIP(hipEventElapsedTime(&ms, e0, e1));
    if (ms_out) *ms_out = iters > 0 ? ms / iters : 0.f;
    HIPTS_HIP(hipEventDestroy(e0));
    HIPTS_HIP(hipEventDestroy(e1));
    HIPTS_HIP(hipMemcpy(out_f16, out.p, n * 2, hipMemcpyDeviceToHost));
    return HIPTS_OK;
}

// Host only (no GPU call): the lane images dw_toeplitz_lanes builds from weights [channels][49], u32 [channels][7][64]
// (tests/test_host_layouts.py, runs without a GPU).
int hiptsdbg_dw_toeplitz(const float* w, int channels, uint32_t* out) {
    HIPTS_REQUIRE(w && out && channels >= 1, "hiptsdbg_dw_toeplitz: bad argument");
    const std::vector<uint32_t> t = dw_toeplitz_lanes(w, channels);
    memcpy(out, t.data(), t.size() * 4);
    return HIPTS_OK;
}

// the stamps of a -DHIPTS_DW_STAMPS build (zeros otherwise): [0] start, [1] operands built, then per tile 8 stamps from [2]: start, loads
// requested, planes written, barrier, products done, barrier, results in LDS + barrier, stores issued; [31] end
int hiptsdbg_dwconv7_stamps(unsigned long long* host, int n) {
    HIPTS_REQUIRE(host && n >= 1 && n <= 32, "hiptsdbg_dwconv7_stamps: bad argument");
    HIPTS_HIP(hipMemcpyFromSymbol(host, HIP_SYMBOL(dw_stamps), (size_t)n * 8));
    return HIPTS_OK;
}

// Debug / test entry: stem_im2col_u8_kernel once, launched as the forward launches it, into an a0 of a0_bytes filled with `fill` and copied
// back whole (tests/test_gpu_rows.py compares it with the generic gather of csrc/rows_dbg.hip).
int hiptsdbg_ccip_stem_u8(const uint8_t* images, const float* lut, int batch, int S, int f16, int fill, uint16_t* a0, uint64_t a0_bytes) {
    HIPTS_REQUIRE(images && lut && a0 && batch >= 1 && batch <= 64 && S >= 4 && S <= 1024 && S % 4 == 0, "hiptsdbg_ccip_stem_u8: bad argument");
    const int H0 = S / 4, xtiles = ceil_div(H0, 64);
    HIPTS_REQUIRE(a0_bytes >= (uint64_t)batch * H0 * H0 * STEM_K * 2, "hiptsdbg_ccip_stem_u8: a0 has %llu bytes, the launch's extent is %llu",
                  (unsigned long long)a0_bytes, (unsigned long long)batch * H0 * H0 * STEM_K * 2);
    HIPTS_TRY(use_device(0));
    DevBuf img, lutd, ad;
    HIPTS_TRY(img.alloc((size_t)batch * S * S * 3));
    HIPTS_TRY(upload(img.p, images, (size_t)batch * S * S * 3));
    HIPTS_TRY(upload_f32(lutd, lut, 3 * 256));
    HIPTS_TRY(ad.alloc(a0_bytes));
    HIPTS_HIP(hipMemset(ad.p, fill & 0xff, a0_bytes));
    HIPTS_LAUNCH_F16(f16 != 0, stem_im2col_u8_kernel, batch * H0 * xtiles, 256, 0, nullptr, img.as<uint8_t>(), lutd.as<float>(), ad.as<bf16_t>(), S, H0, xtiles);
    HIPTS_HIP(hipDeviceSynchronize());
    HIPTS_HIP(hipMemcpy(a0, ad.p, a0_bytes, hipMemcpyDeviceToHost));
    return HIPTS_OK;
}

// Debug / test entry (tests/test_gpu_tokens.py): ds_im2col_kernel once, launched as the forward launches it, col filled with `fill` before
// and copied back whole.
int hiptsdbg_ccip_ds_im2col(const uint16_t* xn, uint64_t xn_bytes, int batch, int H, int C, int fill, uint16_t* col, uint64_t col_bytes) {
    const char* who = "hiptsdbg_ccip_ds_im2col";
    HIPTS_REQUIRE(xn && col, "%s: null argument", who);
    HIPTS_REQUIRE(batch >= 1 && batch <= 4096 && H >= 2 && H <= 1024 && H % 2 == 0, "%s: H=%d must be even (batch %d)", who, H, batch);
    HIPTS_REQUIRE(C >= 8 && C % 8 == 0 && C <= 4096, "%s: C=%d must be a multiple of 8", who, C);
    HIPTS_REQUIRE(xn_bytes >= (uint64_t)batch * H * H * C * 2, "%s: xn does not cover the launch", who);
    HIPTS_TRY(use_device(0));
    const int M = batch * (H / 2) * (H / 2);
    DevBuf xd, cd;
    HIPTS_TRY(dbg_guarded(cd, col_bytes, (uint64_t)M * 9 * C * 2, fill, who, "col"));
    HIPTS_TRY(dbg_put(xd, xn, xn_bytes));
    HIPTS_TRY(launch_ds_im2col(xd.as<bf16_t>(), cd.as<bf16_t>(), batch, M, H, C, nullptr));
    HIPTS_HIP(hipDeviceSynchronize());
    return dbg_fetch(col, cd, col_bytes, who);
}

}  // extern "C"
