// eva.hip -- EVA02 tagger forward (the model tagging.py:45 really loads: wd-eva02-large-tagger-v3 =
// timm eva02_large_patch14_448) behind hipts_eva_*.
//
// Replaces `model.forward(batched_tensor)` + `F.sigmoid` (tagging.py:174-176) for that model family:
//   patch-embed conv 14x14 s14 (+bias) -> [cls | patches] + pos_embed -> depth x {
//       x += proj(softmax(rope(q) rope(k)^T / 8) v)     q/k/v = Linear(LN(x)) (q, v biased, k not), 2-D axial
//                                                        RoPE on the patch tokens, head_dim 64
//       x += fc2(LN(silu(fc1_g(LN(x))) * fc1_x(LN(x))))  SwiGLU with inner LayerNorm }
//   -> mean over the patch tokens -> fc_norm -> head (+ sigmoid).            (oracle/eva.py restates the same graph)
//
// Built from the pieces of the ViT-B/16 path: every Linear is the persistent MFMA GEMM of gemm.hip (q|k and v^T
// epilogues write the attention layouts, +bias+residual epilogues do the fp32 read-modify-write, the
// bias+SiLU / bias-only epilogues feed the SwiGLU), attention is attn.hip<64> with the 1025 real tokens masked
// inside a 1088-token padded layout.  An image owns TS = 1032 rows of the token matrices (1025 rounded up to 8):
// the 7 spare rows are zero-initialised, stay finite and are never read as keys (masked) or pooled.
// First version of this model: RoPE and SwiGLU-product + LayerNorm are separate HBM-bound kernels.
// Tested one launch at a time: eva_assemble_kernel (row-major and the blocked copy) and eva_colsum_kernel through hiptsdbg_eva_assemble /
// hiptsdbg_eva_colsum at the end of this file (tests/test_gpu_tokens.py: bit for bit; the column sums also chained into pool_ln_kernel
// against float64), the GEMM epilogues, LayerNorms, patch gather and attention through their own entries (tests/test_gpu_gemm_epi.py,
// test_gpu_rows.py, test_gpu_ln_fold.py, test_gpu_attention_exact.py), the whole forward against oracle/eva.py (tests/test_gpu_eva.py).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/hip_tagsearch_debug.h"
#include "vit_internal.h"
#include "dbg_buf.h"
#include "model_host.h"
#include "row_ln.h"
#include "patch_rows.h"

using namespace hipts;

namespace {

struct EvaLayer {
    DevBuf ln1_g, ln1_b, ln2_g, ln2_b;
    DevBuf qkv_w, qkv_b, proj_w, proj_b, gx_w, gx_b;     // gx: fc1_g | fc1_x rows interleaved per 32 hidden units
    // fc2 with the inner LayerNorm (mlp.norm) folded in: fc2(LN(p)) = rstd (W (gamma p)) - rstd mean u + c with
    // u[n] = sum_k W[n][k] gamma[k] (of the rounded operand values of W), c = W beta + b; the fc1 epilogue stores gamma p.
    // Built when all four tensors are set; the host copies stay so that any of them can be set again.
    DevBuf fc2_w, fc2_u, fc2_c, mn_g;
    // pre-LayerNorms folded into the GEMM epilogues (EPI_RESID_XG): W gamma and W beta + b of the GEMMs that consume norm1 / norm2
    DevBuf qkv_u, qkv_c, gx_u, gx_c;
    std::vector<float> h_fc2_w, h_fc2_b, h_mn_g, h_mn_b;
};

}  // namespace

struct hipts_eva {
    int device = 0;
    hipts_eva_config_t cfg{};
    int grid = 0, np = 0, T = 0, TS = 0, Tp = 0, PK = 0, HN = 0, HK = 0;
    std::vector<EvaLayer> layers;
    DevBuf patch_w, patch_b, cls, pos, fcn_g, fcn_b, head_w, head_b, rope;
    TensorLedger ledger;
    DevBuf img_in, a0, tmp, x, xn, q, k, v, att, g1, stat_part, rowstat, xstat, pool_part, pooled2, logits, probs;
    DevBuf x0, x_rm;               // blocked residual stream (GemmArgs::x_blocked): the assembled rows row-major for layer 0's LayerNorm, the last layer's rows row-major for the pool
    bool fold_ln = false, fold_dirty = true;      // as in the ViT forward (vit.hip)
    bool split_att = false;                       // cfg.operand_f16 bit 4 (HIPTS_OPERAND_SPLIT_ATT), as in the ViT forward
    DevBuf sk_ws;                                 // split-K workspaces of proj / fc2 (GemmArgs::sk_ws), one per sub-batch stream, zeroed once
    SubStreams<2> streams;
};

namespace {

// x[b*TS + 0] = cls + pos[0]; x[b*TS + 1 + t] = tmp[b*np + t] (conv + bias + pos[1 + t], from the GEMM epilogue);
// x[b*TS + T .. TS) = 0.   One thread per float4.
// xblk (optional): the same rows a second time in the residual stream's blocked layout, [m / 16][n / 16][m % 16][n % 16] (gemm_epi.h::x_off)
__global__ __launch_bounds__(256) void eva_assemble_kernel(const float* __restrict__ tmp, const float* __restrict__ cls,
                                                           const float* __restrict__ pos, float* __restrict__ x, int batch, int np, int TS,
                                                           int D, float* __restrict__ xblk) {
    const int dq = D >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)batch * TS * dq;
    if (idx >= total) return;
    const int c4 = (int)(idx % dq);
    const int r = (int)((idx / dq) % TS);
    const int64_t b = idx / ((int64_t)dq * TS);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r == 0) {
        const float4 a = reinterpret_cast<const float4*>(cls)[c4], p = reinterpret_cast<const float4*>(pos)[c4];
        v = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
    } else if (r <= np) {
        v = reinterpret_cast<const float4*>(tmp)[(b * np + (r - 1)) * dq + c4];
    }
    reinterpret_cast<float4*>(x)[idx] = v;
    if (xblk) {
        const int64_t m = idx / dq;
        *reinterpret_cast<float4*>(xblk + ((((m >> 4) * (int64_t)(D >> 4) + (c4 >> 2)) << 8) + (m & 15) * 16 + (c4 & 3) * 4)) = v;
    }
}

// part[b][split][:] = sum of the patch-token rows of split `split` of image b (grid (POOL_SPLITS, batch)): the whole chip
// reads the 4 MB an image's tokens occupy instead of one workgroup per image (312 -> ~20 us at batch 32).
constexpr int POOL_SPLITS = 16;
__global__ __launch_bounds__(256) void eva_colsum_kernel(const float* __restrict__ x, float* __restrict__ part, int np, int TS, int D) {
    const int split = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int per = (np + POOL_SPLITS - 1) / POOL_SPLITS;
    const int r0 = split * per, r1 = min(np, r0 + per);
    if (tid * 4 >= D) return;
    const float4* xb = reinterpret_cast<const float4*>(x + ((int64_t)b * TS + 1) * D) + tid;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const int dq = D >> 2;
#pragma unroll 8
    for (int r = r0; r < r1; ++r) {
        const float4 v = xb[(int64_t)r * dq];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    reinterpret_cast<float4*>(part + ((int64_t)b * POOL_SPLITS + split) * D)[tid] = acc;
}

// The two kernels' launch shapes, shared by the forward and the debug entries (hiptsdbg_eva_assemble, hiptsdbg_eva_colsum)
int launch_eva_assemble(const float* tmp, const float* cls, const float* pos, float* x, int batch, int np, int TS, int D, float* xblk, hipStream_t s) {
    const int64_t tot4 = (int64_t)batch * TS * (D / 4);
    eva_assemble_kernel<<<ceil_div(tot4, 256), 256, 0, s>>>(tmp, cls, pos, x, batch, np, TS, D, xblk);
    HIPTS_LAUNCH_CHECK();
    return HIPTS_OK;
}

int launch_eva_colsum(const float* x, float* part, int batch, int np, int TS, int D, hipStream_t s) {
    eva_colsum_kernel<<<dim3(POOL_SPLITS, batch), 256, 0, s>>>(x, part, np, TS, D);
    HIPTS_LAUNCH_CHECK();
    return HIPTS_OK;
}

// rows x cols float block -> 16-bit operand bits at row offset `row0` of a [*, ld] matrix that was allocated zeroed
int put_rows16(DevBuf& buf, const float* data, int rows, int cols, int row0, int ld, bool f16) {
    std::vector<uint16_t> h((size_t)rows * ld, 0);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) h[(size_t)r * ld + c] = f16 ? f32_to_f16_rne(data[(size_t)r * cols + c]) : f32_to_bf16_rne(data[(size_t)r * cols + c]);
    return upload(buf.as<uint16_t>() + (size_t)row0 * ld, h.data(), h.size() * 2);
}

int alloc_zero(DevBuf& buf, size_t bytes) {
    HIPTS_TRY(buf.alloc(bytes));
    HIPTS_HIP(hipMemset(buf.p, 0, bytes));
    return HIPTS_OK;
}

// The whole kernel sequence for images [i0, i0 + batch) on stream s (every buffer is indexed by image)
int eva_run_images(hipts_eva* h, const void* in_dev, bool is_u8, int i0, int batch, float* lg, float* pr, hipStream_t s, bool shared_chip,
                   int sub = 0) {
    const auto& c = h->cfg;
    const int S = c.image_size, D = c.dim, P = c.patch, H = c.heads, T = h->T, TS = h->TS, Tp = h->Tp, np = h->np;
    const bool f16 = (c.operand_f16 & 1) != 0;
    const int M = batch * TS;
    in_dev = (const char*)in_dev + (size_t)i0 * S * S * 3 * (is_u8 ? 1 : 4);
    const size_t r0 = (size_t)i0 * TS, qo = (size_t)i0 * H * Tp * 64;
    bf16_t* a0_p = h->a0.as<bf16_t>() + (size_t)i0 * np * 2 * h->PK;
    float* tmp_p = h->tmp.as<float>() + (size_t)i0 * np * D;
    // the fp32 residual stream as 16 x 16 blocks (round 5; csrc/gemm_epi.h::x_off, the ViT forward has the measurements): a sub-batch's
    // region starts at a multiple of 16 rows of its own (1032 rows per image: odd image offsets are not)
    static const bool xb_env = !(getenv("HIPTS_X_BLOCKED") && atoi(getenv("HIPTS_X_BLOCKED")) == 0);
    const bool xb = xb_env && h->fold_ln && D % 16 == 0;
    float* x = h->x.as<float>() + (xb ? ((r0 + 15) / 16 * 16 + (size_t)16 * sub) : r0) * D;
    float* x0 = xb ? h->x0.as<float>() + r0 * D : x;                // what eva_assemble_kernel writes row-major (layer 0's LayerNorm reads it)
    float* x_rm = h->x_rm.as<float>() + r0 * D;                     // the last layer's rows for the column sums
    bf16_t* xn = h->xn.as<bf16_t>() + r0 * D;
    bf16_t* q_p = h->q.as<bf16_t>() + qo;
    bf16_t* k_p = h->k.as<bf16_t>() + qo;
    bf16_t* v_p = h->v.as<bf16_t>() + qo;
    const int att_k = h->split_att ? 2 * D : D;
    bf16_t* att_p = h->att.as<bf16_t>() + r0 * att_k;
    bf16_t* g1_p = h->g1.as<bf16_t>() + r0 * h->HK;
    const int sblocks = (2 * h->HK + 255) / 256;                               // 256-column tiles of the fc1 launch: one partial (sum, sum of squares) pair per tile and row
    float* stat_p = h->stat_part.as<float>() + 2 * (size_t)sblocks * r0;      // [sblocks][M] float2, this sub-batch's region
    float* rowstat_p = h->rowstat.as<float>() + 2 * r0;
    bf16_t* pooled2_p = h->pooled2.as<bf16_t>() + (size_t)i0 * 2 * D;
    if (lg) lg += (size_t)i0 * c.num_classes;
    if (pr) pr += (size_t)i0 * c.num_classes;
    GemmArgs g;
    {
        const int64_t total = (int64_t)batch * np * P;
        const int blocks = ceil_div(total, 256);
        // patch matrix, hi | lo halves of the normalised pixel (K = 2 PK, PK = P*P*3 rounded up to 64; the pad columns stay zero as
        // allocated).  uint8: ToTensor and Normalize in float32 like the reference; float32: already BGR, the flip of tagging.py:243
        // lives in the weight permutation
        const PixelU8Affine from_u8{(const uint8_t*)in_dev};
        const PixelF32Planes<true> from_f32{(const float*)in_dev};
        HIPTS_LAUNCH_U8_F16(is_u8, f16, patch_gather_kernel, blocks, 256, 0, s, from_u8, from_f32, WindowPatch{P, h->PK}, a0_p, total, S, h->grid);
        g = gemm_args(f16, shared_chip);
        g.A = a0_p; g.W = h->patch_w.as<bf16_t>(); g.M = batch * np; g.N = D; g.K = 2 * h->PK;
        g.bias = h->patch_b.as<float>(); g.out_f32 = tmp_p; g.pos = h->pos.as<float>() + D; g.tokens = np; g.qscale = 1.0f;
        HIPTS_TRY(launch_gemm(EPI_PATCH, g, s));
        HIPTS_TRY(launch_eva_assemble(tmp_p, h->cls.as<float>(), h->pos.as<float>(), x0, batch, np, TS, D, xb ? x : nullptr, s));
    }
    // pre-LayerNorms folded into the neighbouring GEMM epilogues, as in the ViT forward: the residual GEMM writes gamma * x (16-bit)
    // and the per-tile row sums of x; the consumer finishes the statistics per tile and applies rstd / mean / beta
    const bool fold = h->fold_ln;
    const int xblocks = (D + 255) / 256;
    float* xstat_p = fold ? h->xstat.as<float>() + 2 * (size_t)xblocks * r0 : nullptr;
    auto folded = [&](GemmArgs& ga, const float* u, const float* cvec) {
        ga.stat_in = xstat_p; ga.stat_in_blocks = xblocks; ga.stat_in_stride = M; ga.ln_dim = D; ga.ln_eps = c.ln_eps;
        ga.col_u = u; ga.bias = cvec;
    };
    for (int li = 0; li < c.depth; ++li) {
        EvaLayer& L = h->layers[li];
        const bool ln1_folded = fold && li > 0;
        if (!ln1_folded) HIPTS_TRY(launch_layernorm(li == 0 ? x0 : x, L.ln1_g.as<float>(), L.ln1_b.as<float>(), xn, M, D, c.ln_eps, f16, s));
        g = gemm_args(f16, shared_chip);
        g.A = xn; g.W = L.qkv_w.as<bf16_t>(); g.M = M; g.N = 3 * D; g.K = D; g.bias = L.qkv_b.as<float>();
        g.out_bf16 = q_p; g.out2_bf16 = k_p; g.out3_bf16 = v_p;       // one launch: q and k rotated, v as it is, all [image][head][token][64]
        g.tokens = TS; g.tokens_pad = Tp; g.heads = H; g.dim = D;
        g.qscale = 0.125f * 1.4426950408889634f;           // 64^-0.5 * log2(e); linear, so it commutes with the rotation
        g.rope = h->rope.as<float>(); g.rope_tokens = np;  // 2-D rotary embedding on the fp32 result, in the epilogue
        if (ln1_folded) folded(g, L.qkv_u.as<float>(), L.qkv_c.as<float>());
        HIPTS_TRY(launch_gemm(EPI_QK_ROPE, g, s));
        HIPTS_TRY(launch_attention2(q_p, k_p, v_p, att_p, batch, H, T, Tp, f16, s, TS, 0, h->split_att ? 1 : 0, split_lo_scale(f16)));
        g = gemm_args(f16, shared_chip);
        g.A = att_p; g.W = L.proj_w.as<bf16_t>(); g.M = M; g.N = D; g.K = att_k; g.bias = L.proj_b.as<float>(); g.out_f32 = x;
        g.x_blocked = xb ? 1 : 0;
        g.sk_ws = h->sk_ws.as<char>() + (size_t)sub * GEMM_SK_WS_BYTES; g.sk_ws_bytes = GEMM_SK_WS_BYTES;      // split-K when the launch under-fills the chip
        if (fold) {
            g.out_bf16 = xn; g.ln_gamma = L.ln2_g.as<float>(); g.stat_part = xstat_p; g.stat_stride = M;
            HIPTS_TRY(launch_gemm(EPI_RESID_XG, g, s));
        } else {
            HIPTS_TRY(launch_gemm(EPI_RESID, g, s));
            HIPTS_TRY(launch_layernorm(x, L.ln2_g.as<float>(), L.ln2_b.as<float>(), xn, M, D, c.ln_eps, f16, s));
        }
        g = gemm_args(f16, shared_chip);
        // fc1_g and fc1_x in one launch (rows interleaved per 32 hidden units); silu(gate) * value in the epilogue
        g.A = xn; g.W = L.gx_w.as<bf16_t>(); g.M = M; g.N = 2 * h->HK; g.K = D; g.bias = L.gx_b.as<float>();
        g.out_bf16 = g1_p; g.ld_out = h->HK;
        g.stat_part = stat_p; g.stat_stride = M;             // row sums of the product for the LayerNorm folded into fc2
        g.ln_gamma = L.mn_g.as<float>();
        if (fold) folded(g, L.gx_u.as<float>(), L.gx_c.as<float>());
        HIPTS_TRY(launch_gemm(EPI_SWIGLU, g, s));
        // (round 3) no rowstat kernel between the two GEMMs: the SwiGLU epilogue leaves ONE partial pair per (256-column tile, row) -- the four
        // waves of a row meet in LDS -- and fc2's workgroups finish the 22 pairs of their tile's rows into an LDS table before their epilogue
        g = gemm_args(f16, shared_chip);
        g.A = g1_p; g.W = L.fc2_w.as<bf16_t>(); g.M = M; g.N = D; g.K = h->HK; g.bias = L.fc2_c.as<float>(); g.out_f32 = x;
        g.x_blocked = xb ? 1 : 0;
        g.sk_ws = h->sk_ws.as<char>() + (size_t)sub * GEMM_SK_WS_BYTES; g.sk_ws_bytes = GEMM_SK_WS_BYTES;
        static const bool rowstat_kernel = getenv("HIPTS_EVA_ROWSTAT_KERNEL") && atoi(getenv("HIPTS_EVA_ROWSTAT_KERNEL"));      // A/B: finish the pairs in a kernel of its own
        if (rowstat_kernel) {
            HIPTS_TRY(launch_rowstat(stat_p, rowstat_p, M, M, sblocks, c.mlp_hidden, c.ln_eps, s));
            g.rowstat = rowstat_p;
        } else {
            g.stat_in = stat_p; g.stat_in_blocks = sblocks; g.stat_in_stride = M; g.ln_dim = c.mlp_hidden; g.ln_eps = c.ln_eps;
        }
        g.col_u = L.fc2_u.as<float>();
        if (fold && li + 1 < c.depth) {      // the next layer's norm1 prepared here
            g.out_bf16 = xn; g.ln_gamma = h->layers[li + 1].ln1_g.as<float>(); g.stat_part = xstat_p; g.stat_stride = M;
            HIPTS_TRY(launch_gemm(EPI_RESID_XGI, g, s));
        } else {
            if (xb) g.resid_rowmajor_out = x_rm;        // the forward's last residual launch (fold: the last layer): rows for the column sums
            HIPTS_TRY(launch_gemm(EPI_RESID_ROWSTAT, g, s));
        }
    }
    float* part_p = h->pool_part.as<float>() + (size_t)i0 * POOL_SPLITS * D;
    HIPTS_TRY(launch_eva_colsum(xb ? x_rm : x, part_p, batch, np, TS, D, s));
    // pooled2 = hi | lo of fc_norm(mean over the patch tokens): the POOL_SPLITS partial rows summed, divided by the np tokens they cover
    HIPTS_LAUNCH_F16(f16, pool_ln_kernel, batch, 1024, 0, s, part_p, h->fcn_g.as<float>(), h->fcn_b.as<float>(), PooledHiLo{pooled2_p}, POOL_SPLITS, D,
                     c.ln_eps, 0, np);
    g = gemm_args(f16, shared_chip);
    g.A = pooled2_p; g.W = h->head_w.as<bf16_t>(); g.M = batch; g.N = c.num_classes; g.K = 2 * D;
    g.sk_ws = h->sk_ws.as<char>() + (size_t)sub * GEMM_SK_WS_BYTES; g.sk_ws_bytes = GEMM_SK_WS_BYTES;      // split-K: 43 tiles on 256 CUs
    g.bias = h->head_b.as<float>(); g.out_f32 = lg; g.out2_f32 = pr;
    HIPTS_TRY(launch_gemm(EPI_HEAD, g, s));
    return HIPTS_OK;
}

int eva_forward_impl(hipts_eva* h, const void* input, int in_memspace, bool is_u8, int batch, float* logits_out, float* probs_out,
                     int out_memspace, hipStream_t s) {
    HIPTS_REQUIRE(h && input && batch >= 1, "hipts_eva_forward: bad arguments");
    HIPTS_REQUIRE(batch <= h->cfg.max_batch, "batch %d exceeds max_batch %d", batch, h->cfg.max_batch);
    HIPTS_TRY(h->ledger.require_complete("hipts_eva_forward"));
    HIPTS_TRY(use_device(h->device));
    const auto& c = h->cfg;
    const int S = c.image_size;
    const void* in_dev = nullptr;
    HIPTS_TRY(stage_input(h->img_in, input, in_memspace, (size_t)batch * S * S * 3 * (is_u8 ? 1 : 4), s, &in_dev));
    const bool dev_out = out_memspace == HIPTS_DEVICE;
    // deliberate: logits are always computed, into the handle's own buffer when the caller passes none (ConvNeXt / SwinV2 pass null on)
    float* lg = (dev_out && logits_out) ? logits_out : h->logits.as<float>();
    float* pr = (probs_out || !dev_out) ? ((dev_out && probs_out) ? probs_out : h->probs.as<float>()) : nullptr;
    if (h->fold_ln && h->fold_dirty) {
        const bool f16w = (c.operand_f16 & 1) != 0;
        for (auto& L : h->layers) {
            HIPTS_TRY(launch_fold_ln(L.qkv_w.as<bf16_t>(), f16w, L.ln1_g.as<float>(), L.ln1_b.as<float>(), L.qkv_b.as<float>(), L.qkv_u.as<float>(),
                                     L.qkv_c.as<float>(), 3 * c.dim, c.dim, s));
            HIPTS_TRY(launch_fold_ln(L.gx_w.as<bf16_t>(), f16w, L.ln2_g.as<float>(), L.ln2_b.as<float>(), L.gx_b.as<float>(), L.gx_u.as<float>(),
                                     L.gx_c.as<float>(), 2 * h->HK, c.dim, s));
        }
        h->fold_dirty = false;
    }
    static const int want_streams = getenv("HIPTS_EVA_STREAMS") ? atoi(getenv("HIPTS_EVA_STREAMS")) : 2;
    static const int min_sub = getenv("HIPTS_EVA_MINSUB") ? atoi(getenv("HIPTS_EVA_MINSUB")) : 5;      // images per sub-batch needed to split (the reference batch of 10 as two halves: 980 -> 1005 images/s)
    const int ns = std::min({want_streams, 2, batch / (min_sub > 0 ? min_sub : 5)});
    // two sub-batches on two internal streams, as in the ViT forward (partial last rounds of the persistent GEMMs)
    HIPTS_TRY(run_split(h->streams, s, batch, ns, [&](int i0, int nb, hipStream_t st, bool shared_chip, int sub) {
        return eva_run_images(h, in_dev, is_u8, i0, nb, lg, pr, st, shared_chip, sub);
    }));
    if (!dev_out) HIPTS_TRY(read_back(s, (size_t)batch * c.num_classes * 4, logits_out, lg, probs_out, pr));
    return HIPTS_OK;
}

}  // namespace

extern "C" {

int hipts_eva_create(const hipts_eva_config_t* cfg, int device, hipts_eva_t** out) {
    HIPTS_REQUIRE(cfg && out, "hipts_eva_create: null argument");
    HIPTS_REQUIRE(cfg->patch >= 1 && cfg->image_size % cfg->patch == 0, "image_size %d must be a multiple of patch %d", cfg->image_size, cfg->patch);
    HIPTS_REQUIRE(cfg->dim % 64 == 0 && cfg->dim <= 1024 && cfg->heads * 64 == cfg->dim, "dim %d / heads %d: head_dim must be 64, dim <= 1024", cfg->dim, cfg->heads);
    HIPTS_REQUIRE(cfg->mlp_hidden >= 8 && cfg->mlp_hidden <= 4096, "mlp_hidden %d must be 8 .. 4096", cfg->mlp_hidden);
    HIPTS_REQUIRE(cfg->depth >= 1 && cfg->num_classes >= 1 && cfg->max_batch >= 1 && cfg->rope_ref_grid >= 1, "bad configuration");
    HIPTS_TRY(use_device(device));
    auto* h = new hipts_eva();
    h->device = device;
    h->cfg = *cfg;
    h->split_att = (cfg->operand_f16 & HIPTS_OPERAND_SPLIT_ATT) != 0;
    const int D = cfg->dim, B = cfg->max_batch;
    h->grid = cfg->image_size / cfg->patch;
    h->np = h->grid * h->grid;
    h->T = h->np + 1;
    h->TS = round_up(h->T, 8);
    h->Tp = round_up(h->T, 64);
    h->PK = round_up(cfg->patch * cfg->patch * 3, 64);
    h->HN = round_up(cfg->mlp_hidden, 16);
    h->HK = round_up(cfg->mlp_hidden, 64);
    h->fold_ln = cfg->dim % 64 == 0 && !getenv("HIPTS_GEMM") && !(getenv("HIPTS_LN_FOLD") && atoi(getenv("HIPTS_LN_FOLD")) == 0);
    h->layers.resize(cfg->depth);
    const size_t M = (size_t)B * h->TS;
    const size_t qk = (size_t)B * cfg->heads * h->Tp * 64 * 2;
    int st = 0;
    if ((st = alloc_zero(h->a0, (size_t)B * h->np * 2 * h->PK * 2)) || (st = h->tmp.alloc((size_t)B * h->np * D * 4)) || (st = alloc_zero(h->x, (M + 16 * 9) * D * 4)) || (st = h->x0.alloc(M * D * 4)) || (st = h->x_rm.alloc(M * D * 4)) ||
        (st = alloc_zero(h->xn, M * D * 2)) || (st = alloc_zero(h->q, qk)) || (st = alloc_zero(h->k, qk)) || (st = alloc_zero(h->v, qk)) ||
        (st = alloc_zero(h->att, M * D * 2 * (h->split_att ? 2 : 1))) || (st = alloc_zero(h->g1, M * h->HK * 2)) ||
        (st = h->stat_part.alloc((size_t)((2 * h->HK + 255) / 256) * M * 8)) || (st = h->xstat.alloc((size_t)((D + 255) / 256) * M * 8)) || (st = h->rowstat.alloc(M * 8)) || (st = h->pooled2.alloc((size_t)B * 2 * D * 2)) || (st = h->pool_part.alloc((size_t)B * 16 * D * 4)) ||
        (st = h->logits.alloc((size_t)B * cfg->num_classes * 4)) || (st = h->probs.alloc((size_t)B * cfg->num_classes * 4)) ||
        (st = alloc_zero(h->sk_ws, 2 * GEMM_SK_WS_BYTES))) {      // split-K tickets start at zero (the kernels leave them so)
        delete h;
        return st;
    }
    // RoPE tables (timm RotaryEmbeddingCat, in_pixels = False, positions rescaled to the reference grid)
    {
        const int nb = 16;      // head_dim / 4
        std::vector<float> sn((size_t)h->np * 64), cs((size_t)h->np * 64), tab((size_t)h->np * 64);
        for (int y = 0; y < h->grid; ++y)
            for (int xx = 0; xx < h->grid; ++xx)
                for (int ax = 0; ax < 2; ++ax)
                    for (int i = 0; i < nb; ++i) {
                        const float band = 1.0f / powf(10000.0f, (float)i / (float)nb);
                        const float t = (float)(ax == 0 ? y : xx) / (float)h->grid * (float)cfg->rope_ref_grid;
                        const float a = t * band;
                        const size_t o = ((size_t)y * h->grid + xx) * 64 + (size_t)(ax * nb + i) * 2;
                        sn[o] = sn[o + 1] = sinf(a);
                        cs[o] = cs[o + 1] = cosf(a);
                    }
        for (size_t t = 0; t < (size_t)h->np; ++t)
            for (int i = 0; i < 32; ++i) {          // (sin, cos) of column pair (2i, 2i+1)
                tab[t * 64 + 2 * i] = sn[t * 64 + 2 * i];
                tab[t * 64 + 2 * i + 1] = cs[t * 64 + 2 * i];
            }
        if ((st = upload_f32(h->rope, tab.data(), tab.size()))) {
            delete h;
            return st;
        }
    }
    for (auto& L : h->layers) {
        // assembled from three tensors each: allocate zeroed now (k has no bias; pad rows / columns stay zero)
        if ((st = alloc_zero(L.qkv_w, (size_t)(round_up(2 * D, 256) + round_up(D, 256) + 256) * D * 2)) || (st = alloc_zero(L.qkv_b, (size_t)3 * D * 4)) ||
            (st = alloc_zero(L.gx_w, (size_t)round_up(2 * h->HK, 256) * D * 2)) || (st = alloc_zero(L.gx_b, (size_t)round_up(2 * h->HK, 256) * 4)) ||
            (st = alloc_zero(L.fc2_w, (size_t)round_up(D, 256) * h->HK * 2)) || (st = alloc_zero(L.fc2_u, (size_t)round_up(D, 256) * 4)) ||
            (st = alloc_zero(L.fc2_c, (size_t)round_up(D, 256) * 4)) ||
            (st = alloc_zero(L.mn_g, (size_t)h->HK * 4)) || (st = alloc_zero(L.qkv_u, (size_t)3 * D * 4)) || (st = alloc_zero(L.qkv_c, (size_t)3 * D * 4)) ||
            (st = alloc_zero(L.gx_u, (size_t)2 * h->HK * 4)) || (st = alloc_zero(L.gx_c, (size_t)2 * h->HK * 4))) {
            delete h;
            return st;
        }
    }
    if ((st = alloc_zero(h->patch_w, (size_t)round_up(D, 256) * 2 * h->PK * 2))) {
        delete h;
        return st;
    }
    auto need = [&](const std::string& k) { h->ledger.need(k); };
    for (const char* k : {"patch_embed.proj.weight", "patch_embed.proj.bias", "cls_token", "pos_embed", "fc_norm.weight", "fc_norm.bias", "head.weight",
                          "head.bias"})
        need(k);
    for (int i = 0; i < cfg->depth; ++i) {
        const std::string p = "blocks." + std::to_string(i) + ".";
        for (const char* k : {"norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias", "attn.q_proj.weight", "attn.q_proj.bias", "attn.k_proj.weight",
                              "attn.v_proj.weight", "attn.v_proj.bias", "attn.proj.weight", "attn.proj.bias", "mlp.fc1_g.weight", "mlp.fc1_g.bias",
                              "mlp.fc1_x.weight", "mlp.fc1_x.bias", "mlp.norm.weight", "mlp.norm.bias", "mlp.fc2.weight", "mlp.fc2.bias"})
            need(p + k);
    }
    *out = h;
    return HIPTS_OK;
}

int hipts_eva_destroy(hipts_eva_t* h) {
    if (h) {
        (void)hipSetDevice(h->device);
        (void)hipDeviceSynchronize();
        delete h;
    }
    return HIPTS_OK;
}

int hipts_eva_set_tensor(hipts_eva_t* h, const char* key_c, const float* data, int64_t numel) {
    HIPTS_REQUIRE(h && key_c && data, "hipts_eva_set_tensor: null argument");
    HIPTS_TRY(use_device(h->device));
    const std::string key(key_c);
    const auto& c = h->cfg;
    const bool f16 = (c.operand_f16 & 1) != 0;
    const int D = c.dim, P = c.patch, Hd = c.mlp_hidden, C = c.num_classes;
    int st = HIPTS_OK, li = 0;
    std::string t;
    if (key == "patch_embed.proj.weight") {
        EXPECT_NUMEL((int64_t)D * 3 * P * P);
        const std::vector<float> w2 = stem_weight_hilo(data, D, P * P, h->PK, true);      // BGR flip; the hi | lo halves of patch_gather_kernel
        st = put_rows16(h->patch_w, w2.data(), D, 2 * h->PK, 0, 2 * h->PK, f16);
    } else if (key == "patch_embed.proj.bias") { EXPECT_NUMEL(D); st = upload_f32(h->patch_b, data, D); }
    else if (key == "cls_token") { EXPECT_NUMEL(D); st = upload_f32(h->cls, data, D); }
    else if (key == "pos_embed") { EXPECT_NUMEL((int64_t)h->T * D); st = upload_f32(h->pos, data, (size_t)h->T * D); }
    else if (key == "fc_norm.weight") { EXPECT_NUMEL(D); st = upload_f32(h->fcn_g, data, D); }
    else if (key == "fc_norm.bias") { EXPECT_NUMEL(D); st = upload_f32(h->fcn_b, data, D); }
    else if (key == "head.bias") { EXPECT_NUMEL(C); st = upload_f32(h->head_b, data, C); }
    else if (key == "head.weight") {
        EXPECT_NUMEL((int64_t)C * D);
        st = upload_matrix16_dup(h->head_w, data, C, D, round_up(C, 256), f16);
    } else if (parse_indexed(key, "blocks.", &li, &t)) {
        if (li < 0 || li >= c.depth) return set_error(HIPTS_ERR_INVALID, "tensor %s: block out of range", key_c);
        EvaLayer& L = h->layers[li];
        if (t == "norm1.weight") { EXPECT_NUMEL(D); st = upload_f32(L.ln1_g, data, D); }
        else if (t == "norm1.bias") { EXPECT_NUMEL(D); st = upload_f32(L.ln1_b, data, D); }
        else if (t == "norm2.weight") { EXPECT_NUMEL(D); st = upload_f32(L.ln2_g, data, D); }
        else if (t == "norm2.bias") { EXPECT_NUMEL(D); st = upload_f32(L.ln2_b, data, D); }
        else if (t == "attn.q_proj.weight") { EXPECT_NUMEL((int64_t)D * D); st = put_rows16(L.qkv_w, data, D, D, 0, D, f16); }
        else if (t == "attn.k_proj.weight") { EXPECT_NUMEL((int64_t)D * D); st = put_rows16(L.qkv_w, data, D, D, D, D, f16); }
        else if (t == "attn.v_proj.weight") { EXPECT_NUMEL((int64_t)D * D); st = put_rows16(L.qkv_w, data, D, D, 2 * D, D, f16); }
        else if (t == "attn.q_proj.bias") { EXPECT_NUMEL(D); st = upload(L.qkv_b.as<float>(), data, (size_t)D * 4); }
        else if (t == "attn.v_proj.bias") { EXPECT_NUMEL(D); st = upload(L.qkv_b.as<float>() + 2 * D, data, (size_t)D * 4); }
        else if (t == "attn.proj.weight") {
            EXPECT_NUMEL((int64_t)D * D);
            if (h->split_att) {      // [W | W] against the (hi | lo) halves of the attention output
                st = upload_matrix16_dup(L.proj_w, data, D, D, round_up(D, 256), f16, split_lo_scale(f16));      // the low halves arrive multiplied by the scale
            } else {
                st = upload_matrix16(L.proj_w, data, D, D, round_up(D, 256), f16);
            }
        }
        else if (t == "attn.proj.bias") { EXPECT_NUMEL(D); st = upload_f32(L.proj_b, data, D); }
        else if (t == "mlp.fc1_g.weight" || t == "mlp.fc1_x.weight") {
            // hidden unit u -> physical row 64 (u / 32) + (u % 32), + 32 for the value half (EPI_SWIGLU)
            EXPECT_NUMEL((int64_t)Hd * D);
            const int half = t == "mlp.fc1_x.weight" ? 32 : 0;
            for (int u0 = 0; u0 < Hd && !st; u0 += 32)
                st = put_rows16(L.gx_w, data + (size_t)u0 * D, std::min(32, Hd - u0), D, (u0 / 32) * 64 + half, D, f16);
        }
        else if (t == "mlp.fc1_g.bias" || t == "mlp.fc1_x.bias") {
            EXPECT_NUMEL(Hd);
            const int half = t == "mlp.fc1_x.bias" ? 32 : 0;
            for (int u0 = 0; u0 < Hd && !st; u0 += 32)
                st = upload(L.gx_b.as<float>() + (u0 / 32) * 64 + half, data + u0, (size_t)std::min(32, Hd - u0) * 4);
        }
        else if (t == "mlp.norm.weight" || t == "mlp.norm.bias" || t == "mlp.fc2.weight" || t == "mlp.fc2.bias") {
            if (t == "mlp.norm.weight") { EXPECT_NUMEL(Hd); L.h_mn_g.assign(data, data + Hd); }
            else if (t == "mlp.norm.bias") { EXPECT_NUMEL(Hd); L.h_mn_b.assign(data, data + Hd); }
            else if (t == "mlp.fc2.weight") { EXPECT_NUMEL((int64_t)D * Hd); L.h_fc2_w.assign(data, data + (size_t)D * Hd); }
            else { EXPECT_NUMEL(D); L.h_fc2_b.assign(data, data + D); }
            if (!L.h_mn_g.empty() && !L.h_mn_b.empty() && !L.h_fc2_w.empty() && !L.h_fc2_b.empty()) {
                // u and c from the rounded operand values of W, so that the mean term cancels against what the MFMA sums
                std::vector<float> u(D), cc(D);
                for (int n = 0; n < D; ++n) {
                    double su = 0.0, sc = 0.0;
                    for (int k = 0; k < Hd; ++k) {
                        const float w = L.h_fc2_w[(size_t)n * Hd + k];
                        float r;
                        if (f16) r = f16_bits_to_f32(f32_to_f16_rne(w));
                        else { const uint32_t bits = (uint32_t)f32_to_bf16_rne(w) << 16; memcpy(&r, &bits, 4); }
                        su += (double)r * (double)L.h_mn_g[k];
                        sc += (double)r * (double)L.h_mn_b[k];
                    }
                    u[n] = (float)su;
                    cc[n] = (float)(sc + (double)L.h_fc2_b[n]);
                }
                st = put_rows16(L.fc2_w, L.h_fc2_w.data(), D, Hd, 0, h->HK, f16);
                if (!st) st = upload(L.mn_g.as<float>(), L.h_mn_g.data(), (size_t)Hd * 4);      // pad entries stay zero
                if (!st) st = upload(L.fc2_u.as<float>(), u.data(), (size_t)D * 4);
                if (!st) st = upload(L.fc2_c.as<float>(), cc.data(), (size_t)D * 4);
            }
        }
        else return set_error(HIPTS_ERR_INVALID, "unknown tensor key %s", key_c);
    } else return set_error(HIPTS_ERR_INVALID, "unknown tensor key %s", key_c);
    if (st) return st;
    h->fold_dirty = true;
    h->ledger.mark_set(key);
    return HIPTS_OK;
}

int hipts_eva_forward_u8(hipts_eva_t* h, const uint8_t* images, int images_memspace, int batch, float* logits_out, float* probs_out,
                         int out_memspace, void* stream) {
    return eva_forward_impl(h, images, images_memspace, true, batch, logits_out, probs_out, out_memspace, (hipStream_t)stream);
}

int hipts_eva_forward_f32(hipts_eva_t* h, const float* x, int x_memspace, int batch, float* logits_out, float* probs_out, int out_memspace,
                          void* stream) {
    return eva_forward_impl(h, x, x_memspace, false, batch, logits_out, probs_out, out_memspace, (hipStream_t)stream);
}

int hipts_eva_flops_per_image(const hipts_eva_t* h, double* flops) {
    HIPTS_REQUIRE(h && flops, "null argument");
    const auto& c = h->cfg;
    const double T = h->T, D = c.dim, Hd = c.mlp_hidden;
    double f = 2.0 * h->np * D * (double)(c.patch * c.patch * 3);
    f += c.depth * (2.0 * T * 3 * D * D + 4.0 * T * T * D + 2.0 * T * D * D + 2.0 * T * D * Hd * 3);
    f += 2.0 * D * c.num_classes;
    *flops = f;
    return HIPTS_OK;
}

// Debug / test entries (include/hip_tagsearch_debug.h; tests/test_gpu_tokens.py): eva_assemble_kernel and eva_colsum_kernel once each,
// launched as the forward launches them, every output filled with `fill` before and copied back whole.
int hiptsdbg_eva_assemble(const float* tmp, uint64_t tmp_bytes, const float* cls, const float* pos, int batch, int np, int TS, int D, int blocked, int fill,
                          float* x, uint64_t x_bytes, float* xblk, uint64_t xblk_bytes) {
    const char* who = "hiptsdbg_eva_assemble";
    HIPTS_REQUIRE(tmp && cls && pos && x && (xblk || xblk_bytes == 0), "%s: null argument", who);
    HIPTS_REQUIRE(batch >= 1 && batch <= 4096 && np >= 1 && np <= (1 << 16) && TS >= np + 1 && TS <= (1 << 16), "%s: unsupported shape", who);
    HIPTS_REQUIRE(D >= 4 && D % 4 == 0 && D <= 4096, "%s: D=%d must be a multiple of 4", who, D);
    HIPTS_REQUIRE(!blocked || D % 16 == 0, "%s: the blocked copy needs D %% 16 == 0", who);
    HIPTS_REQUIRE(tmp_bytes >= (uint64_t)batch * np * D * 4, "%s: tmp does not cover the launch", who);
    HIPTS_TRY(use_device(0));
    const uint64_t M = (uint64_t)batch * TS;
    DevBuf td, cd, pd, xd, bd;
    HIPTS_TRY(dbg_guarded(xd, x_bytes, M * D * 4, fill, who, "x"));
    HIPTS_TRY(dbg_guarded(bd, xblk_bytes, blocked ? (M + 15) / 16 * 16 * D * 4 : 0, fill, who, "blocked"));      // the last 16-row block may be ragged
    HIPTS_TRY(dbg_put(td, tmp, tmp_bytes));
    HIPTS_TRY(dbg_put(cd, cls, (size_t)D * 4));
    HIPTS_TRY(dbg_put(pd, pos, (size_t)D * 4));
    HIPTS_TRY(launch_eva_assemble(td.as<float>(), cd.as<float>(), pd.as<float>(), xd.as<float>(), batch, np, TS, D, blocked ? bd.as<float>() : nullptr, nullptr));
    HIPTS_HIP(hipDeviceSynchronize());
    HIPTS_TRY(dbg_fetch(x, xd, x_bytes, who));
    return dbg_fetch(xblk, bd, xblk_bytes, who);
}

int hiptsdbg_eva_colsum(const float* x, uint64_t x_bytes, int batch, int np, int TS, int D, int fill, float* part, uint64_t part_bytes) {
    const char* who = "hiptsdbg_eva_colsum";
    HIPTS_REQUIRE(x && part, "%s: null argument", who);
    HIPTS_REQUIRE(batch >= 1 && batch <= 4096 && np >= 1 && np <= (1 << 16) && TS >= np + 1 && TS <= (1 << 16), "%s: unsupported shape", who);
    HIPTS_REQUIRE(D >= 4 && D % 4 == 0 && D <= 1024, "%s: D=%d must be a multiple of 4, at most 1024", who, D);
    HIPTS_REQUIRE(x_bytes >= (uint64_t)batch * TS * D * 4, "%s: x does not cover the launch", who);
    HIPTS_TRY(use_device(0));
    DevBuf xd, pd;
    HIPTS_TRY(dbg_guarded(pd, part_bytes, (uint64_t)batch * POOL_SPLITS * D * 4, fill, who, "partial"));
    HIPTS_TRY(dbg_put(xd, x, x_bytes));
    HIPTS_TRY(launch_eva_colsum(xd.as<float>(), pd.as<float>(), batch, np, TS, D, nullptr));
    HIPTS_HIP(hipDeviceSynchronize());
    return dbg_fetch(part, pd, part_bytes, who);
}

}  // extern "C"
