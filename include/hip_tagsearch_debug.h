/* hip_tagsearch_debug.h -- diagnostic entry points of libhip_tagsearch.so.
 *
 * NOT part of the drop-in boundary (include/hip_tagsearch.h): nothing in the reference binds to these.  They exist for
 * the kernel tests (tests/test_gpu_gemm.py), the standalone GEMM timers (tools/gemm_bench.py) and bench.py's clock probe.
 * They may change or disappear between versions; HIPTS_ABI_VERSION does not cover them.
 */
#ifndef HIP_TAGSEARCH_DEBUG_H
#define HIP_TAGSEARCH_DEBUG_H

#include <stddef.h>
#include <stdint.h>

#include "hip_tagsearch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Average device time of `iters` back-to-back launches of the bf16 GEMM [M,K] x [N,K]^T with epilogue `epi`
 * (the GemmEpilogue enumerator of csrc/vit_internal.h) on synthetic operands. */
int hiptsdbg_gemm_time(int M, int N, int K, int epi, int iters, float* ms_out);
/* The same, and the shader clock (GHz) held inside the main loop of the stamped workgroup (s_memtime against the
 * 100 MHz s_memrealtime); 0 when the library was built without HIPTS_GEMM_STAMPS support for that epilogue. */
int hiptsdbg_gemm_clock(int M, int N, int K, int epi, int iters, float* ms_out, float* loop_ghz);
/* One GEMM launch through the 8-wave loop (csrc/gemm.hip) and through the 4-wave loop (csrc/gemm4.hip) on the same random operands: number
 * of output bytes that differ (must be 0) and the average launch time each way (ms_out[0]: 8-wave, ms_out[1]: 4-wave).  epi: 4 (GELU),
 * 1 (QK; N % 3 == 0: fused q | k | v), 13 (RESID_XG); M % 256 == 0, M % 784 == 0, N % 256 == 0, K % 128 == 0. */
int hiptsdbg_gemm_q4_compare(int M, int N, int K, int epi, int f16, int iters, long long* mismatch_out, float* ms_out);
/* y_host[i] = the GELU of the fc1 epilogue (csrc/gemm.hip gelu_f4) of x_host[i]; n % 4 == 0; tanh_form as hipts_vit_config::gelu_tanh. */
int hiptsdbg_gelu(const float* x_host, int n, int tanh_form, float* y_host);
/* The depthwise 7 x 7 (padding 3) of the CCIP encoder's SepConv blocks on its own: in / out IEEE-half bit patterns [batch][H][H][C] (host),
 * w float32 [C][49]; mode 0: the float32-FMA kernel, 1: the matrix-core kernel with its tile chosen by H, 2 / 3: its 32- / 48-column tile;
 * ms_out: average device time of `iters` launches after one untimed launch. */
int hiptsdbg_dwconv7(const uint16_t* in_f16, const float* w, uint16_t* out_f16, int batch, int H, int C, int mode, int iters, float* ms_out);
/* Phase time stamps (100 MHz) of one workgroup of the matrix-core kernel's last launch; zeros unless csrc/ccip.hip was built with
 * -DHIPTS_DW_STAMPS=<workgroup> (tools/dwconv_stamps.py). */
int hiptsdbg_dwconv7_stamps(unsigned long long* host, int n);
/* The ConvNeXt forward's float32 residual stream [batch][H*H][dims[stage]] after the last block of `stage` (0..3), from host
 * float32 input in the layout of hipts_convnext_forward_f32: places a parity failure in the network. */
int hiptsdbg_convnext_stream(hipts_convnext_t* h, const float* x_host, int batch, int stage, float* out_host);
/* The SwinV2 forward's float32 residual stream [batch][H*H][dims[stage]] after the last block of `stage` (0..3), from host float32
 * input in the layout of hipts_swinv2_forward_f32. */
int hiptsdbg_swinv2_stream(hipts_swinv2_t* h, const float* x_host, int batch, int stage, float* out_host);
/* SwinV2 window attention on its own (csrc/swin_attn.hip).  Host float32 q, k, v [batch][side*side][heads*32] in raster order (q, k
 * as they leave the qkv Linear, before F.normalize), logit_scale [heads] (before the clamp at ln 100), cpb [heads][(2w-1)^2] (the
 * table 16 sigmoid(cpb_mlp(.)), indexed (dy + w - 1) (2w - 1) + dx + w - 1 for query minus key offsets); the windows are shifted
 * by `shift` (0: none).  out: float32 [batch][side*side][heads*32], the kernel's 16-bit output widened. */
int hiptsdbg_swinv2_window_attention(const float* q, const float* k, const float* v, const float* logit_scale, const float* cpb, int batch,
                                     int heads, int side, int window, int shift, int operand_f16, float* out);
/* The fused MLP of the CCIP encoder's stages 0-1 on its own (csrc/mlp.hip): x[m] = rs * x[m] + StarReLU(xn[m] W1^T) W2^T, xn_out[m] = LayerNorm(x[m]) * gamma.
 * Host arrays: xn / xn_out IEEE-half bits [M][C], w1 [4C][C], w2 [C][4C], x [M][C] in / out, res_scale / gamma [C] or null; C = 128 or 256;
 * ms_out: average device time of iters - 1 launches (iters >= 2); waves: 4 / 8 waves per workgroup, 0 = chosen by the size of the launch. */
int hiptsdbg_mlp_fused(const uint16_t* xn, const float* w1, const float* w2, float* x, const float* res_scale, const float* gamma, uint16_t* xn_out,
                       int M, int C, float star_s, float star_b, float eps, int iters, float* ms_out, int waves);
/* Phase time stamps (100 MHz) of one wave of the fused MLP kernel's last launch; zeros unless csrc/mlp.hip was built with
 * -DHIPTS_MLP_STAMPS=<workgroup> (tools/mlp_stamps.py). */
int hiptsdbg_mlp_stamps(unsigned long long* host, int n);
/* Host only, no GPU call: the weight layouts the two round-4 CCIP kernels read (tests/test_host_layouts.py builds them again in numpy).
 * hiptsdbg_mlp_weight_image: per 32 hidden units one block of IEEE-half bits [32 rows of w1, pitch C + 16 halves][C rows of w2, pitch 40 halves,
 * position 8 q + e of a row = hidden unit 16 (e >> 2) + 4 q + (e & 3) of the chunk]; out_halves = (4C / 32) * (32 * (C + 16) + C * 40).
 * hiptsdbg_dw_toeplitz: out u32 [channels][7][64] -- per (channel, kernel row) the 7 weights as halves Z[16 + kx] inside 48 zero halves;
 * lane L < 24 holds (Z[2L], Z[2L+1]), lane 32 + L holds (Z[2L+1], Z[2L+2]), the other lanes zero. */
int hiptsdbg_mlp_weight_image(const float* w1, const float* w2, int C, uint16_t* out, long long out_halves);
int hiptsdbg_dw_toeplitz(const float* w, int channels, uint32_t* out);
/* How the GEMM launcher would run a launch (csrc/gemm_plan.h: gemm_plan() is the one place the launch policy lives and the launcher
 * consumes exactly this).  Host only, no GPU call.  loop: the main loop; mr: rows of a tile / 32 (8 / 7 / 6); interior: the residual
 * instantiation without per-lane predication; stamped: the instantiation with in-kernel cycle stamps; tiles_m x tiles_n tiles on
 * `grid` workgroups of `block` threads with lds_bytes of dynamic LDS; tiles from sk_first on are cut into sk_slices K ranges
 * (1: no split); the raster_* / epi_* fields as the kernel receives them. */
enum { HIPTSDBG_GEMM_V1 = 0, HIPTSDBG_GEMM_PP = 1, HIPTSDBG_GEMM_S3 = 2, HIPTSDBG_GEMM_PP2 = 3, HIPTSDBG_GEMM_DW = 4,
       HIPTSDBG_GEMM_Q4 = 5, HIPTSDBG_GEMM_PP_E4M3 = 6 };
typedef struct hiptsdbg_gemm_plan_t {
    int32_t loop, mr, interior, stamped;
    int32_t tiles_m, tiles_n, grid, block, lds_bytes;
    int32_t sk_first, sk_slices;
    int32_t raster_gm, raster_gn, epi_prio, epi_prefetch;
    int32_t error;      /* 0, or why the launch is refused: 1 half operands outside the pp / dw loops, 2 e4m3 operands not built for the epilogue */
} hiptsdbg_gemm_plan_t;
/* The plan of the launch [M,K] x [N,K]^T with epilogue `epi` (GemmEpilogue) on a device of `cus` compute units, under this process's
 * HIPTS_GEMM* / HIPTS_EPI_* / HIPTS_RESID_GENERAL environment (read once) and the 4-wave mask q4_mask.  f16 / shared_chip / ld_out / dim
 * as GemmArgs; `features`: which optional arguments are present -- 1 stat_part, 2 sk_ws (the standard workspace size), 4 pos,
 * 8 res_scale, 16 the 16-bit copy (out_bf16 with ln_gamma), 32 stat_in (a folded input), 64 op8, 128 stamps.  A launch the launcher
 * refuses returns its error (and out->error). */
int hiptsdbg_gemm_plan(int epi, int M, int N, int K, int f16, int shared_chip, unsigned features, int ld_out, int dim, int cus,
                       unsigned q4_mask, hiptsdbg_gemm_plan_t* out);
/* The tile walk of the persistent GEMM loops (csrc/gemm_loop.h tile_origin, the function the kernels call).  Host only, no GPU call.
 * m0[id], n0[id]: first row and first column of the tile that work id `id` of [0, tiles_m * tiles_n) is handed, for tiles of tile_rows
 * (256 / 224 / 192) x 256 under the raster pair (raster_gm, raster_gn) of a plan. */
int hiptsdbg_gemm_tile_walk(int tiles_m, int tiles_n, int tile_rows, int raster_gm, int raster_gn, int32_t* m0, int32_t* n0);
/* What the loaded code object says of the ping-pong GEMM kernel the launcher picks for (epilogue, mr = tile rows / 32, operand type,
 * e4m3 operands, split-K, interior), from hipFuncGetAttributes: VGPRs per lane, bytes of scratch (private segment) per lane -- 0 means
 * nothing is spilled --, bytes of static LDS.  A combination no kernel is built for is refused. */
int hiptsdbg_gemm_kernel_resources(int epi, int mr, int f16, int op8, int sk, int interior, int* num_regs, int* scratch_bytes, int* static_lds);
/* ONE production launch -- launch_gemm(epi, g, null stream): the plan is gemm_plan()'s for this process and device, nothing is forced --
 * on caller-supplied operands, every output copied back whole (csrc/gemm_dbg.hip; tests/test_gpu_gemm_epi.py).
 * Inputs (host): a [M][K] and w [N][K] as 16-bit patterns (bf16, or IEEE half with f16 = 1; the entry pads w with zero rows to a multiple
 * of 256); the per-column float32 vectors bias / res_scale / ln_gamma / ln_beta / col_u of N elements (ln_gamma of EPI_SWIGLU: N / 2);
 * pos [tokens][N]; rowstat [M] pairs (rstd, rstd * mean) or stat_in [stat_in_blocks][stat_in_stride] pairs (sum, sum of squares);
 * rope [rope_tokens][32] pairs (sin, cos).  A null vector is absent from GemmArgs, except bias: null = zeros.  The scalar fields are
 * GemmArgs' of the same name (csrc/vit_internal.h); sk_ws != 0 hands the launch a zeroed split-K workspace as the forwards do.
 * Outputs: the caller sizes every buffer (hiptsdbg_gemm_out_t: host pointer and bytes; 0 bytes = the pointer stays null in GemmArgs) --
 * what the epilogue may write plus as many guard rows and pad elements as the test wants to watch.  The entry refuses a buffer smaller
 * than the launch's extent, fills each whole device buffer with the byte `fill`, copies x_init (x_init_bytes <= x_bytes; the fp32 stream's
 * initial contents, row-major or in the blocked layout as x_blocked says: [m / 16][n / 16][m % 16][n % 16], ld_out % 16 == 0, rows up to
 * a multiple of 16) over the start of x, launches once and copies every buffer back whole: a byte outside [M][N] that no longer holds
 * `fill` was written by the kernel.
 *   x: out_f32 (the fp32 stream; EPI_HEAD: logits)    rowmajor: resid_rowmajor_out    probs: out2_f32 (EPI_HEAD)
 *   out16[0..2]: out_bf16, out2_bf16, out3_bf16       stat_part: [column tile][stat_stride] pairs (EPI_SWIGLU, EPI_RESID_XG / XGI) */
typedef struct hiptsdbg_gemm_case_t {
    int32_t epi, M, N, K, f16, shared_chip;
    const uint16_t* a;
    const uint16_t* w;
    const float* bias;
    const float* pos;
    const float* res_scale;
    const float* ln_gamma;
    const float* ln_beta;
    const float* col_u;
    const float* rowstat;
    const float* stat_in;
    const float* rope;
    const float* x_init;
    uint64_t x_init_bytes;
    int32_t tokens, tokens_pad, heads, dim, hd_log2;
    int32_t stat_in_blocks, stat_in_stride, ln_dim, rope_tokens, stat_stride;
    int32_t gelu_tanh, star_kind, ld_out, x_blocked, sk_ws, fill;
    float qscale, ln_eps, star_scale, star_bias;
} hiptsdbg_gemm_case_t;
typedef struct hiptsdbg_gemm_out_t {
    void* x;
    void* rowmajor;
    void* probs;
    void* out16[3];
    void* stat_part;
    uint64_t x_bytes, rowmajor_bytes, probs_bytes, out16_bytes[3], stat_part_bytes;
} hiptsdbg_gemm_out_t;
int hiptsdbg_gemm_epilogue(const hiptsdbg_gemm_case_t* in, hiptsdbg_gemm_out_t* out);
/* The row kernels of csrc/row_ln.h and csrc/patch_rows.h, ONE launch each on caller-supplied operands (csrc/rows_dbg.hip;
 * tests/test_gpu_rows.py), modelled on hiptsdbg_gemm_epilogue: the caller sizes every output buffer, the entry refuses one smaller than
 * the launch's extent, fills each whole device buffer with the byte `fill`, launches once and copies every buffer back whole.  A buffer
 * the launch does not use may still be given: it comes back holding `fill`.
 *
 * hiptsdbg_row_ln: row_ln_kernel<f16, source, affine, sink>(rows, D, eps).  Only the tuples a forward launches are built; any other is
 * refused (HIPTS_ERR_INVALID), as are D % 4 != 0, D outside [4, 1024], a blocked layout with rows % 16 != 0 or D % 16 != 0, and
 * SINK_PATCH2X2 with an odd H or rows % (H * H) != 0.
 *   (SRC_F32, AFF_GAMMA_OPT_BETA, SINK_16)                vit.hip, launch_layernorm (b may be null)
 *   (SRC_F32_BLOCKED, AFF_GAMMA_ADD_ZERO, SINK_16)        ccip.hip
 *   (SRC_F32_INPLACE, AFF_GAMMA_PLAIN, SINK_BACK)         ccip.hip; blk = 0 / 1
 *   (SRC_F32, AFF_GAMMA_BETA, SINK_F32_AND_16)            convnext.hip, swinv2.hip: in place
 *   (SRC_F32, AFF_GAMMA_BETA, SINK_PATCH2X2)              convnext.hip
 *   (SRC_16_BIAS, AFF_GAMMA_BETA, SINK_16)                convnext.hip
 *   (SRC_F32, AFF_GAMMA_BETA, SINK_ADD_HILO)              swinv2.hip
 *   (SRC_F32, AFF_GAMMA_BETA, SINK_F32)                   swinv2.hip
 * in: the source rows [rows][D], float32 (the blocked layout [m / 16][n / 16][m % 16][n % 16] for SRC_F32_BLOCKED) or 16-bit patterns
 * (SRC_16_BIAS, with bias [D]); null for the in-place tuples (SRC_F32_INPLACE, SINK_F32_AND_16), whose rows are x_init.  g, b: [D].
 * out->f32: the float32 buffer the sink writes (SINK_F32: y; SINK_F32_AND_16, SINK_BACK, SINK_ADD_HILO: the stream x); x_init
 * (x_init_bytes <= f32_bytes) is copied over its start after the fill.  out->o16: the 16-bit buffer (SINK_16: [rows][D]; SINK_F32_AND_16:
 * the copy; SINK_PATCH2X2: [rows / 4][4 D]; SINK_ADD_HILO: [rows][hi(D) | lo(D)]). */
enum { HIPTSDBG_SRC_F32 = 0, HIPTSDBG_SRC_F32_BLOCKED = 1, HIPTSDBG_SRC_F32_INPLACE = 2, HIPTSDBG_SRC_16_BIAS = 3 };
enum { HIPTSDBG_AFF_GAMMA_BETA = 0, HIPTSDBG_AFF_GAMMA_OPT_BETA = 1, HIPTSDBG_AFF_GAMMA_ADD_ZERO = 2, HIPTSDBG_AFF_GAMMA_PLAIN = 3 };
enum { HIPTSDBG_SINK_16 = 0, HIPTSDBG_SINK_E4M3 = 1, HIPTSDBG_SINK_F32 = 2, HIPTSDBG_SINK_F32_AND_16 = 3, HIPTSDBG_SINK_PATCH2X2 = 4,
       HIPTSDBG_SINK_ADD_HILO = 5, HIPTSDBG_SINK_BACK = 6 };
typedef struct hiptsdbg_row_ln_case_t {
    int32_t src, affine, sink, f16, blk, H, D, fill;
    int64_t rows;
    float eps;
    const void* in;
    uint64_t in_bytes;
    const float* bias;
    const float* g;
    const float* b;
    const float* x_init;
    uint64_t x_init_bytes;
} hiptsdbg_row_ln_case_t;
typedef struct hiptsdbg_rows_out_t {
    void* f32;
    void* o16;
    uint64_t f32_bytes, o16_bytes;
} hiptsdbg_rows_out_t;
int hiptsdbg_row_ln(const hiptsdbg_row_ln_case_t* in, hiptsdbg_rows_out_t* out);
/* pool_ln_kernel once: out[b] = LN((sum over the T rows of x[b]) / count) for x float32 [batch][T][C] (blk != 0: each image's rows in the
 * blocked layout; T % 16 == 0 and C % 16 == 0 then), g, b [C]; 1 <= C <= 1024.  hilo == 0: the PooledF32 sink, out float32 [batch][C];
 * otherwise PooledHiLo, out 16-bit patterns [batch][hi(C) | lo(C)].  out_bytes >= 4 batch C either way. */
int hiptsdbg_pool_ln(const float* x, uint64_t x_bytes, const float* g, const float* b, int batch, int T, int C, int count, int blk, float eps,
                     int hilo, int f16, int fill, void* out, uint64_t out_bytes);
/* The two kernels of the folded LayerNorm that no GEMM launch contains (csrc/vit.hip; tests/test_gpu_ln_fold.py), ONE launch each through
 * launch_rowstat / launch_fold_ln, same conventions: the entry fills each whole device output buffer with `fill`, launches once and copies it
 * back whole; a buffer smaller than the launch's extent is refused.
 * hiptsdbg_rowstat: out[m] = (rstd, rstd * mean) of row m < M from part [blocks][stride] pairs (sum, sum of squares) over D columns in all;
 * stride >= M, blocks <= 64, part_bytes >= 8 blocks stride, out_bytes >= 8 M.
 * hiptsdbg_fold_ln: u[n] = sum_k W[n][k] gamma[k], c[n] = sum_k W[n][k] beta[k] + bias[n] from the 16-bit patterns w16 [N][K] (f16: IEEE half);
 * gamma, beta [K], bias [N]; beta and bias may be null (absent).  u and c have out_bytes each, out_bytes >= 4 N. */
int hiptsdbg_rowstat(const float* part, uint64_t part_bytes, int M, int stride, int blocks, int D, float eps, int fill, float* out, uint64_t out_bytes);
int hiptsdbg_fold_ln(const uint16_t* w16, int f16, const float* gamma, const float* beta, const float* bias, int N, int K, int fill, float* u, float* c,
                     uint64_t out_bytes);
/* patch_gather_kernel once with a (pixel, window) tuple a forward launches -- (PIX_U8_AFFINE, WIN_PATCH), (PIX_U8_TABLE, WIN_4X4),
 * (PIX_F32_FLIP, WIN_PATCH), (PIX_F32_FLIP, WIN_4X4), (PIX_F32, WIN_7X7) -- or, with PIX_U8_RAW and WIN_PATCH, patchify_u8_kernel.
 * images: uint8 [batch][S][S][3] or float32 [batch][3][S][S]; lut: float32 [3][256] (PIX_U8_TABLE).  WIN_PATCH: P x P patches, S % P == 0,
 * rows of 2 KH (KH >= 3 P P; PIX_U8_RAW: rows of 3 P P, KH unused); the others: S % 4 == 0, S / 4 tokens a side, rows of 128 / 320.
 * a0: 16-bit patterns, a0_bytes >= the rows of the launch. */
enum { HIPTSDBG_PIX_U8_AFFINE = 0, HIPTSDBG_PIX_U8_TABLE = 1, HIPTSDBG_PIX_F32_FLIP = 2, HIPTSDBG_PIX_F32 = 3, HIPTSDBG_PIX_U8_RAW = 4 };
enum { HIPTSDBG_WIN_PATCH = 0, HIPTSDBG_WIN_4X4 = 1, HIPTSDBG_WIN_7X7 = 2 };
int hiptsdbg_patch_gather(int pixel, int window, int f16, const void* images, uint64_t image_bytes, const float* lut, int batch, int S, int P,
                          int KH, int fill, uint16_t* a0, uint64_t a0_bytes);
/* The two LDS-tiled uint8 stems, file-local to their forwards, once each into a guarded a0 as above: stem_im2col_u8_kernel (csrc/ccip.hip;
 * images [batch][S][S][3], S % 4 == 0, lut [3][256]; rows of 320) and patchify_u8_p16_kernel (csrc/vit.hip; images of side 16 grid; rows
 * of 768). */
int hiptsdbg_ccip_stem_u8(const uint8_t* images, const float* lut, int batch, int S, int f16, int fill, uint16_t* a0, uint64_t a0_bytes);
int hiptsdbg_vit_patchify_u8_p16(const uint8_t* images, int batch, int grid, int f16, int fill, uint16_t* a0, uint64_t a0_bytes);
/* The small file-local kernels at the head and tail of the five forwards, ONE launch each beside the kernel, with the grid and block the
 * forward uses (each file's launch_* helper; tests/test_gpu_tokens.py against tests/tokens_ref.py).  Same conventions as above: the caller
 * gives every buffer's byte size, an input or output smaller than the launch's extent is refused (HIPTS_ERR_INVALID, nothing launched),
 * every output is filled whole with the byte `fill`, and copied back whole.  f16: IEEE half operands, otherwise bf16.
 *
 * hiptsdbg_vit_pool: pool_partial_kernel on a grid of (splits, batch), then pool_finalize_kernel (csrc/vit.hip).  x float32
 * [batch][tokens][D]; g, b float32 [D].  pool_then_norm == 0: the feature is g * mean_t((x_t - mean) * rstd) + b; otherwise
 * LN(mean_t x_t).  part_out: float32 [batch][splits][D], split s the sum over tokens [s * per, min(tokens, (s + 1) * per)),
 * per = ceil(tokens / splits), zeros for a split that owns none; part_bytes >= 4 batch splits D.  out16: 16-bit patterns
 * [batch][hi(D) | lo(D)]; out16_bytes >= 4 batch D.  Refused: D % 4 != 0, D > 1024, splits outside 1..32. */
int hiptsdbg_vit_pool(const float* x, uint64_t x_bytes, const float* g, const float* b, int batch, int tokens, int D, float eps, int pool_then_norm,
                      int splits, int f16, int fill, float* part_out, uint64_t part_bytes, uint16_t* out16, uint64_t out16_bytes);
/* eva_assemble_kernel (csrc/eva.hip).  tmp float32 [batch][np][D] (the patch rows); cls, pos float32 [D] (pos: row 0 of the position table).
 * x: float32 [batch][TS][D], row 0 of an image cls + pos, rows 1 .. np its patch rows, rows np + 1 .. TS - 1 zero; x_bytes >= 4 batch TS D.
 * blocked != 0: xblk holds the same rows a second time as 16 x 16 blocks [m / 16][n / 16][m % 16][n % 16] over m = b TS + r; rows of a
 * ragged last block that no image owns are not written; xblk_bytes >= 4 roundup(batch TS, 16) D.  blocked == 0: xblk (may be null)
 * comes back holding `fill`.  Refused: TS < np + 1, D % 4 != 0, blocked with D % 16 != 0. */
int hiptsdbg_eva_assemble(const float* tmp, uint64_t tmp_bytes, const float* cls, const float* pos, int batch, int np, int TS, int D, int blocked, int fill,
                          float* x, uint64_t x_bytes, float* xblk, uint64_t xblk_bytes);
/* eva_colsum_kernel (csrc/eva.hip).  x float32 [batch][TS][D]; part: float32 [batch][16][D], split s the sum of patch rows
 * [s * per, min(np, (s + 1) * per)), per = ceil(np / 16), patch row r at row 1 + r of its image (row 0 and rows past np are not read); zeros
 * for a split that owns none; part_bytes >= 64 batch D.  Refused: TS < np + 1, D % 4 != 0, D > 1024. */
int hiptsdbg_eva_colsum(const float* x, uint64_t x_bytes, int batch, int np, int TS, int D, int fill, float* part, uint64_t part_bytes);
/* The three small kernels of csrc/swinv2.hip.
 * hiptsdbg_swinv2_merge: sw_merge_kernel.  x float32 [batch][H][H][C]; col: 16-bit patterns [batch (H / 2)^2][hi(4 C) | lo(4 C)], the 4 C
 * columns of row (b, oy, ox) being x[b][2 oy + dy][2 ox + dx][:] for (dy, dx) = (0,0) (1,0) (0,1) (1,1) in that order; col_bytes >= 4 batch
 * H H C.  Refused: odd H, C % 4 != 0.
 * hiptsdbg_swinv2_split_x: sw_split_x_kernel.  x float32 [rows][D]; xh2: 16-bit patterns [rows][hi(D) | lo(D)]; xh2_bytes >= 4 rows D.
 * Refused: D % 4 != 0.
 * hiptsdbg_swinv2_mean: sw_mean_kernel with the PooledHiLo sink (the only one a forward launches).  y float32 [batch][T][C]; out: 16-bit
 * patterns [batch][hi(C) | lo(C)] of (sum of the T rows in order) / T; out_bytes >= 4 batch C. */
int hiptsdbg_swinv2_merge(const float* x, uint64_t x_bytes, int batch, int H, int C, int f16, int fill, uint16_t* col, uint64_t col_bytes);
int hiptsdbg_swinv2_split_x(const float* x, uint64_t x_bytes, int64_t rows, int D, int f16, int fill, uint16_t* xh2, uint64_t xh2_bytes);
int hiptsdbg_swinv2_mean(const float* y, uint64_t y_bytes, int batch, int T, int C, int f16, int fill, uint16_t* out, uint64_t out_bytes);
/* ds_im2col_kernel (csrc/ccip.hip): the 3 x 3 stride-2 pad-1 patch matrix.  xn: 16-bit patterns [batch][H][H][C] (moved, never
 * converted: no operand type); col: 16-bit patterns [batch (H / 2)^2][9][C], tap (ky, kx) of row (b, oy, ox) being
 * xn[b][2 oy - 1 + ky][2 ox - 1 + kx][:], zeros outside the image; col_bytes >= 18 batch (H / 2)^2 C.  Refused: odd H, C % 8 != 0. */
int hiptsdbg_ccip_ds_im2col(const uint16_t* xn, uint64_t xn_bytes, int batch, int H, int C, int fill, uint16_t* col, uint64_t col_bytes);
/* cnx_cast_kernel (csrc/convnext.hip).  x float32 [4 n4]; xh: 16-bit patterns [4 n4], each value rounded to nearest even; xh_bytes >= 8 n4. */
int hiptsdbg_convnext_cast(const float* x, uint64_t x_bytes, int64_t n4, int f16, int fill, uint16_t* xh, uint64_t xh_bytes);
/* out_host float32 [M][N] = A W^T for bf16 bit patterns a_bf16 [M][K], w_bf16 [N][K] (plain epilogue). */
int hiptsdbg_gemm_run(int M, int N, int K, const uint16_t* a_bf16, const uint16_t* w_bf16, float* out_host);
/* The e4m3 operand path: a_f32 / w_f32 are quantised by the library (per-tensor power-of-two weight scale returned in
 * w_exp); kind 0: float32 output, 1: e4m3 output through the StarReLU epilogue's store path. */
int hiptsdbg_gemm8_run(int M, int N, int K, const float* a_f32, const float* w_f32, int kind, void* out_host, int* w_exp);
/* Copies a named workspace tensor of the last forward ("x", "xn", "q", "k", "v", "att", "hmid") to the host. */
int hiptsdbg_vit_dump(hipts_vit_t* h, const char* name, void* out_host, size_t max_bytes, size_t* bytes);

/* The attention kernel alone: q, k 16-bit patterns [batch * heads][tokens_pad][head_dim] (q pre-scaled by head_dim^-0.5 * log2 e, rows past
 * `tokens` zero), vT [batch * heads][head_dim][tokens_pad]; out 16-bit patterns [batch][tokens][heads * head_dim].  f16: IEEE half operands. */
int hiptsdbg_attention_run(const uint16_t* q, const uint16_t* k, const uint16_t* vT, uint16_t* out_host, int batch, int heads, int tokens,
                           int tokens_pad, int head_dim, int f16);
/* The same launch timed: average device microseconds over `iters` launches (HIP events) with the chip to itself. */
int hiptsdbg_attention_time(const uint16_t* q, const uint16_t* k, const uint16_t* vT, int batch, int heads, int tokens, int tokens_pad,
                            int head_dim, int f16, int iters, double* avg_us);

/* The head_dim-64 attention kernel of round 3 (csrc/attn2.hip) alone: as above but v in its natural layout [batch * heads][tokens_pad][64].
 * iters == 0: one launch, result in out_host; iters > 0: average device microseconds of that many launches in *avg_us (out_host unused).
 * variant 0: the default geometry; 1: 4 waves x 64 query rows, 2: 8 waves x 32, 3: 4 waves x 32. */
int hiptsdbg_attention2(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out_host, int batch, int heads, int tokens, int tokens_pad,
                        int f16, int variant, int iters, double* avg_us);

/* ONE production launch of the same kernel through launch_attention2 with its whole argument list (tests/test_gpu_attention_exact.py),
 * modelled on hiptsdbg_gemm_epilogue.  q, k, v as above.  out_tokens_stride: rows an image owns in the output (0 = tokens; EVA02 passes its
 * padded token count); variant as above (6: the persistent one-wave-per-SIMD kernel of csrc/attn3.h); split_lo != 0: rows are
 * [hi | lo * lo_scale] (operand_f16 bit 4), lo_scale = split_lo_scale(f16) as the forwards pass it: 64 for IEEE half, 1 for bf16.
 * out_host: out_rows rows of out_ld = (split_lo ? 2 : 1) * heads * 64 16-bit values, out_rows >= batch * stride (stride = out_tokens_stride
 * or tokens) plus as many guard rows as the caller wants to watch.  Fill convention: the entry sets every byte of the device buffer to
 * 0xFF, launches once and copies the whole buffer back.  0xFFFF is a NaN in both 16-bit types and never a legitimate output: a real row
 * (image b, token t at row b * stride + t) that still holds it was not written; a gap row (t >= tokens) or guard row that no longer holds
 * it was written by the kernel. */
int hiptsdbg_attention2_launch(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out_host, long long out_rows, int batch, int heads,
                               int tokens, int tokens_pad, int f16, int out_tokens_stride, int variant, int split_lo);

/* What the loaded code object says of the kernel that hiptsdbg_attention2 (launch_attention2) runs for (tokens_pad, operand type, variant)
 * in this process, from hipFuncGetAttributes: VGPRs per lane, bytes of scratch (private segment) per lane -- 0 means nothing is spilled --,
 * bytes of static LDS.  Nothing is launched. */
int hiptsdbg_attention2_kernel_resources(int tokens_pad, int f16, int variant, int* num_regs, int* scratch_bytes, int* static_lds);

/* Measurement-only builds of csrc/attn2.hip (-DHIPTS_X_STAMPS=<workgroup>): the cycle stamps of one wave (tools/attn2_check.py stamps);
 * HIPTS_ERR_STATE in an ordinary build. */
int hiptsdbg_attention2_stamps(unsigned long long* host, int n);

/* One-query search path (hipts_search with nq == 1): how many candidates its threshold step collected for the last query and
 * whether the ranking used them (1) or fell through to the exact radix select (0). */
int hiptsdbg_search1_last(hipts_bm25_t* h, uint32_t* candidates, uint32_t* took_candidate_path);
/* How the query path would run a call (csrc/query_plan.h: search1_plan() and sim_plan() are the one place these decisions live and the
 * launchers of csrc/query.hip consume exactly these).  Host only, no GPU call.  knob_bits state the four switches the plans depend on
 * explicitly, whatever the process's environment says: the default is all four.
 *
 * hiptsdbg_search1_plan: hipts_search with one query over D documents, k results.  kk = min(k, D); waves of 64 documents; a group of
 * the threshold step is gl lanes of a wave (gw == 1) or gw whole waves; `groups` group maxima; bcap candidate slots per collect
 * workgroup; finish: search1_finish_kernel instead of the combine and collect kernels.  grid_score / blocks2 / blocks3: workgroups of
 * the score, combine and collect (or finish) kernels.  off_*: byte offsets into the workspace of ws_bytes -- group maxima (u64), candidate
 * counts and flags (u32 per collect workgroup), keys (u64 [blocks3][bcap]), ids (u32 [blocks3][bcap]), witness records (32 B, two per
 * score wave; present when finish).  out_bytes of results in pinned memory, the completion flag at off_flag. */
enum { HIPTSDBG_QUERY_FINISH = 1, HIPTSDBG_QUERY_WIDE = 2, HIPTSDBG_QUERY_TILED = 4, HIPTSDBG_QUERY_PARTS = 8, HIPTSDBG_QUERY_DEFAULT = 15 };
typedef struct hiptsdbg_search1_plan_t {
    int64_t waves;
    int32_t kk, gw, gl, groups, bcap, finish;
    int32_t grid_score, blocks2, blocks3, reserved;
    uint64_t off_wmax, off_bcnt, off_bflag, off_bkey, off_bid, off_wit, ws_bytes;
    uint64_t out_bytes, off_flag;
} hiptsdbg_search1_plan_t;
int hiptsdbg_search1_plan(int64_t D, int k, unsigned knob_bits, hiptsdbg_search1_plan_t* out);
/* hiptsdbg_sim_plan: the index product of nq queries of K floats against D rows (have_tiled: the tile-major copy exists).  wide_passes
 * launches of sim_mfma_wide_kernel, pass i over queries [256 i, ...): 256 queries in 8 query blocks on wide_grid workgroups, except the
 * last pass: last_n queries, last_nqb blocks, last_grid workgroups.  Then tail_passes launches of sim_mfma_kernel (tail_tiled: over
 * the tile-major copy) of up to 32 queries from query tail_q0 on, tail_grid workgroups each.  index_passes: all launches, each one pass
 * over the index.  parts_bytes (only with want_parts): the buffer the caller reserves for per-workgroup row maxima, one group per 256
 * queries; parts_grid > 0: every wide pass leaves the maxima of its parts_grid workgroups there; 0: the caller runs rowmax_kernel. */
typedef struct hiptsdbg_sim_plan_t {
    int32_t wide_passes, wide_grid, last_n, last_nqb, last_grid;
    int32_t tail_q0, tail_passes, tail_grid, tail_tiled;
    int32_t parts_grid, index_passes, reserved;
    uint64_t parts_bytes;
} hiptsdbg_sim_plan_t;
int hiptsdbg_sim_plan(int have_tiled, int64_t D, int K, int nq, int want_parts, unsigned knob_bits, hiptsdbg_sim_plan_t* out);
/* measurement-only builds (-DHIPTS_X_TOPK_STAMPS=<workgroup>): the 16 wall-clock stamps (10 ns units) of the last batched hipts_topk launch */
int hiptsdbg_topk_stamps(unsigned long long* host16);
/* The last hipts_bm25_related call on this handle: the HIP-event time of its count launches (all passes) and how many work items
 * (workgroups) took the LDS histogram arm and the direct global-atomics arm (tools/related_bench.py).  Any pointer may be NULL. */
int hiptsdbg_related_last(const hipts_bm25_t* h, double* count_ms, int64_t* lds_items, int64_t* direct_items);
/* The create call that built this handle (hipts_radius_create or hipts_radius_create_hamming): the HIP-event times of its pass 1
 * (the pair kernel counting degrees), of its pass 2 (the pair kernel filling the ids) and of the row sort (tools/dedup_bench.py).
 * Any pointer may be NULL. */
int hiptsdbg_radius_passes(const hipts_radius_t* h, double* pass1_ms, double* pass2_ms, double* sort_ms);

#ifdef __cplusplus
}
#endif
#endif /* HIP_TAGSEARCH_DEBUG_H */
