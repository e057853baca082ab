// gemm_dbg.hip -- hiptsdbg_gemm_epilogue (include/hip_tagsearch_debug.h): one launch_gemm() on caller-supplied operands with every
// output buffer pre-filled, guarded and copied back whole.  Test aid, host code only: it decides nothing about the launch.
#include <vector>

#include "../../include/hip_tagsearch_debug.h"
#include "vit_internal.h"

namespace hipts {
namespace {

// a device copy of n floats of a host vector (null stays null)
int put_f32(DevBuf& buf, const float* host, size_t n, const float** dev) {
    *dev = nullptr;
    if (!host) return HIPTS_OK;
    HIPTS_TRY(buf.alloc(n * 4));
    HIPTS_TRY(upload(buf.p, host, n * 4));
    *dev = buf.as<float>();
    return HIPTS_OK;
}

// a device buffer of `bytes` filled with `fill`; refused when smaller than `need` (0 bytes: absent, allowed only when need == 0)
int guarded(DevBuf& buf, uint64_t bytes, uint64_t need, int fill, const char* what, bool required) {
    if (bytes == 0) {
        HIPTS_REQUIRE(!required, "hiptsdbg_gemm_epilogue: the %s buffer is required by this epilogue", what);
        return HIPTS_OK;
    }
    HIPTS_REQUIRE(bytes >= need, "hiptsdbg_gemm_epilogue: the %s buffer has %llu bytes, the launch's extent is %llu", what, (unsigned long long)bytes,
                  (unsigned long long)need);
    HIPTS_TRY(buf.alloc(bytes));
    HIPTS_HIP(hipMemset(buf.p, fill & 0xff, bytes));
    return HIPTS_OK;
}

int fetch(void* host, const DevBuf& buf, uint64_t bytes) {
    if (bytes == 0) return HIPTS_OK;
    HIPTS_REQUIRE(host, "hiptsdbg_gemm_epilogue: an output buffer has a size but no host pointer");
    HIPTS_HIP(hipMemcpy(host, buf.p, bytes, hipMemcpyDeviceToHost));
    return HIPTS_OK;
}

}  // namespace
}  // namespace hipts

extern "C" int hiptsdbg_gemm_epilogue(const hiptsdbg_gemm_case_t* in, hiptsdbg_gemm_out_t* out) {
    using namespace hipts;
    HIPTS_REQUIRE(in && out && in->a && in->w, "hiptsdbg_gemm_epilogue: null argument");
    const int epi = in->epi, M = in->M, N = in->N, K = in->K;
    HIPTS_REQUIRE(epi >= EPI_PATCH && epi <= EPI_RESID_LS && M >= 1 && N >= 1 && K >= 64 && K % 64 == 0 && (long long)M * K < (1ll << 31) &&
                      (long long)N * K < (1ll << 31),
                  "hiptsdbg_gemm_epilogue: unsupported shape");
    HIPTS_REQUIRE(epi == EPI_HEAD || N % 16 == 0, "hiptsdbg_gemm_epilogue: N must be a multiple of 16");
    HIPTS_TRY(use_device(0));

    // ---- the launch's extent in every output buffer
    const bool is_qk = epi == EPI_QK || epi == EPI_QK_ROPE;
    const uint64_t ld = in->ld_out ? in->ld_out : (epi == EPI_SWIGLU ? N / 2 : N);
    HIPTS_REQUIRE(ld >= (uint64_t)(epi == EPI_SWIGLU ? N / 2 : N) || is_qk || epi == EPI_VT, "hiptsdbg_gemm_epilogue: ld_out is smaller than a row");
    const bool blocked_ok = epi == EPI_RESID || epi == EPI_RESCALE || epi == EPI_RESID_ROWSTAT || epi == EPI_RESID_XG || epi == EPI_RESID_XGI ||
                            epi == EPI_BIAS || epi == EPI_RESID_LN;
    HIPTS_REQUIRE(!in->x_blocked || (blocked_ok && ld % 16 == 0), "hiptsdbg_gemm_epilogue: x_blocked needs a residual / bias epilogue and ld %% 16 == 0");
    const bool writes_x = blocked_ok || epi == EPI_PATCH || epi == EPI_RESID_LS;
    const uint64_t rows_x = in->x_blocked ? (uint64_t)round_up(M, 16) : (uint64_t)M;
    uint64_t need16[3] = {0, 0, 0};
    bool req16[3] = {false, false, false};
    if (is_qk || epi == EPI_VT) {
        HIPTS_REQUIRE(in->tokens >= 1 && in->tokens_pad >= in->tokens && in->dim >= 16 && (in->hd_log2 == 5 || in->hd_log2 == 6) &&
                          (in->heads << in->hd_log2) == in->dim && N <= (is_qk ? 3 : 1) * in->dim,
                      "hiptsdbg_gemm_epilogue: q / k / v layouts need tokens <= tokens_pad, heads * head_dim == dim and N within the layouts");
        const uint64_t images = (uint64_t)(M + in->tokens - 1) / in->tokens;
        const uint64_t layout = images * in->tokens_pad * in->dim * 2;
        need16[0] = layout; req16[0] = true;
        if (is_qk) { need16[1] = layout; req16[1] = true; }
        if (is_qk && N > 2 * in->dim) { need16[2] = layout; req16[2] = true; }
    } else if (epi == EPI_GELU || epi == EPI_STAR || epi == EPI_SWIGLU || epi == EPI_RESID_LN) {
        need16[0] = (uint64_t)M * ld * 2; req16[0] = true;
    } else if (epi == EPI_RESID_XG || epi == EPI_RESID_XGI || epi == EPI_RESID_LS) {
        need16[0] = (uint64_t)M * ld * 2;
    }
    if (epi == EPI_PATCH || in->pos) HIPTS_REQUIRE(in->pos && in->tokens >= 1, "hiptsdbg_gemm_epilogue: pos needs tokens");
    const bool has_stat = epi == EPI_SWIGLU || epi == EPI_RESID_XG || epi == EPI_RESID_XGI;
    HIPTS_REQUIRE(out->stat_part_bytes == 0 || (has_stat && in->stat_stride >= M), "hiptsdbg_gemm_epilogue: stat_part needs SWIGLU / RESID_XG / RESID_XGI and stat_stride >= M");
    HIPTS_REQUIRE(out->rowmajor_bytes == 0 || (in->x_blocked && (epi == EPI_RESID || epi == EPI_RESCALE || epi == EPI_RESID_ROWSTAT)),
                  "hiptsdbg_gemm_epilogue: resid_rowmajor_out needs x_blocked and a plain residual epilogue");
    HIPTS_REQUIRE(out->probs_bytes == 0 || epi == EPI_HEAD, "hiptsdbg_gemm_epilogue: probs is EPI_HEAD's");
    HIPTS_REQUIRE(in->x_init_bytes <= out->x_bytes && (in->x_init_bytes == 0 || in->x_init), "hiptsdbg_gemm_epilogue: x_init does not fit x");
    if (in->stat_in)
        HIPTS_REQUIRE(in->stat_in_blocks >= 1 && in->stat_in_blocks <= 64 && in->stat_in_stride >= M, "hiptsdbg_gemm_epilogue: stat_in needs its block count and stride");

    DevBuf x, rowmajor, probs, o16[3], stat;
    HIPTS_TRY(guarded(x, out->x_bytes, (writes_x || epi == EPI_HEAD) ? rows_x * ld * 4 : 0, in->fill, "x", writes_x));
    HIPTS_TRY(guarded(rowmajor, out->rowmajor_bytes, (uint64_t)M * ld * 4, in->fill, "rowmajor", false));
    HIPTS_TRY(guarded(probs, out->probs_bytes, (uint64_t)M * ld * 4, in->fill, "probs", false));
    for (int i = 0; i < 3; ++i) {
        HIPTS_REQUIRE(out->out16_bytes[i] == 0 || need16[i] > 0, "hiptsdbg_gemm_epilogue: this epilogue has no 16-bit output %d", i);
        HIPTS_TRY(guarded(o16[i], out->out16_bytes[i], need16[i], in->fill, "out16", req16[i]));
    }
    HIPTS_TRY(guarded(stat, out->stat_part_bytes, (uint64_t)((N + 255) / 256) * (uint64_t)in->stat_stride * 8, in->fill, "stat_part", false));
    if (in->x_init_bytes) HIPTS_TRY(upload(x.p, in->x_init, in->x_init_bytes));

    // ---- operands
    DevBuf A, W, bias, pos, rs, lg, lb, cu, rst, sti, rope, skws;
    const int Np = round_up(N, 256);
    HIPTS_TRY(A.alloc((size_t)M * K * 2));
    HIPTS_TRY(W.alloc((size_t)Np * K * 2));
    HIPTS_HIP(hipMemset(W.p, 0, W.bytes));
    HIPTS_TRY(upload(A.p, in->a, (size_t)M * K * 2));
    HIPTS_TRY(upload(W.p, in->w, (size_t)N * K * 2));
    GemmArgs g{};
    g.A = A.as<bf16_t>(); g.W = W.as<bf16_t>(); g.M = M; g.N = N; g.K = K; g.f16 = in->f16 ? 1 : 0; g.shared_chip = in->shared_chip ? 1 : 0;
    if (in->bias) {
        HIPTS_TRY(put_f32(bias, in->bias, (size_t)N, &g.bias));
    } else {
        HIPTS_TRY(bias.alloc((size_t)Np * 4));
        HIPTS_HIP(hipMemset(bias.p, 0, bias.bytes));
        g.bias = bias.as<float>();
    }
    HIPTS_TRY(put_f32(pos, in->pos, in->pos ? (size_t)in->tokens * N : 0, &g.pos));
    HIPTS_TRY(put_f32(rs, in->res_scale, (size_t)N, &g.res_scale));
    HIPTS_TRY(put_f32(lg, in->ln_gamma, (size_t)(epi == EPI_SWIGLU ? N / 2 : N), &g.ln_gamma));
    HIPTS_TRY(put_f32(lb, in->ln_beta, (size_t)N, &g.ln_beta));
    HIPTS_TRY(put_f32(cu, in->col_u, (size_t)N, &g.col_u));
    HIPTS_TRY(put_f32(rst, in->rowstat, (size_t)2 * M, &g.rowstat));
    HIPTS_TRY(put_f32(sti, in->stat_in, in->stat_in ? (size_t)2 * in->stat_in_blocks * in->stat_in_stride : 0, &g.stat_in));
    if (epi == EPI_QK_ROPE) {       // the kernel reads row 0 of the table for tokens it does not rotate
        HIPTS_REQUIRE(in->rope && in->rope_tokens >= 1, "hiptsdbg_gemm_epilogue: QK_ROPE needs the rotary table");
        HIPTS_TRY(put_f32(rope, in->rope, (size_t)in->rope_tokens * 64, &g.rope));
    }
    if (in->sk_ws) {
        HIPTS_TRY(skws.alloc(GEMM_SK_WS_BYTES));
        HIPTS_HIP(hipMemset(skws.p, 0, skws.bytes));
        g.sk_ws = skws.p; g.sk_ws_bytes = GEMM_SK_WS_BYTES;
    }
    g.out_f32 = out->x_bytes ? x.as<float>() : nullptr;
    g.resid_rowmajor_out = out->rowmajor_bytes ? rowmajor.as<float>() : nullptr;
    g.out2_f32 = out->probs_bytes ? probs.as<float>() : nullptr;
    g.out_bf16 = out->out16_bytes[0] ? o16[0].as<bf16_t>() : nullptr;
    g.out2_bf16 = out->out16_bytes[1] ? o16[1].as<bf16_t>() : nullptr;
    g.out3_bf16 = out->out16_bytes[2] ? o16[2].as<bf16_t>() : nullptr;
    g.stat_part = out->stat_part_bytes ? stat.as<float>() : nullptr;
    g.stat_stride = in->stat_stride;
    g.tokens = in->tokens; g.tokens_pad = in->tokens_pad; g.heads = in->heads; g.dim = in->dim; g.hd_log2 = in->hd_log2;
    g.stat_in_blocks = in->stat_in_blocks; g.stat_in_stride = in->stat_in_stride; g.ln_dim = in->ln_dim; g.rope_tokens = in->rope_tokens;
    g.gelu_tanh = in->gelu_tanh; g.star_kind = in->star_kind; g.ld_out = in->ld_out; g.x_blocked = in->x_blocked ? 1 : 0;
    g.qscale = in->qscale; g.ln_eps = in->ln_eps; g.star_scale = in->star_scale; g.star_bias = in->star_bias;

    HIPTS_TRY(launch_gemm((GemmEpilogue)epi, g, nullptr));
    HIPTS_HIP(hipDeviceSynchronize());

    HIPTS_TRY(fetch(out->x, x, out->x_bytes));
    HIPTS_TRY(fetch(out->rowmajor, rowmajor, out->rowmajor_bytes));
    HIPTS_TRY(fetch(out->probs, probs, out->probs_bytes));
    for (int i = 0; i < 3; ++i) HIPTS_TRY(fetch(out->out16[i], o16[i], out->out16_bytes[i]));
    HIPTS_TRY(fetch(out->stat_part, stat, out->stat_part_bytes));
    return HIPTS_OK;
}
