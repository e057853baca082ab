// rows_dbg.hip -- hiptsdbg_row_ln, hiptsdbg_pool_ln, hiptsdbg_patch_gather (include/hip_tagsearch_debug.h): one launch of a kernel of
// row_ln.h / patch_rows.h on caller-supplied operands with every output buffer pre-filled, guarded and copied back whole.  Test aid, host
// code only: it decides nothing about a launch.  hiptsdbg_rowstat and hiptsdbg_fold_ln do the same for the folded LayerNorm's two kernels
// of vit.hip, through that file's own launchers (vit_internal.h): those run vit.o's copy.
//
// row_ln.h and patch_rows.h keep everything in an anonymous namespace, so this object compiles its OWN copy of the templates, from the
// same source with the same flags as vit.o, eva.o, ccip.o, convnext.o and swinv2.o compile theirs.  These entries therefore test the
// source; the forwards' own tests (parity, batch invariance, u8 == f32 inputs) remain the check on each object's copy.
#include "../../include/hip_tagsearch_debug.h"
#include "dbg_buf.h"
#include "model_host.h"
#include "patch_rows.h"
#include "row_ln.h"

namespace hipts {
namespace {

// the (source, affine, sink) tuples the forwards launch, in the order of the header's list
enum RowLnTuple { RL_OPT_16, RL_BLOCKED_16, RL_INPLACE, RL_F32_AND_16, RL_PATCH2X2, RL_16BIAS_16, RL_ADD_HILO, RL_F32, RL_COUNT };
const int ROW_LN_TUPLES[RL_COUNT][3] = {
    {HIPTSDBG_SRC_F32, HIPTSDBG_AFF_GAMMA_OPT_BETA, HIPTSDBG_SINK_16},
    {HIPTSDBG_SRC_F32_BLOCKED, HIPTSDBG_AFF_GAMMA_ADD_ZERO, HIPTSDBG_SINK_16},
    {HIPTSDBG_SRC_F32_INPLACE, HIPTSDBG_AFF_GAMMA_PLAIN, HIPTSDBG_SINK_BACK},
    {HIPTSDBG_SRC_F32, HIPTSDBG_AFF_GAMMA_BETA, HIPTSDBG_SINK_F32_AND_16},
    {HIPTSDBG_SRC_F32, HIPTSDBG_AFF_GAMMA_BETA, HIPTSDBG_SINK_PATCH2X2},
    {HIPTSDBG_SRC_16_BIAS, HIPTSDBG_AFF_GAMMA_BETA, HIPTSDBG_SINK_16},
    {HIPTSDBG_SRC_F32, HIPTSDBG_AFF_GAMMA_BETA, HIPTSDBG_SINK_ADD_HILO},
    {HIPTSDBG_SRC_F32, HIPTSDBG_AFF_GAMMA_BETA, HIPTSDBG_SINK_F32},
};

}  // namespace
}  // namespace hipts

extern "C" int hiptsdbg_row_ln(const hiptsdbg_row_ln_case_t* in, hiptsdbg_rows_out_t* out) {
    using namespace hipts;
    const char* who = "hiptsdbg_row_ln";
    HIPTS_REQUIRE(in && out && in->g, "%s: null argument", who);
    const int64_t rows = in->rows;
    const int D = in->D;
    const bool f16 = in->f16 != 0;
    HIPTS_REQUIRE(rows >= 1 && rows <= (1 << 22), "%s: rows=%lld", who, (long long)rows);
    HIPTS_REQUIRE(D % 4 == 0 && D >= 4 && D <= 1024, "%s: D=%d must be a multiple of 4, at most 1024", who, D);
    int tuple = -1;
    for (int i = 0; i < RL_COUNT; ++i)
        if (ROW_LN_TUPLES[i][0] == in->src && ROW_LN_TUPLES[i][1] == in->affine && ROW_LN_TUPLES[i][2] == in->sink) tuple = i;
    HIPTS_REQUIRE(tuple >= 0, "%s: no forward launches (source %d, affine %d, sink %d)", who, in->src, in->affine, in->sink);
    const bool has_op = tuple != RL_INPLACE && tuple != RL_F32;          // the others read or write the 16-bit operand type
    HIPTS_REQUIRE(has_op || !f16, "%s: this tuple has no operand type (launched as <false>)", who);
    HIPTS_REQUIRE(in->blk == 0 || tuple == RL_INPLACE, "%s: blk is SRC_F32_INPLACE's", who);
    const bool blocked = tuple == RL_BLOCKED_16 || (tuple == RL_INPLACE && in->blk);
    HIPTS_REQUIRE(!blocked || (rows % 16 == 0 && D % 16 == 0), "%s: the blocked layout needs rows %% 16 == 0 and D %% 16 == 0", who);
    if (tuple == RL_PATCH2X2)
        HIPTS_REQUIRE(in->H >= 2 && in->H % 2 == 0 && in->H <= 1024 && rows % ((int64_t)in->H * in->H) == 0, "%s: SINK_PATCH2X2 needs an even H and rows == batch * H * H",
                      who);
    const bool with_b = in->affine == HIPTSDBG_AFF_GAMMA_BETA || in->affine == HIPTSDBG_AFF_GAMMA_OPT_BETA;
    HIPTS_REQUIRE(in->affine == HIPTSDBG_AFF_GAMMA_BETA ? in->b != nullptr : (with_b || !in->b), "%s: beta does not fit the affine", who);
    HIPTS_TRY(use_device(0));

    // ---- the launch's extent in every buffer
    const uint64_t n = (uint64_t)rows * D;
    const bool in_place = tuple == RL_INPLACE || tuple == RL_F32_AND_16;
    const uint64_t need_f32 = (in_place || tuple == RL_ADD_HILO || tuple == RL_F32) ? n * 4 : 0;
    const uint64_t need_16 = (tuple == RL_INPLACE || tuple == RL_F32) ? 0 : (tuple == RL_ADD_HILO ? 2 * n * 2 : n * 2);
    if (in_place) {
        HIPTS_REQUIRE(!in->in && in->x_init && in->x_init_bytes >= n * 4, "%s: an in-place tuple takes its rows from x_init", who);
    } else {
        HIPTS_REQUIRE(in->in && in->in_bytes >= n * (tuple == RL_16BIAS_16 ? 2 : 4), "%s: the source rows do not cover the launch", who);
        HIPTS_REQUIRE(tuple != RL_16BIAS_16 || in->bias, "%s: SRC_16_BIAS needs bias", who);
    }
    HIPTS_REQUIRE(in->x_init_bytes <= out->f32_bytes && (in->x_init_bytes == 0 || in->x_init), "%s: x_init does not fit the float32 buffer", who);
    DevBuf f32, o16, src, bias, gv, bv;
    HIPTS_TRY(dbg_guarded(f32, out->f32_bytes, need_f32, in->fill, who, "float32"));
    HIPTS_TRY(dbg_guarded(o16, out->o16_bytes, need_16, in->fill, who, "16-bit"));
    if (in->x_init_bytes) HIPTS_TRY(upload(f32.p, in->x_init, in->x_init_bytes));
    if (!in_place) HIPTS_TRY(dbg_put(src, in->in, in->in_bytes));
    if (in->bias) HIPTS_TRY(dbg_put(bias, in->bias, (size_t)D * 4));
    HIPTS_TRY(dbg_put(gv, in->g, (size_t)D * 4));
    if (in->b) HIPTS_TRY(dbg_put(bv, in->b, (size_t)D * 4));

    float* x = f32.as<float>();
    bf16_t* h = o16.as<bf16_t>();
    const float* s32 = src.as<float>();
    const float* g = gv.as<float>();
    const float* b = in->b ? bv.as<float>() : nullptr;
    const int blocks = (int)((rows + 3) / 4);
    const float eps = in->eps;
    const LnGammaBeta gb{g, b};
    switch (tuple) {
    case RL_OPT_16:
        HIPTS_LAUNCH_F16(f16, row_ln_kernel, blocks, 256, 0, nullptr, FromF32{s32}, LnGammaOptBeta{g, b}, To16{h}, rows, D, eps);
        break;
    case RL_BLOCKED_16:
        HIPTS_LAUNCH_F16(f16, row_ln_kernel, blocks, 256, 0, nullptr, FromF32Blocked{s32}, LnGamma<true>{g}, To16{h}, rows, D, eps);
        break;
    case RL_INPLACE:
        row_ln_kernel<false><<<blocks, 256, 0, nullptr>>>(F32InPlace{x, in->blk ? 1 : 0}, LnGamma<false>{g}, BackToSource{}, rows, D, eps);
        HIPTS_LAUNCH_CHECK();
        break;
    case RL_F32_AND_16:
        HIPTS_LAUNCH_F16(f16, row_ln_kernel, blocks, 256, 0, nullptr, FromF32{x}, gb, ToF32And16{x, h}, rows, D, eps);
        break;
    case RL_PATCH2X2:
        HIPTS_LAUNCH_F16(f16, row_ln_kernel, blocks, 256, 0, nullptr, FromF32{s32}, gb, ToPatch2x2{h, in->H}, rows, D, eps);
        break;
    case RL_16BIAS_16:
        HIPTS_LAUNCH_F16(f16, row_ln_kernel, blocks, 256, 0, nullptr, From16Bias{src.as<bf16_t>(), bias.as<float>()}, gb, To16{h}, rows, D, eps);
        break;
    case RL_ADD_HILO:
        HIPTS_LAUNCH_F16(f16, row_ln_kernel, blocks, 256, 0, nullptr, FromF32{s32}, gb, AddToStreamHiLo{x, h, h + D}, rows, D, eps);
        break;
    default:
        row_ln_kernel<false><<<blocks, 256, 0, nullptr>>>(FromF32{s32}, gb, ToF32{x}, rows, D, eps);
        HIPTS_LAUNCH_CHECK();
        break;
    }
    HIPTS_HIP(hipDeviceSynchronize());
    HIPTS_TRY(dbg_fetch(out->f32, f32, out->f32_bytes, who));
    HIPTS_TRY(dbg_fetch(out->o16, o16, out->o16_bytes, who));
    return HIPTS_OK;
}

extern "C" int hiptsdbg_pool_ln(const float* x, uint64_t x_bytes, const float* g, const float* b, int batch, int T, int C, int count, int blk,
                                float eps, int hilo, int f16, int fill, void* out, uint64_t out_bytes) {
    using namespace hipts;
    const char* who = "hiptsdbg_pool_ln";
    HIPTS_REQUIRE(x && g && b && out, "%s: null argument", who);
    HIPTS_REQUIRE(batch >= 1 && batch <= 4096 && T >= 1 && T <= (1 << 16) && C >= 1 && C <= 1024 && count >= 1, "%s: unsupported shape", who);
    HIPTS_REQUIRE(!blk || (T % 16 == 0 && C % 16 == 0), "%s: the blocked layout needs T %% 16 == 0 and C %% 16 == 0", who);
    HIPTS_REQUIRE(hilo || !f16, "%s: the float32 sink has no operand type (launched as <false>)", who);
    HIPTS_REQUIRE(x_bytes >= (uint64_t)batch * T * C * 4, "%s: x does not cover the launch", who);
    HIPTS_TRY(use_device(0));
    DevBuf xd, gd, bd, od;
    HIPTS_TRY(dbg_guarded(od, out_bytes, (uint64_t)batch * C * 4, fill, who, "output"));
    HIPTS_TRY(dbg_put(xd, x, x_bytes));
    HIPTS_TRY(dbg_put(gd, g, (size_t)C * 4));
    HIPTS_TRY(dbg_put(bd, b, (size_t)C * 4));
    if (hilo) {
        HIPTS_LAUNCH_F16(f16 != 0, pool_ln_kernel, batch, 1024, 0, nullptr, xd.as<float>(), gd.as<float>(), bd.as<float>(), PooledHiLo{od.as<bf16_t>()}, T, C,
                         eps, blk ? 1 : 0, count);
    } else {
        pool_ln_kernel<false><<<batch, 1024, 0, nullptr>>>(xd.as<float>(), gd.as<float>(), bd.as<float>(), PooledF32{od.as<float>()}, T, C, eps, blk ? 1 : 0,
                                                           count);
        HIPTS_LAUNCH_CHECK();
    }
    HIPTS_HIP(hipDeviceSynchronize());
    return dbg_fetch(out, od, out_bytes, who);
}

extern "C" int hiptsdbg_rowstat(const float* part, uint64_t part_bytes, int M, int stride, int blocks, int D, float eps, int fill, float* out,
                               uint64_t out_bytes) {
    using namespace hipts;
    const char* who = "hiptsdbg_rowstat";
    HIPTS_REQUIRE(part && out, "%s: null argument", who);
    HIPTS_REQUIRE(M >= 1 && M <= (1 << 22) && stride >= M && blocks >= 1 && blocks <= 64 && D >= 1, "%s: unsupported shape", who);
    HIPTS_REQUIRE(part_bytes >= (uint64_t)blocks * stride * 8, "%s: the partial pairs do not cover [blocks][stride]", who);
    HIPTS_TRY(use_device(0));
    DevBuf pd, od;
    HIPTS_TRY(dbg_guarded(od, out_bytes, (uint64_t)M * 8, fill, who, "output"));
    HIPTS_TRY(dbg_put(pd, part, part_bytes));
    HIPTS_TRY(launch_rowstat(pd.as<float>(), od.as<float>(), M, stride, blocks, D, eps, nullptr));
    HIPTS_HIP(hipDeviceSynchronize());
    return dbg_fetch(out, od, out_bytes, who);
}

extern "C" int hiptsdbg_fold_ln(const uint16_t* w16, int f16, const float* gamma, const float* beta, const float* bias, int N, int K, int fill, float* u,
                                float* c, uint64_t out_bytes) {
    using namespace hipts;
    const char* who = "hiptsdbg_fold_ln";
    HIPTS_REQUIRE(w16 && gamma && u && c, "%s: null argument", who);
    HIPTS_REQUIRE(N >= 1 && N <= (1 << 16) && K >= 1 && K <= (1 << 16), "%s: unsupported shape", who);
    HIPTS_TRY(use_device(0));
    DevBuf wd, gd, bd, bi, ud, cd;
    HIPTS_TRY(dbg_guarded(ud, out_bytes, (uint64_t)N * 4, fill, who, "u"));
    HIPTS_TRY(dbg_guarded(cd, out_bytes, (uint64_t)N * 4, fill, who, "c"));
    HIPTS_TRY(dbg_put(wd, w16, (size_t)N * K * 2));
    HIPTS_TRY(dbg_put(gd, gamma, (size_t)K * 4));
    if (beta) HIPTS_TRY(dbg_put(bd, beta, (size_t)K * 4));
    if (bias) HIPTS_TRY(dbg_put(bi, bias, (size_t)N * 4));
    HIPTS_TRY(launch_fold_ln(wd.as<bf16_t>(), f16 != 0, gd.as<float>(), beta ? bd.as<float>() : nullptr, bias ? bi.as<float>() : nullptr, ud.as<float>(),
                             cd.as<float>(), N, K, nullptr));
    HIPTS_HIP(hipDeviceSynchronize());
    HIPTS_TRY(dbg_fetch(u, ud, out_bytes, who));
    return dbg_fetch(c, cd, out_bytes, who);
}

extern "C" int hiptsdbg_patch_gather(int pixel, int window, int f16, const void* images, uint64_t image_bytes, const float* lut, int batch, int S,
                                     int P, int KH, int fill, uint16_t* a0, uint64_t a0_bytes) {
    using namespace hipts;
    const char* who = "hiptsdbg_patch_gather";
    HIPTS_REQUIRE(images && a0, "%s: null argument", who);
    HIPTS_REQUIRE(batch >= 1 && batch <= 64 && S >= 4 && S <= 1024, "%s: unsupported shape", who);
    const bool raw = pixel == HIPTSDBG_PIX_U8_RAW;
    const bool listed = (pixel == HIPTSDBG_PIX_U8_AFFINE && window == HIPTSDBG_WIN_PATCH) || (pixel == HIPTSDBG_PIX_U8_TABLE && window == HIPTSDBG_WIN_4X4) ||
                        (pixel == HIPTSDBG_PIX_F32_FLIP && (window == HIPTSDBG_WIN_PATCH || window == HIPTSDBG_WIN_4X4)) ||
                        (pixel == HIPTSDBG_PIX_F32 && window == HIPTSDBG_WIN_7X7) || (raw && window == HIPTSDBG_WIN_PATCH);
    HIPTS_REQUIRE(listed, "%s: no forward launches (pixel %d, window %d)", who, pixel, window);
    int G, ks, half;
    if (window == HIPTSDBG_WIN_PATCH) {
        HIPTS_REQUIRE(P >= 1 && P <= 64 && S % P == 0 && (raw || KH >= 3 * P * P), "%s: WIN_PATCH needs S %% P == 0 and KH >= 3 P P", who);
        G = S / P; ks = P; half = KH;
    } else {
        HIPTS_REQUIRE(S % 4 == 0, "%s: the 4 x 4 and 7 x 7 windows need S %% 4 == 0", who);
        G = S / 4; ks = window == HIPTSDBG_WIN_4X4 ? 4 : 7; half = window == HIPTSDBG_WIN_4X4 ? 64 : 160;
    }
    const bool u8 = pixel == HIPTSDBG_PIX_U8_AFFINE || pixel == HIPTSDBG_PIX_U8_TABLE || raw;
    HIPTS_REQUIRE(image_bytes >= (uint64_t)batch * S * S * 3 * (u8 ? 1 : 4), "%s: the images do not cover the launch", who);
    HIPTS_REQUIRE(pixel != HIPTSDBG_PIX_U8_TABLE || lut, "%s: PIX_U8_TABLE needs lut", who);
    HIPTS_TRY(use_device(0));
    const int64_t tokens = (int64_t)batch * G * G, total = tokens * ks;
    DevBuf img, lutd, ad;
    HIPTS_TRY(dbg_guarded(ad, a0_bytes, (uint64_t)tokens * (raw ? 3 * P * P : 2 * half) * 2, fill, who, "a0"));
    HIPTS_TRY(dbg_put(img, images, image_bytes));
    if (lut) HIPTS_TRY(dbg_put(lutd, lut, 3 * 256 * 4));
    const int blocks = (int)ceil_div(total, 256);
    bf16_t* a = ad.as<bf16_t>();
    const bool h = f16 != 0;
    if (raw) {
        HIPTS_LAUNCH_F16(h, patchify_u8_kernel, blocks, 256, 0, nullptr, img.as<uint8_t>(), a, batch, S, P, G);
    } else if (pixel == HIPTSDBG_PIX_U8_AFFINE) {
        HIPTS_LAUNCH_F16(h, patch_gather_kernel, blocks, 256, 0, nullptr, PixelU8Affine{img.as<uint8_t>()}, WindowPatch{P, KH}, a, total, S, G);
    } else if (pixel == HIPTSDBG_PIX_U8_TABLE) {
        HIPTS_LAUNCH_F16(h, patch_gather_kernel, blocks, 256, 0, nullptr, PixelU8Table{img.as<uint8_t>(), lutd.as<float>()}, Window4x4{}, a, total, S, G);
    } else if (pixel == HIPTSDBG_PIX_F32_FLIP && window == HIPTSDBG_WIN_PATCH) {
        HIPTS_LAUNCH_F16(h, patch_gather_kernel, blocks, 256, 0, nullptr, PixelF32Planes<true>{img.as<float>()}, WindowPatch{P, KH}, a, total, S, G);
    } else if (pixel == HIPTSDBG_PIX_F32_FLIP) {
        HIPTS_LAUNCH_F16(h, patch_gather_kernel, blocks, 256, 0, nullptr, PixelF32Planes<true>{img.as<float>()}, Window4x4{}, a, total, S, G);
    } else {
        HIPTS_LAUNCH_F16(h, patch_gather_kernel, blocks, 256, 0, nullptr, PixelF32Planes<false>{img.as<float>()}, Window7x7{}, a, total, S, G);
    }
    HIPTS_HIP(hipDeviceSynchronize());
    return dbg_fetch(a0, ad, a0_bytes, who);
}
