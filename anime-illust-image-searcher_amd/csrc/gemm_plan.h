// gemm_plan.h -- the GEMM launch policy as one pure function (host code only).  gemm_plan() decides which main loop, tile height and
// instantiation a launch takes, its grid and the launcher-set GemmArgs fields; gemm.hip's launch_t only carries the decision out, and
// models (ccip.hip), tests and tools ask it without a GPU (hiptsdbg_gemm_plan).
#pragma once
#include <algorithm>

#include "../../include/hip_tagsearch_debug.h"
#include "vit_internal.h"

namespace hipts {

// The environment switches of the launcher (A/B runs), read once per process by gemm_knobs()
struct GemmKnobs {
    // HIPTS_GEMM selects the main loop: "pp" (default) ping-pong with 16-MFMA segments; "pp2" 32-MFMA segments (better at K >= 4096,
    // slightly worse on the ViT's K = 768 shapes); "s3" three-stage 256x128 tile, two workgroups per CU; "v1" simple two-barrier loop;
    // "dw" the 256 x 128 x 32 two-workgroups-per-CU loop
    int variant = HIPTSDBG_GEMM_PP;
    bool variant_set = false;       // HIPTS_GEMM is in the environment, whatever it says
    bool auto_dw = true;            // HIPTS_GEMM_AUTO_DW
    int dw_limit4 = 2;              // HIPTS_GEMM_DW_LIMIT = n/4 of the CUs
    unsigned dw_mask = 0;           // HIPTS_GEMM_DW_MASK
    int min_mr = 6;                 // HIPTS_GEMM_BM = 256 / 224 / 192: the lowest tile the cost rule may pick
    int mr_shared = -1;             // HIPTS_GEMM_MR_SHARED
    bool persist = true;            // HIPTS_GEMM_PERSIST
    int raster = 8;                 // HIPTS_GEMM_RASTER; measured: 8 +0.4..0.8 % on the ViT forward, 4 / 16 +-0
    int raster_gn = 6;              // HIPTS_GEMM_RASTER_GN; measured (r03): fc1 fetches 251 -> 207 MB, q|k|v 194 -> 167 MB per launch, images/s +-0; 0 = off
    int epi_prio = 0;               // HIPTS_EPI_PRIO
    int epi_prefetch = 0;           // HIPTS_EPI_PREFETCH
    bool resid_general = false;     // HIPTS_RESID_GENERAL: the predicated residual epilogue on interior tiles too
    int splitk = 0, splitk_head = 0, splitk_minkt = 5;      // HIPTS_GEMM_SPLITK, _SPLITK_HEAD, _SPLITK_MINKT
};
const GemmKnobs& gemm_knobs();      // gemm.hip

using GemmPlan = hiptsdbg_gemm_plan_t;
int launch_gemm_q4(GemmEpilogue epi, const GemmArgs& a, const GemmPlan& p, int dev, hipStream_t s);      // gemm4.hip: a plan whose loop is HIPTSDBG_GEMM_Q4
constexpr int GEMM_PLAN_TILE = 256, GEMM_PLAN_HALF_BN = 128, GEMM_PLAN_BK = 64;       // gemm.hip asserts these against its kernels' constants
constexpr int GEMM_PLAN_LDS = 128 * 1024, GEMM_PLAN_LDS3 = 72 * 1024;

// "This many 256 x 256 tiles is small enough for the two-workgroups-per-CU dw loop."  A launch with fewer 256 x 256 tiles than CUs (the
// CAFormer's late stages: 11 520 tokens x 512 columns = 90 tiles) leaves most of the chip idle; the 256 x 128 two-per-CU kernel has 2 x
// the tiles and 2 x the slots (measured, CCIP B36 @384 batch 20: 9.3 -> 8.8 ms; no difference at batch 64).
// (round 3: only below 3/4 of the CUs -- EVA02-L's q|k|v at batch 10 is 252 tiles on 256 CUs and runs 1 % faster on the persistent kernel.
// Late round 4: only up to HALF the CUs, where every 256 x 128 tile gets a CU of its own; between a half and the whole chip the
// persistent kernel with 192-row tiles -- one round of 3/4 the length -- is faster: CCIP batch 64, whose stage-2 launches are 144
// tiles, 3244 -> 3412 images/s, batch 20 (90 tiles) stays on this kernel: 2586 against 2553.)
inline bool gemm_dw_size(long tiles256, int cus, const GemmKnobs& k) { return k.auto_dw && tiles256 * 4 <= (long)cus * k.dw_limit4; }

inline GemmPlan gemm_plan(GemmEpilogue epi, const GemmArgs& a, int cus, const GemmKnobs& k, unsigned q4_mask) {
    constexpr int T = GEMM_PLAN_TILE;
    GemmPlan p{};
    p.mr = 8; p.block = 512; p.lds_bytes = GEMM_PLAN_LDS; p.sk_slices = 1;
    p.tiles_m = (a.M + T - 1) / T;
    p.tiles_n = (a.N + T - 1) / T;
    // persistent grid: one workgroup per CU (a multiple of 8 so that a workgroup's tiles keep their XCD)
    const int slots = cus >= 8 ? cus / 8 * 8 : cus;
    if (a.op8) {
        // e4m3 operands: the persistent ping-pong loop with full tiles only
        if (epi != EPI_STAR && epi != EPI_RESID && epi != EPI_RESCALE && epi != EPI_RESID_LN && epi != EPI_QK && epi != EPI_VT && epi != EPI_BIAS) {
            p.error = 2;
            return p;
        }
        p.loop = HIPTSDBG_GEMM_PP_E4M3;
        p.grid = std::min(p.tiles_m * p.tiles_n, slots);
        return p;
    }
    const bool staged_only = epi == EPI_QK_ROPE || epi == EPI_SWIGLU || epi == EPI_RESID_XG || epi == EPI_RESID_XGI;
    const bool next_ln = epi == EPI_RESID_XG || epi == EPI_RESID_XGI;
    int variant = k.variant;
    if (staged_only) variant = HIPTSDBG_GEMM_PP;                // staged epilogue only (pp, or dw below)
    if (epi == EPI_RESID_LN) variant = HIPTSDBG_GEMM_PP;       // the row reduction across waves uses the persistent loop's LDS scratch stage
    // the dw loop has no statistics epilogue
    if (variant == HIPTSDBG_GEMM_PP && epi != EPI_HEAD && epi != EPI_RESID_LN && (!k.variant_set || staged_only) &&
        gemm_dw_size((long)p.tiles_m * p.tiles_n, cus, k) && a.M > T && !((next_ln || epi == EPI_SWIGLU) && a.stat_part))
        variant = HIPTSDBG_GEMM_DW;
    // A/B: HIPTS_GEMM_DW_MASK = bit mask over epilogue numbers whose launches take the two-workgroups-per-CU 256 x 128 kernel (its
    // residents run out of phase, so one's epilogue overlaps the other's main loop; it pays only where the epilogue is long and K short)
#ifdef HIPTS_X_DW_STAT      // timing probe only (the statistics come out wrong): lets the masked epilogues take the dw kernel even with stat_part
    const bool mask_stat_ok = true;
#else
    const bool mask_stat_ok = !(next_ln && a.stat_part);
#endif
    if (variant == HIPTSDBG_GEMM_PP && ((k.dw_mask >> (int)epi) & 1u) && a.M > T && mask_stat_ok) variant = HIPTSDBG_GEMM_DW;
    if (a.f16 && variant != HIPTSDBG_GEMM_PP && variant != HIPTSDBG_GEMM_DW) {
        p.error = 1;
        return p;
    }
    p.loop = variant;
    if (variant == HIPTSDBG_GEMM_DW || variant == HIPTSDBG_GEMM_S3) {
        p.tiles_n = (a.N + GEMM_PLAN_HALF_BN - 1) / GEMM_PLAN_HALF_BN;
        p.block = 256;
        p.lds_bytes = GEMM_PLAN_LDS3;
    }
    p.grid = p.tiles_m * p.tiles_n;
    if (variant == HIPTSDBG_GEMM_PP2) p.stamped = epi == EPI_GELU && a.stamps;
    if (variant != HIPTSDBG_GEMM_PP) return p;

    // 256-, 224- or 192-row tiles, whichever needs fewer (size-weighted) rounds over the CUs
    const int tiles_n = p.tiles_n;
    auto tiles_of = [&](int mr) { return (a.M + 32 * mr - 1) / (32 * mr); };
    auto cost_of = [&](int mr) { return ((long)tiles_of(mr) * tiles_n + cus - 1) / cus * (32 * mr); };
    // measured (r01): the switch pays when the predicted saving is large (N = 768: 2.625 vs 3 rounds,
    // -4..6 %) and costs 3 % when it is marginal (N = 3072: 9.6 vs 10) -- smaller tiles re-read W more.
    // ... and only when the launch has the chip to itself: with sub-batches on several streams the
    // partial last round is filled by the other stream's kernel and full tiles win (4.50 -> 4.59 k img/s).
    // 192 rows (round 3, half operands only): EVA02-L at the reference's batch of 10 -- 10 250 rows x 1024 columns are 164
    // tiles of 256 rows on 256 CUs (one round, 64 % of the chip) but 216 tiles of 192 rows (one round of 3/4 the length).
    // ... unless the whole launch is smaller than the chip (late round 4): then there is no last round for the other stream to fill,
    // and shorter tiles end the launch sooner (HIPTS_GEMM_MR_SHARED=0: as before, 1: by cost for every shared launch)
    int mr = 8;
    if (!a.shared_chip || k.mr_shared == 1 || (k.mr_shared != 0 && (long)tiles_of(8) * tiles_n < cus)) {
        long best = cost_of(8) * 93;
        for (int c = 7; c >= (a.f16 ? k.min_mr : std::max(k.min_mr, 7)); --c)
            if (cost_of(c) * 100 < best) {
                best = cost_of(c) * 100;
                mr = c;
            }
    }
    if (epi == EPI_HEAD && a.sk_ws && k.splitk_head >= 2) mr = 8;       // the split-K instantiation is built for 256-row tiles
    p.mr = mr;
    p.tiles_m = tiles_of(mr);
    const int ntile = p.tiles_m * tiles_n;
    p.grid = (k.persist && ntile > slots) ? slots : ntile;
    p.epi_prio = k.epi_prio;
    p.epi_prefetch = k.epi_prefetch;
    p.raster_gm = (k.raster > 0 && tiles_n >= 8) ? k.raster : 0;
    p.raster_gn = (k.raster_gn > 0 && tiles_n >= 8 && tiles_n > k.raster_gn) ? k.raster_gn : 0;
    // every tile inside the matrix: the RESID_XG instantiation without per-lane predication.
    // (Not instantiated for RESID_XGI: its only user, EVA02, has 1025 tokens per image -- no launch of whole tiles -- and with the
    // input fold's extra column vector the interior form compiled to 60 spilled registers.)
    const bool whole = epi == EPI_RESID_XG && mr == 8 && a.M % T == 0 && a.N % T == 0 && a.N <= 1024 && !a.pos && !a.res_scale && a.out_bf16 && a.stat_part;

    // the 4-wave, one-wave-per-SIMD loop (gemm4.hip) where it is built: q4_mask = bit mask over epilogue numbers (A/B).  Launches whose
    // tiles all lie inside the matrix with an even number of K-tiles; stamps where a stamped instantiation exists
    if (mr == 8 && ((q4_mask >> (int)epi) & 1u) && (epi == EPI_GELU || epi == EPI_QK || epi == EPI_RESID_XG) && a.sk_slices <= 1 &&
        !(a.stamps && !(a.f16 && (epi == EPI_GELU || epi == EPI_RESID_XG))) && a.M % T == 0 && a.N % T == 0 && a.K % 128 == 0 && a.K >= 128 &&
        !(epi == EPI_GELU && (a.ld_out ? a.ld_out : a.N) % 8) && !(epi == EPI_QK && a.dim % 64) &&
        (size_t)256 * a.K * 2 < ((size_t)1 << 31)) {       // per-lane source offsets are 32-bit: 256 rows of a tile
        p.loop = HIPTSDBG_GEMM_Q4;
        p.block = 256;
        p.grid = std::min(ntile, slots);
        p.interior = whole && !a.rowstat && !a.stat_in;
        p.stamped = a.stamps && a.f16 && (epi == EPI_GELU || p.interior);       // measurement build: in-kernel cycle stamps of workgroup 8 (tools/gemm_bench.py)
        return p;
    }
    // Split-K tail (GemmArgs::sk_*), an EXPERIMENT that lost (round 4) and stays off: the residual GEMMs with a long K whose last round
    // fills less than half of the chip -- EVA02-L's proj / fc2 at the reference's batch of 10 (84 tiles per sub-batch on 256 CUs), the
    // ViT's fc2 per 32-image sub-batch (294 tiles: 38 in the second round) -- with S <= HIPTS_GEMM_SPLITK slices of at least
    // HIPTS_GEMM_SPLITK_MINKT K-tiles.  Measured (tools/gpurun/r4_splitk.sh, one box): ViT-B/16 5093-5103 -> 4894-4898 images/s
    // (S = 4; S = 2: 4982), EVA02-L batch 10 1044 -> 829-832 images/s (S = 3), batch 32 unchanged.  A 256 x 256 fp32 slab is 256 KB:
    // 84 tiles x 3 slices write 64 MB through to memory and their last arrivers read it back, ~50 us per launch, more than the
    // under-filled main loop costs (cdna_hip_programming.md says as much: combine in-launch only when the slabs of a tile are tens of
    // KB).  It also gives up batch invariance -- a tile summed as S partial chains has other low bits than the same tile summed as one
    // chain, and WHICH tiles are split depends on the launch's size (tests/test_gpu_vit.py::test_folded_layernorm_path..., the sharded
    // CLIs' byte-equal output files) -- though run to run it is deterministic (slabs are added in slice order).  The tag head's launch
    // (EPI_HEAD: one row panel of 43 column tiles whatever the batch) would keep the invariance; HIPTS_GEMM_SPLITK_HEAD=4 enables it.
    if (epi == EPI_RESID || next_ln || epi == EPI_RESID_ROWSTAT || epi == EPI_HEAD) {
        const int sk_max = epi == EPI_HEAD ? (p.tiles_m == 1 ? k.splitk_head : 0) : k.splitk;
        const int rem = ntile % slots;      // tiles of the partial last round (the whole launch when it is smaller than the chip)
        if (a.sk_ws && mr == 8 && sk_max >= 2 && rem > 0 && rem * 2 <= slots && rem <= 1024) {
            int sl = std::min(sk_max, std::min(slots / rem, a.K / GEMM_PLAN_BK / (k.splitk_minkt > 0 ? k.splitk_minkt : 1)));
            while (sl >= 2 && 4096 + (size_t)rem * sl * ((size_t)T * T * 4) > a.sk_ws_bytes) --sl;
            if (sl >= 2) {
                p.sk_first = ntile - rem;
                p.sk_slices = sl;
                const int items = p.sk_first + rem * sl;
                p.grid = (k.persist && items > slots) ? slots : items;
                return p;
            }
        }
    }
    p.interior = whole && !k.resid_general;
    return p;
}

}  // namespace hipts
