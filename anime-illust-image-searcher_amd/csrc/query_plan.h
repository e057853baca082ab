// query_plan.h -- the launch decisions of the query path as pure functions (host code only; no HIP call, no environment read), after
// gemm_plan.h: which kernels a call runs, their grids, its workspace layout.  query.hip's launchers carry a plan out, tests ask for it
// without a GPU (hiptsdbg_search1_plan, hiptsdbg_sim_plan).
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/hip_tagsearch_debug.h"

namespace hipts {
#pragma GCC visibility push(hidden)      // internal: nothing here joins the library's exported symbols
// The environment switches of the query path (A/B runs), read once per process by query_knobs()
struct QueryKnobs {
    bool sim_tiled = true;       // HIPTS_SIM=rows: the index product reads the row-major index, 32 queries a pass
    bool sim_wide = true;        // HIPTS_SIM_WIDE=0: the 32-query passes over the tile-major copy only
    bool sim_parts = true;       // HIPTS_SIM_PARTS=0: the batched search takes the products' row maxima with rowmax_kernel again
    bool bm25_scan = false;      // HIPTS_BM25=scan: the document-major scan
    int bm25_parts = 0;          // HIPTS_BM25_PARTS: workgroups per query of the sliced kernel (1 = the one-workgroup-per-query kernel; default: ~1024 on the chip)
    bool search1 = true;         // HIPTS_SEARCH1=0: one query takes the batched kernels
    bool s1_finish = true;       // HIPTS_SEARCH1_FINISH=0: combine and collect as two kernels
    bool s1_d2h = false;         // HIPTS_SEARCH1_D2H=1: results into a device buffer + copy
    bool s1_flag = true;         // HIPTS_SEARCH1_FLAG=0: completion by stream synchronise
    bool s1_pipe = true;         // HIPTS_S1_PIPE=0: the sequential form of the score kernel
    bool fused_topk = true;      // HIPTS_SEARCH_FUSED_TOPK=0: combine_kernel + top-k over the stored rows
    bool overlap = false;        // HIPTS_SEARCH_OVERLAP=1: BM25 on a side stream beside the index product
};
const QueryKnobs& query_knobs();      // query.hip

// The kernels' launch constants (query.hip and topk.h use these names; query.hip asserts the two structure sizes)
constexpr int SIM_THREADS = 512;     // 8 waves share one LDS query tile: 3 workgroups = 6 dependent MFMA chains per SIMD
constexpr int SIM_WIDE_QUERIES = 256, SIM_PARTS_MAX_GRID = 256;      // queries and, at most, workgroups of one sim_mfma_wide_kernel launch
constexpr int SIM_PARTS_GROUP_FLOATS = SIM_PARTS_MAX_GRID * SIM_WIDE_QUERIES;    // row maxima of one group of 256 queries: [workgroup][256]
constexpr int S1_MAX_DIM = 768, S1_MIN_DOCS = 8192, S1_THREADS = 128, S1_COLLECT_THREADS = 1024;
constexpr int S1_GROUPS = 4096;      // at most this many document groups (a group = 64 * gw consecutive documents, one wave of search1_combine_kernel)
constexpr int S1_BLOCK_CAP = 64;     // candidates one search1_collect_kernel workgroup (1024 documents) may hand on: at least this many (search1_plan sizes it)
constexpr size_t S1_STATE_BYTES = 3088, S1_WITNESS_BYTES = 32;       // sizeof(Search1State), sizeof(Search1Witness)

// The index product of nq queries (launch_sim): passes of up to 256 queries through sim_mfma_wide_kernel while more than 32 queries
// are left, the rest in passes of 32 through sim_mfma_kernel.  Every wide pass but the last takes 256 queries, so the plan holds the
// full pass and the last one instead of a list.  want_parts: the caller can use the wide kernel's per-workgroup row maxima.
using SimPlan = hiptsdbg_sim_plan_t;
struct SimPass { int q0, n, nqb, grid; };       // queries [q0, q0 + n), the kernel's query blocks, its grid
inline SimPass sim_wide_pass(const SimPlan& p, int i) {
    const bool last = i == p.wide_passes - 1;
    return SimPass{i * SIM_WIDE_QUERIES, last ? p.last_n : SIM_WIDE_QUERIES, last ? p.last_nqb : 8, last ? p.last_grid : p.wide_grid};
}
inline SimPlan sim_plan(bool have_tiled, int64_t D, int K, int nq, bool want_parts, const QueryKnobs& k) {
    SimPlan p{};
    const int64_t ntiles = (D + 31) / 32;
    p.tail_tiled = have_tiled && k.sim_tiled;
    if (p.tail_tiled && k.sim_wide && K % 4 == 0 && nq > 32) {
        // up to one workgroup per CU; a small index still fills them: the kernel splits the tiles it has across the query blocks
        auto grid_for = [&](int nqb) { return (int)std::max<int64_t>(1, std::min<int64_t>((ntiles * nqb + 7) / 8, SIM_PARTS_MAX_GRID)); };
        const int rest = nq % SIM_WIDE_QUERIES;         // more than 32: a wide pass of its own; otherwise the 32-query kernel's
        p.wide_passes = nq / SIM_WIDE_QUERIES + (rest > 32 ? 1 : 0);
        p.wide_grid = grid_for(8);
        p.last_n = rest > 32 ? rest : SIM_WIDE_QUERIES;
        p.last_nqb = p.last_n <= 64 ? 2 : p.last_n <= 128 ? 4 : 8;
        p.last_grid = grid_for(p.last_nqb);
        p.tail_q0 = rest > 32 ? nq : nq - rest;
    }
    p.tail_passes = (nq - p.tail_q0 + 31) / 32;
    p.tail_grid = (int)std::max<int64_t>(1, std::min<int64_t>((ntiles + SIM_THREADS / 64 - 1) / (SIM_THREADS / 64), 256 * 4));
    p.index_passes = p.wide_passes + p.tail_passes;
    // the row maxima come out of the accumulators when no query is left for the 32-query kernel and the groups share a grid
    if (want_parts && k.sim_parts) p.parts_bytes = (uint64_t)((nq + SIM_WIDE_QUERIES - 1) / SIM_WIDE_QUERIES) * SIM_PARTS_GROUP_FLOATS * sizeof(float);
    if (p.parts_bytes && p.wide_passes > 0 && p.tail_passes == 0 && (p.wide_passes == 1 || p.last_grid == p.wide_grid)) p.parts_grid = p.last_grid;
    return p;
}

// hipts_search for one query (search_one): geometry of its kernels, layout of its workspace and of the pinned results; and the
// conditions both one-query entries share (each adds its own: terms that fit the kernel arguments, a host query)
using Search1Plan = hiptsdbg_search1_plan_t;
inline bool search1_eligible(int nq, int dim, bool have_tiled, int64_t D, const QueryKnobs& k) {
    return nq == 1 && k.search1 && dim <= S1_MAX_DIM && dim % 4 == 0 && have_tiled && D >= S1_MIN_DOCS;
}
inline Search1Plan search1_plan(int64_t D, int k, const QueryKnobs& kn) {
    Search1Plan p{};
    p.waves = (D + 63) / 64;
    p.gw = (int)((p.waves + S1_GROUPS - 1) / S1_GROUPS);                   // 64 * gw documents per group
    p.grid_score = (int)((D + S1_THREADS - 1) / S1_THREADS);
    p.blocks2 = (int)((p.waves + (int64_t)p.gw * 4 - 1) / ((int64_t)p.gw * 4));
    p.blocks3 = (int)((D + S1_COLLECT_THREADS - 1) / S1_COLLECT_THREADS);
    p.kk = (int)std::min<int64_t>(k, D);
    // lanes per group: 64 unless that leaves fewer than 2.5 k groups (then the k-th largest group maximum bounds little: with fewer
    // groups than k every finite score is a candidate); down to 4.  G groups give about G * -ln(1 - k / G) candidates.
    p.gl = 64;
    while (p.gw == 1 && p.gl > 4 && D / p.gl < (int64_t)p.kk * 5 / 2) p.gl >>= 1;
    p.groups = p.blocks2 * 4 * (64 / p.gl);
    // candidate slots per collect workgroup (1024 documents): four times the expected share of ~1.7 k candidates, 64 .. 1024
    p.bcap = S1_BLOCK_CAP;
    while (p.bcap < 1024 && (int64_t)p.bcap * D < (int64_t)4 * 1024 * 17 * p.kk / 10) p.bcap <<= 1;
    // combine + collect in one launch (search1_finish_kernel) when a group is exactly one wave of the score kernel: its threshold comes
    // from the score kernel's witness records, two per wave
    p.finish = kn.s1_finish && p.gl == 64 && p.gw == 1;
    // workspace: state | group maxima u64[groups] | per-workgroup counts u32[blocks3] | flags u32[blocks3] | keys u64[blocks3][bcap] |
    // ids u32[blocks3][bcap] | witnesses [score workgroups][waves of one]
    p.off_wmax = (S1_STATE_BYTES + 15) / 16 * 16;
    p.off_bcnt = p.off_wmax + (uint64_t)p.groups * 8;
    p.off_bflag = p.off_bcnt + (uint64_t)p.blocks3 * 4;
    p.off_bkey = (p.off_bflag + (uint64_t)p.blocks3 * 4 + 15) / 16 * 16;
    p.off_bid = p.off_bkey + (uint64_t)p.blocks3 * p.bcap * 8;
    p.off_wit = (p.off_bid + (uint64_t)p.blocks3 * p.bcap * 4 + 31) / 32 * 32;
    p.ws_bytes = p.off_wit + (p.finish ? (uint64_t)p.grid_score * (S1_THREADS / 64) * S1_WITNESS_BYTES : 0);
    // pinned results: kk float64 scores, kk int32 ids, the completion flag on its own cache line behind them
    p.out_bytes = (uint64_t)p.kk * 12;
    p.off_flag = (p.out_bytes + 63) / 64 * 64;
    return p;
}

// BM25 rows of a batch (launch_bm25): term-major postings cut into document slices with `parts` workgroups per query, the same
// postings with one workgroup per query (an index too small to slice), or the document-major scan
struct Bm25Plan { enum Kernel { SLICED, POSTINGS, SCAN } kernel; int parts; };
inline Bm25Plan bm25_plan(int nq, int64_t slice_docs, const QueryKnobs& k) {
    if (k.bm25_scan) return Bm25Plan{Bm25Plan::SCAN, 0};
    if (slice_docs <= 0 || k.bm25_parts == 1) return Bm25Plan{Bm25Plan::POSTINGS, 0};
    const int parts = k.bm25_parts;
    return Bm25Plan{Bm25Plan::SLICED, (parts == 2 || parts == 4 || parts == 8) ? parts : nq >= 256 ? 4 : 8};
}

// The queries of a batch as one packed buffer: int32 terms[nt] | float64 weights[nt] | int32 ptr[nq + 1] | float32 vectors[nq][dim] (dim = 0: none)
struct QueryPack { size_t off_w, off_p, off_v, bytes; };
inline QueryPack query_pack(int nt, int nq, int dim) {
    const size_t off_w = ((size_t)nt * 4 + 15) / 16 * 16, off_p = off_w + (size_t)nt * 8, end_p = off_p + (size_t)(nq + 1) * 4;
    if (dim == 0) return QueryPack{off_w, off_p, end_p, end_p};
    const size_t off_v = (end_p + 15) / 16 * 16;
    return QueryPack{off_w, off_p, off_v, off_v + (size_t)nq * dim * 4};
}
#pragma GCC visibility pop
}  // namespace hipts
