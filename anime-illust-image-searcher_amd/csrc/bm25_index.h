// bm25_index.h -- struct hipts_bm25, the BM25 handle: the corpus statistics on host and device and the grow-only workspaces of the
// entry points that take it.  Internal (not part of the ABI): query.hip builds, scores and searches through it, related.hip counts
// co-occurrences over its two CSR images.
#pragma once
#include <vector>

#include "common.h"
#include "prof.h"
#include "../../include/hip_tagsearch_debug.h"

using hipts::DevBuf;
using hipts::PinBuf;

struct hipts_bm25 {
    int device = 0;
    int64_t D = 0, nnz = 0;
    int32_t V = 0;
    double avgdl = 0.0;
    std::vector<int64_t> h_ptr, h_dl, h_df;
    std::vector<int32_t> h_term, h_tf;
    std::vector<double> h_idf;
    DevBuf d_ptr, d_term, d_tf, d_dl, d_idf;   // int64[D+1], int32[nnz], int32[nnz], int32[D], double[V]
    DevBuf d_tptr, d_tdoc, d_ttf;              // term-major postings: int64[V+1], int32[nnz], int32[nnz]
    DevBuf d_tslice;                           // int64[V][BM25_SLICES + 1]: a term's postings cut at fixed document boundaries (bm25_postings_sliced_kernel)
    DevBuf ws_maxpart;                         // [queries][slices] partial row maxima of that kernel
    int64_t slice_docs = 0;                    // documents per slice (a multiple of 8); 0: the index is too small to be sliced
    DevBuf ws_q, ws_scores, ws_sims, ws_max, ws_final, ws_mark, ws_out, ws_parts;
    PinBuf pin_in, pin_out;                    // hipts_search: one H2D of the packed queries, one D2H of the packed results
    // hipts_search_submit / _collect (round 4): two batches in flight -- the host packs and launches batch i + 1 while the device runs batch i.
    // The device workspaces are shared (the batches run on one stream, in order); only the pinned buffers exist per slot.
    struct SearchSlot {
        PinBuf pin_in, pin_out;
        hipEvent_t done = nullptr;
        int nq = 0, k = 0, kk = 0;
        hipStream_t stream = nullptr;                   // the stream of the pending batch (both slots share the device workspaces: one stream)
        bool pending = false, host_result = false;      // host_result: the one-query path ran synchronously, its results wait in ids1 / vals1
        std::vector<int32_t> ids1;
        std::vector<double> vals1;
    } slot[2];
    DevBuf s1_state;                           // one-query path: Search1State + group maxima + per-workgroup candidate slots
    uint32_t s1_seq = 0;                       // sequence number of the last one-query call (completion flag in pinned memory)
    bool s1_dirty = true;                      // s1_state may hold leftovers (first use, or a call that failed half way)
    // batched hipts_search (round 4): BM25 postings on a side stream beside the index product -- the two do not depend on each other
    hipStream_t side = nullptr;
    hipEvent_t ev_in = nullptr, ev_bm25 = nullptr;
    // hipts_bm25_related (related.hip): one device pass of at most 256 queries -- their descriptors and work items, int32 [256][V] counts
    // followed by the matched counts, float64 [256][V] scores, the packed top-k rows; HIP events around the count launch of every pass
    DevBuf ws_rel_in, ws_rel_cnt, ws_rel_score, ws_rel_out;
    PinBuf pin_rel_in, pin_rel_out;            // the descriptors and items on their way in, the packed rows on their way out
    hipEvent_t rel_ev[2] = {nullptr, nullptr};
    double rel_count_ms = 0.0;                 // count launches of the last call
    int64_t rel_items[2] = {0, 0};             // work items of the last call: LDS histogram arm, direct arm
    // per-kernel HIP-event timing (hipts_query_profile_*): events on the stream each kernel is launched on
    bool prof = false;
    hipts::EventProfile<HIPTS_QUERY_PROF_CATEGORIES> ep;
};
