// related.hip -- related tags: co-occurrence counts over the BM25 index and their ranking (hipts_bm25_related).
//
// The reference has no such step: its README tells the user to grep the tag file when a query word is unknown.  The definition
// (restated from include/hip_tagsearch.h; tests/related_ref.py is the numpy statement of it):
//   T(d)   the distinct term ids of document d (csr_term of hipts_bm25_export; tf is ignored)
//   M      { d : include is a subset of T(d) and exclude does not meet T(d) };  n = |M|;  both lists empty: every document
//   c[u]   |{ d in M : u in T(d) }|
//   score  COUNT (double)c;  JACCARD (double)c / (double)(n + df[u] - c);  LIFT ((double)c / (double)n) / ((double)df[u] / (double)D)
//   a term is a candidate iff c[u] >= max(min_count, 1) and u is in neither list; candidates rank by (score descending, id ascending)
// Counts are integer adds (the result does not depend on arrival order); the scores are float64 expressions of integers that are
// exact in a double, one rounding per operation (-ffp-contract=off), so the whole result is bit-reproducible.
//
// One device pass takes up to REL_PASS queries:
//   related_count_kernel   one workgroup per (query, chunk of REL_CHUNK entries of the query's driving list) -- the shortest include
//                          posting list, or the document range when nothing is included.  Phase A, a thread per entry: the document's
//                          CSR row bounds, and the row tested against the remaining include and the exclude terms; matching rows go
//                          on a list in LDS.  Phase B, sixteen lanes per row (a row's terms are distinct: at most four lanes of a wave
//                          instruction can meet on one bin): every term of every listed row adds 1 to a histogram of the vocabulary --
//                          in LDS, flushed bin by bin (non-zero bins only) with integer global atomics into the query's count row
//                          (the LDS arm), or straight in the count row (the direct arm: a vocabulary above REL_LDS_MAX_V; for short
//                          driving lists it was measured and is not used, see REL_DIRECT_MAX).
//   related_score_kernel   thread per (query, term): -inf for non-candidates (never scored: nothing divides by zero)
//   topk_kernel            through hipts_topk on the device rows: the ranking rule of topk.h, not a second one
//   related_finish_kernel  ids of -inf results become -1, the results' counts are gathered, the matched counts join them: one copy back
// Algorithmic traffic of the count pass: 4 B per driving entry + 16 B of row bounds per tested document + 4 B per term of every
// tested row (test) and of every matching row (add); atomics: one LDS (or global) add per term of a matching row, and per
// workgroup of the LDS arm V LDS clears, V LDS reads and one global add per non-zero bin.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "bm25_index.h"
#include "common.h"

using namespace hipts;

namespace {

constexpr int REL_MAX_TERMS = 32;        // terms in either list of a query
constexpr int REL_MAX_K = 1024;          // hipts_topk's limit
constexpr int REL_PASS = 256;            // queries per device pass (the workspace is REL_PASS x V counts and scores)
constexpr int REL_THREADS = 256;
constexpr int REL_CHUNK = 1024;          // driving-list entries per workgroup: 4 per thread, all their loads in flight at once
constexpr int REL_GROUP = 16;            // lanes that walk one row in phase B
// The LDS arm's vocabulary limit: 128 KiB of bins + 12.3 KiB of row list and query terms of the CU's 160 KiB (one workgroup per CU at
// the limit; the wd-tagger vocabulary, 10 861 terms = 43 KB, leaves room for three).
constexpr int REL_LDS_MAX_V = 32768;
// Driving lists up to this long take the direct arm although the vocabulary fits LDS.  0: none does -- measured at limits 0, 256 and
// 4096 (HIPTS_RELATED_DIRECT_MAX sets it for a measurement; tools/related_bench.py, profiles/related_tags.txt), the direct arm was
// never faster: one query on a list of 100 entries 10 us either way, the count launches of the all-terms table 0.61 ms with every
// list through LDS against 0.79 ms (limit 256) and 1.22 ms (limit 4096).
constexpr int64_t REL_DIRECT_MAX = 0;

struct RelQuery {
    int32_t inc[REL_MAX_TERMS], exc[REL_MAX_TERMS];
    int32_t ninc, nexc;
    int32_t drive;                       // position in inc of the term whose posting list drives the walk; -1: the document range
    int32_t pad;
    int64_t len;                         // entries of the driving list (df of the driving term, or D)
};
struct RelItem {
    int32_t q, lds;                      // query of the pass; 1: LDS histogram arm, 0: direct arm
    int64_t start;                       // first driving-list entry of this workgroup
};

// Phase B for rows [0, nr) of the workgroup's list: dst[t] += 1 for every term t of every row.
__device__ __forceinline__ void rel_add_rows(int32_t* __restrict__ dst, const int32_t* __restrict__ term, const int64_t* row_b,
                                             const int32_t* row_n, int nr) {
    const int sub = threadIdx.x % REL_GROUP, grp = threadIdx.x / REL_GROUP;
    constexpr int GROUPS = REL_THREADS / REL_GROUP, RU = 4;      // four rows per group in flight
    for (int r0 = grp; r0 < nr; r0 += GROUPS * RU) {
        int64_t b[RU];
        int32_t n[RU], t[RU];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const int r = r0 + u * GROUPS;
            n[u] = r < nr ? row_n[r] : 0;
            b[u] = r < nr ? row_b[r] : 0;
        }
#pragma unroll
        for (int u = 0; u < RU; ++u) t[u] = sub < n[u] ? term[b[u] + sub] : -1;
#pragma unroll
        for (int u = 0; u < RU; ++u)
            if (t[u] >= 0) atomicAdd(&dst[t[u]], 1);
#pragma unroll
        for (int u = 0; u < RU; ++u)                             // rows longer than the group
            for (int i = sub + REL_GROUP; i < n[u]; i += REL_GROUP) atomicAdd(&dst[term[b[u] + i]], 1);
    }
}

__global__ __launch_bounds__(REL_THREADS) void related_count_kernel(const RelQuery* __restrict__ queries, const RelItem* __restrict__ items,
                                                                    const int64_t* __restrict__ ptr, const int32_t* __restrict__ term,
                                                                    const int64_t* __restrict__ tptr, const int32_t* __restrict__ tdoc,
                                                                    int32_t V, int32_t* __restrict__ cnt, int32_t* __restrict__ matched) {
    extern __shared__ int32_t hist[];                            // [V], the LDS arm only
    __shared__ int64_t row_b[REL_CHUNK];
    __shared__ int32_t row_n[REL_CHUNK];
    __shared__ int32_t qterm[2 * REL_MAX_TERMS];                 // the include terms but the driving one, then the exclude terms
    __shared__ int nrows;
    const int tid = threadIdx.x;
    const RelItem it = items[blockIdx.x];
    const RelQuery* __restrict__ Q = queries + it.q;
    const int ninc = Q->ninc, nexc = Q->nexc, drive = Q->drive;
    const int nrest = ninc - (drive >= 0 ? 1 : 0), ntest = nrest + nexc;
    if (tid < ninc) {
        if (tid != drive) qterm[tid - ((drive >= 0 && tid > drive) ? 1 : 0)] = Q->inc[tid];
    } else if (tid < ninc + nexc) {
        qterm[nrest + tid - ninc] = Q->exc[tid - ninc];
    }
    if (tid == 0) nrows = 0;
    if (it.lds)
        for (int t = tid; t < V; t += REL_THREADS) hist[t] = 0;
    const int64_t left = Q->len - it.start;
    const int n = left < REL_CHUNK ? (int)left : REL_CHUNK;
    // ---- phase A: this thread's entries -> documents -> row bounds, requested together
    constexpr int EU = REL_CHUNK / REL_THREADS;
    const int64_t list0 = (drive >= 0 ? tptr[Q->inc[drive]] : 0) + it.start;
    int64_t d[EU], b[EU], e[EU];
#pragma unroll
    for (int u = 0; u < EU; ++u) {
        const int i = tid + u * REL_THREADS;
        d[u] = i < n ? (drive >= 0 ? (int64_t)tdoc[list0 + i] : list0 + i) : -1;
    }
#pragma unroll
    for (int u = 0; u < EU; ++u) {
        b[u] = d[u] >= 0 ? ptr[d[u]] : 0;
        e[u] = d[u] >= 0 ? ptr[d[u] + 1] : 0;
    }
    __syncthreads();                                             // qterm, nrows, hist
#pragma unroll
    for (int u = 0; u < EU; ++u) {
        if (d[u] < 0) continue;
        bool ok = true;
        if (ntest > 0) {
            int hits = 0;
            for (int64_t i = b[u]; i < e[u]; ++i) {
                const int32_t t = term[i];
                for (int x = 0; x < nrest; ++x) hits += t == qterm[x] ? 1 : 0;       // a row's terms are distinct, and so are a list's
                for (int x = nrest; x < ntest; ++x) ok = ok && t != qterm[x];
            }
            ok = ok && hits == nrest;
        }
        if (ok) {
            const int slot = atomicAdd(&nrows, 1);               // at most n <= REL_CHUNK appends
            row_b[slot] = b[u];
            row_n[slot] = (int32_t)(e[u] - b[u]);
        }
    }
    __syncthreads();
    const int nr = nrows;
    if (nr == 0) return;                                         // uniform
    int32_t* __restrict__ row = cnt + (int64_t)it.q * V;
    if (tid == 0) atomicAdd(&matched[it.q], nr);
    // ---- phase B
    if (it.lds) {
        rel_add_rows(hist, term, row_b, row_n, nr);
        __syncthreads();
        for (int t = tid; t < V; t += REL_THREADS) {
            const int32_t v = hist[t];
            if (v) atomicAdd(&row[t], v);
        }
    } else {
        rel_add_rows(row, term, row_b, row_n, nr);
    }
}

__device__ __forceinline__ bool rel_in_list(const int32_t* __restrict__ list, int n, int32_t u) {
    bool in = false;
    for (int i = 0; i < n; ++i) in = in || list[i] == u;
    return in;
}

__global__ __launch_bounds__(256) void related_score_kernel(const RelQuery* __restrict__ queries, const int32_t* __restrict__ cnt,
                                                            const int32_t* __restrict__ matched, const int64_t* __restrict__ tptr, int32_t V,
                                                            int64_t D, int measure, int64_t min_count, double* __restrict__ score) {
    const int q = blockIdx.y;
    const int32_t u = blockIdx.x * 256 + threadIdx.x;
    if (u >= V) return;
    const RelQuery* __restrict__ Q = queries + q;
    const int64_t c = cnt[(int64_t)q * V + u];
    double s = -INFINITY;
    if (c >= (min_count > 1 ? min_count : 1) && !rel_in_list(Q->inc, Q->ninc, u) && !rel_in_list(Q->exc, Q->nexc, u)) {
        const int64_t n = matched[q], df = tptr[u + 1] - tptr[u];
        if (measure == HIPTS_RELATED_COUNT) s = (double)c;
        else if (measure == HIPTS_RELATED_JACCARD) s = (double)c / (double)(n + df - c);
        else s = ((double)c / (double)n) / ((double)df / (double)D);
    }
    score[(int64_t)q * V + u] = s;
}

// vals / ids: [nq][kk] as the top-k left them.  A -inf result is no candidate: its id becomes -1 and its count 0.
__global__ __launch_bounds__(256) void related_finish_kernel(const double* __restrict__ vals, int32_t* __restrict__ ids, const int32_t* __restrict__ cnt,
                                                             const int32_t* __restrict__ matched, int32_t V, int kk, int nq,
                                                             int64_t* __restrict__ counts, int32_t* __restrict__ matched_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, total = (int64_t)nq * kk;
    if (i >= total) return;
    if (i < nq) matched_out[i] = matched[i];                     // (kk >= 1: there are at least nq threads)
    const int64_t q = i / kk;
    const bool cand = vals[i] > -INFINITY;
    const int32_t id = ids[i];
    counts[i] = cand ? (int64_t)cnt[q * V + id] : 0;
    if (!cand) ids[i] = -1;
}

// a list of a query: at most REL_MAX_TERMS ids inside [0, V)
int rel_check_list(const int32_t* terms, const int32_t* ptr, int nq, int32_t V, const char* what) {
    HIPTS_REQUIRE(ptr[0] >= 0, "hipts_bm25_related: %s_ptr[0] is negative", what);
    for (int q = 0; q < nq; ++q) {
        const int64_t n = (int64_t)ptr[q + 1] - ptr[q];
        HIPTS_REQUIRE(n >= 0 && n <= REL_MAX_TERMS, "hipts_bm25_related: query %d has %lld %s terms (at most %d)", q, (long long)n, what,
                      REL_MAX_TERMS);
        HIPTS_REQUIRE(n == 0 || terms, "hipts_bm25_related: %s_terms is NULL", what);
        for (int i = ptr[q]; i < ptr[q + 1]; ++i)
            HIPTS_REQUIRE(terms[i] >= 0 && terms[i] < V, "hipts_bm25_related: query %d: term id %d outside [0, %d)", q, terms[i], V);
    }
    return HIPTS_OK;
}

// distinct ids of terms[b, e) in their order
int rel_copy_distinct(const int32_t* terms, int b, int e, int32_t* out) {
    int n = 0;
    for (int i = b; i < e; ++i)
        if (std::find(out, out + n, terms[i]) == out + n) out[n++] = terms[i];
    return n;
}

int64_t rel_direct_max() {
    const char* e = getenv("HIPTS_RELATED_DIRECT_MAX");
    return e && *e ? atoll(e) : REL_DIRECT_MAX;
}

}  // namespace

extern "C" {

int hipts_bm25_related(hipts_bm25_t* h, const int32_t* inc_terms, const int32_t* inc_ptr, const int32_t* exc_terms, const int32_t* exc_ptr,
                       int nq, int measure, int64_t min_count, int k, int32_t* ids_out, double* scores_out, int64_t* counts_out,
                       int64_t* matched_out, void* stream) {
    HIPTS_REQUIRE(h && inc_ptr && exc_ptr && ids_out && scores_out && counts_out && matched_out && nq >= 1,
                  "hipts_bm25_related: bad arguments");
    HIPTS_REQUIRE(k >= 1 && k <= REL_MAX_K, "hipts_bm25_related: k must be in [1, %d]", REL_MAX_K);
    HIPTS_REQUIRE(measure == HIPTS_RELATED_COUNT || measure == HIPTS_RELATED_JACCARD || measure == HIPTS_RELATED_LIFT,
                  "hipts_bm25_related: unknown measure %d", measure);
    const int32_t V = h->V;
    const int64_t D = h->D;
    HIPTS_REQUIRE(D < (1ll << 31), "hipts_bm25_related: too many documents");
    HIPTS_TRY(rel_check_list(inc_terms, inc_ptr, nq, V, "include"));
    HIPTS_TRY(rel_check_list(exc_terms, exc_ptr, nq, V, "exclude"));
    h->rel_count_ms = 0.0;
    h->rel_items[0] = h->rel_items[1] = 0;
    for (int64_t i = 0; i < (int64_t)nq * k; ++i) {
        ids_out[i] = -1;
        scores_out[i] = -INFINITY;
        counts_out[i] = 0;
    }
    if (V == 0) {                                                // no term can be named: every query is the empty one
        for (int q = 0; q < nq; ++q) matched_out[q] = D;
        return HIPTS_OK;
    }
    HIPTS_TRY(use_device(h->device));
    hipStream_t s = (hipStream_t)stream;
    static PerDevice once;
    HIPTS_TRY(allow_dynamic_lds(once, h->device, REL_LDS_MAX_V * 4, related_count_kernel));
    for (auto& ev : h->rel_ev)
        if (!ev) HIPTS_HIP(hipEventCreate(&ev));
    const bool lds_fits = V <= REL_LDS_MAX_V;
    const int64_t direct_max = rel_direct_max();
    const int kk = (int)std::min<int64_t>(k, V);
    for (int q0 = 0; q0 < nq; q0 += REL_PASS) {
        const int np = std::min(REL_PASS, nq - q0);
        // ---- the pass's descriptors and work items
        std::vector<RelQuery> queries((size_t)np);
        std::vector<RelItem> items;
        for (int j = 0; j < np; ++j) {
            RelQuery& Q = queries[j];
            memset(&Q, 0, sizeof(Q));
            Q.ninc = rel_copy_distinct(inc_terms, inc_ptr[q0 + j], inc_ptr[q0 + j + 1], Q.inc);
            Q.nexc = rel_copy_distinct(exc_terms, exc_ptr[q0 + j], exc_ptr[q0 + j + 1], Q.exc);
            Q.drive = -1;
            Q.len = D;
            for (int i = 0; i < Q.ninc; ++i)
                if (Q.drive < 0 || h->h_df[Q.inc[i]] < Q.len) {
                    Q.drive = i;
                    Q.len = h->h_df[Q.inc[i]];
                }
            for (int i = 0; i < Q.ninc; ++i)                     // a term in both lists: nothing matches
                if (std::find(Q.exc, Q.exc + Q.nexc, Q.inc[i]) != Q.exc + Q.nexc) Q.len = 0;
            const int lds = (lds_fits && Q.len > direct_max) ? 1 : 0;
            for (int64_t st = 0; st < Q.len; st += REL_CHUNK) items.push_back(RelItem{j, lds, st});
            h->rel_items[lds ? 0 : 1] += (Q.len + REL_CHUNK - 1) / REL_CHUNK;
        }
        const size_t q_bytes = queries.size() * sizeof(RelQuery), i_bytes = items.size() * sizeof(RelItem);
        HIPTS_TRY(h->pin_rel_in.reserve(q_bytes + i_bytes));
        memcpy(h->pin_rel_in.p, queries.data(), q_bytes);
        if (i_bytes) memcpy(h->pin_rel_in.as<char>() + q_bytes, items.data(), i_bytes);
        HIPTS_TRY(h->ws_rel_in.reserve(q_bytes + i_bytes));
        const size_t cnt_bytes = (size_t)np * V * 4 + (size_t)np * 4;         // count rows, then the matched counts
        HIPTS_TRY(h->ws_rel_cnt.reserve(cnt_bytes));
        HIPTS_TRY(h->ws_rel_score.reserve((size_t)np * V * 8));
        const size_t nres = (size_t)np * kk;
        const size_t out_bytes = nres * 20 + (size_t)np * 4;                  // scores, counts, ids, matched
        HIPTS_TRY(h->ws_rel_out.reserve(out_bytes));
        HIPTS_TRY(h->pin_rel_out.reserve(out_bytes));
        const RelQuery* d_q = h->ws_rel_in.as<RelQuery>();
        const RelItem* d_items = reinterpret_cast<const RelItem*>(h->ws_rel_in.as<char>() + q_bytes);
        int32_t* d_cnt = h->ws_rel_cnt.as<int32_t>();
        int32_t* d_matched = d_cnt + (size_t)np * V;
        double* d_score = h->ws_rel_score.as<double>();
        double* d_vals = h->ws_rel_out.as<double>();
        int64_t* d_counts = reinterpret_cast<int64_t*>(d_vals + nres);
        int32_t* d_ids = reinterpret_cast<int32_t*>(d_counts + nres);
        HIPTS_HIP(hipMemcpyAsync(h->ws_rel_in.p, h->pin_rel_in.p, q_bytes + i_bytes, hipMemcpyHostToDevice, s));
        HIPTS_HIP(hipMemsetAsync(d_cnt, 0, cnt_bytes, s));
        // ---- count, score, rank, gather
        HIPTS_HIP(hipEventRecord(h->rel_ev[0], s));
        if (!items.empty()) {
            related_count_kernel<<<(unsigned)items.size(), REL_THREADS, lds_fits ? (size_t)V * 4 : 0, s>>>(
                d_q, d_items, h->d_ptr.as<int64_t>(), h->d_term.as<int32_t>(), h->d_tptr.as<int64_t>(), h->d_tdoc.as<int32_t>(), V, d_cnt,
                d_matched);
            HIPTS_LAUNCH_CHECK();
        }
        HIPTS_HIP(hipEventRecord(h->rel_ev[1], s));
        related_score_kernel<<<dim3(ceil_div(V, 256), np), 256, 0, s>>>(d_q, d_cnt, d_matched, h->d_tptr.as<int64_t>(), V, D, measure, min_count,
                                                                       d_score);
        HIPTS_LAUNCH_CHECK();
        HIPTS_TRY(hipts_topk(d_score, np, V, kk, d_ids, d_vals, HIPTS_DEVICE, h->device, stream));
        related_finish_kernel<<<ceil_div((int64_t)nres, 256), 256, 0, s>>>(d_vals, d_ids, d_cnt, d_matched, V, kk, np, d_counts, d_ids + nres);
        HIPTS_LAUNCH_CHECK();
        HIPTS_HIP(hipMemcpyAsync(h->pin_rel_out.p, d_vals, out_bytes, hipMemcpyDeviceToHost, s));
        HIPTS_HIP(hipStreamSynchronize(s));
        float ms = 0.0f;
        HIPTS_HIP(hipEventElapsedTime(&ms, h->rel_ev[0], h->rel_ev[1]));
        h->rel_count_ms += ms;
        const double* hv = h->pin_rel_out.as<double>();
        const int64_t* hc = reinterpret_cast<const int64_t*>(hv + nres);
        const int32_t* hi = reinterpret_cast<const int32_t*>(hc + nres);
        const int32_t* hm = hi + nres;
        for (int j = 0; j < np; ++j) {
            matched_out[q0 + j] = hm[j];
            for (int i = 0; i < kk; ++i) {
                const size_t o = (size_t)(q0 + j) * k + i, r = (size_t)j * kk + i;
                ids_out[o] = hi[r];
                scores_out[o] = hv[r];
                counts_out[o] = hc[r];
            }
        }
    }
    return HIPTS_OK;
}

int hiptsdbg_related_last(const hipts_bm25_t* h, double* count_ms, int64_t* lds_items, int64_t* direct_items) {
    HIPTS_REQUIRE(h, "null handle");
    if (count_ms) *count_ms = h->rel_count_ms;
    if (lds_items) *lds_items = h->rel_items[0];
    if (direct_items) *direct_items = h->rel_items[1];
    return HIPTS_OK;
}

}  // extern "C"
