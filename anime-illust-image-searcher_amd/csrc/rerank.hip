// rerank.hip -- the finishing stage of the normal-mode rerank for a batch of queries: division by the maximum, the pinned top ten,
// removal of their duplicates, the gap filter and the cut to topn, one workgroup per query.
//
// Reference behaviour followed (file:line relative to the reference repository):
//   rf / rf.max() when the maximum is positive          webui.py:210-211
//   the top ten pinned at 1.0, the rest without them    webui.py:217-237
//   filter_searched_result                              webui.py:63-80
//
// Input is the ranked prefix hipts_topk made of  rf = 0.7 * final + 0.3 * rs  (k = min(1024, D) entries per query, device memory)
// and the ids of the first stage's top ten.  A workgroup of 1024 threads holds one ranked entry per thread and the whole list
// F = ten pinned pairs + the rest in LDS; the two ordered compactions (the rest, the emitted entries) are block_excl_scan's.
//
// The gap filter cuts the FULL ranked list at its second cut point (at the only one if there is one, nowhere if there is none), so a
// prefix decides the result only in three cases, and the kernel reports which one held (status 0) or that none did (status 1):
//   * two cut points lie inside the prefix: the list ends at the second, whatever follows;
//   * the prefix is exhausted (k == n, or its last value is -inf: only -inf scores follow, which make no cut point and fail `> 0`);
//   * topn entries were emitted from the indices that are certain in any continuation: below the first cut point when the prefix
//     holds one (the full list ends there or at a later, still unknown second one), below L - 1 when it holds none (the gap after
//     the last entry of the prefix is not known yet).
// This file is compiled with -ffp-contract=off; v / mx is an IEEE double division, the bits of numpy's  rvals / mx.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"
#include "rank_util.h"

using namespace hipts;

namespace {

constexpr int RF_THREADS = 1024;                 // = the largest k of hipts_topk: one ranked entry per thread
constexpr int RF_PIN = 10;                       // webui.py:217: the first stage's top ten
constexpr int RF_MAXL = RF_PIN + RF_THREADS;
constexpr double RF_DIFF_THRESH = 1e-6;          // webui.py:58 DIFF_FILTER_THRESH

__global__ __launch_bounds__(RF_THREADS) void rerank_finish_kernel(const int32_t* __restrict__ ranked_ids, const double* __restrict__ ranked_vals, int k,
                                                                   int k_is_n, const int32_t* __restrict__ top10, int topn, int cap,
                                                                   int32_t* __restrict__ docs_out, double* __restrict__ scores_out,
                                                                   int32_t* __restrict__ counts_out, int32_t* __restrict__ status_out) {
    __shared__ double f_score[RF_MAXL];
    __shared__ int32_t f_id[RF_MAXL];
    __shared__ int32_t s_top[RF_PIN];
    __shared__ int scratch[17];
    __shared__ int s_cut[2];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int32_t* ids = ranked_ids + q * k;
    const double* vals = ranked_vals + q * k;
    if (tid < RF_PIN) {
        const int32_t d = top10[q * RF_PIN + tid];
        s_top[tid] = d;
        f_id[tid] = d;
        f_score[tid] = 1.0;
    }
    if (tid < 2) s_cut[tid] = INT_MAX;
    __syncthreads();
    // the maximum is the first ranked value; the division only when it is positive (webui.py:210-211)
    const double mx = vals[0];
    const bool have = tid < k;
    const int32_t id = have ? ids[tid] : -1;
    double v = have ? vals[tid] : 0.0;
    if (mx > 0.0) v = v / mx;
    bool keep = have;
#pragma unroll
    for (int j = 0; j < RF_PIN; ++j)
        if (s_top[j] == id) keep = false;
    int m;
    const int pos = block_excl_scan<int>(keep ? 1 : 0, scratch, &m);
    if (keep) {                                  // RF_PIN + pos < RF_PIN + k <= RF_MAXL
        f_id[RF_PIN + pos] = id;
        f_score[RF_PIN + pos] = v;
    }
    const int L = RF_PIN + m;
    __syncthreads();
    // cut points: neighbours closer than the threshold without being equal; a NaN difference (-inf - -inf) compares false
    auto is_cut = [&](int i) {
        const double d = f_score[i] - f_score[i + 1];
        return d != 0.0 && d < RF_DIFF_THRESH;
    };
    for (int i = tid; i < L - 1; i += RF_THREADS)
        if (is_cut(i)) atomicMin(&s_cut[0], i);
    __syncthreads();
    const int c1 = s_cut[0];
    for (int i = tid; i < L - 1; i += RF_THREADS)
        if (i > c1 && is_cut(i)) atomicMin(&s_cut[1], i);
    __syncthreads();
    const int c2 = s_cut[1];
    const bool one = c1 != INT_MAX, two = c2 != INT_MAX;
    const bool exhausted = k_is_n || vals[k - 1] == -INFINITY;
    // two cuts: the second.  Otherwise an exhausted prefix is the whole list (the only cut, or its end); an unexhausted one is certain
    // below its only cut, or below its last entry when it has none.
    const int t = two ? c2 : one ? c1 : exhausted ? L : L - 1;
    // emit the entries below t with a positive score, in order: index tid, then the up to RF_PIN indices from RF_THREADS on
    const bool e0 = tid < t && f_score[tid] > 0.0;
    const int i1 = RF_THREADS + tid;
    const bool e1 = i1 < L && i1 < t && f_score[i1] > 0.0;
    int n0, n1;
    const int p0 = block_excl_scan<int>(e0 ? 1 : 0, scratch, &n0);
    const int p1 = n0 + block_excl_scan<int>(e1 ? 1 : 0, scratch, &n1);
    const int emitted = n0 + n1;
    int32_t* docs = docs_out + q * cap;
    double* scores = scores_out + q * cap;
    if (e0 && p0 < topn) {                       // p0 < min(topn, L) <= cap
        docs[p0] = f_id[tid];
        scores[p0] = f_score[tid];
    }
    if (e1 && p1 < topn) {
        docs[p1] = f_id[i1];
        scores[p1] = f_score[i1];
    }
    if (tid == 0) {
        counts_out[q] = emitted < topn ? emitted : topn;
        status_out[q] = (two || exhausted || emitted >= topn) ? 0 : 1;
    }
}

// device and pinned staging of the call, per device; never destroyed (as scratch_buf() in query.hip: the runtime may be gone first)
struct FinishBufs {
    DevBuf d_top10, d_out;
    PinBuf pin_top10, pin_out;
};
FinishBufs& finish_bufs(int device) {
    static FinishBufs* bufs = new FinishBufs[64];
    return bufs[device & 63];
}

}  // namespace

extern "C" int hipts_rerank_finish(const int32_t* ranked_ids, const double* ranked_vals, int nq, int k, int64_t n, const int32_t* top10, int topn,
                                   int32_t* docs_out, double* scores_out, int32_t* counts_out, int32_t* status_out, int device, void* stream) {
    HIPTS_REQUIRE(ranked_ids && ranked_vals && top10 && docs_out && scores_out && counts_out && status_out && nq >= 1,
                  "hipts_rerank_finish: bad arguments");
    HIPTS_REQUIRE(n > RF_PIN, "hipts_rerank_finish: n must exceed %d (smaller corpora are not reranked, webui.py:247-253)", RF_PIN);
    HIPTS_REQUIRE(k >= 1 && k <= RF_THREADS && k <= n, "hipts_rerank_finish: k must be in [1, min(%d, n)]", RF_THREADS);
    HIPTS_REQUIRE(topn >= 1, "hipts_rerank_finish: topn must be positive");
    for (int64_t i = 0; i < (int64_t)nq * RF_PIN; ++i)
        HIPTS_REQUIRE(top10[i] >= 0 && top10[i] < n, "hipts_rerank_finish: top10[%lld] = %d is no document id", (long long)i, top10[i]);
    HIPTS_TRY(use_device(device));
    hipStream_t s = (hipStream_t)stream;
    const int cap = std::min(topn, RF_PIN + k);
    FinishBufs& B = finish_bufs(device);
    // outputs in one block: scores float64 [nq][cap] | docs int32 [nq][cap] | counts int32 [nq] | status int32 [nq]
    const size_t n_out = (size_t)nq * cap;
    const size_t off_docs = n_out * 8, off_counts = off_docs + n_out * 4, off_status = off_counts + (size_t)nq * 4;
    const size_t out_bytes = off_status + (size_t)nq * 4;
    const size_t top_bytes = (size_t)nq * RF_PIN * 4;
    HIPTS_TRY(B.d_top10.reserve(top_bytes));
    HIPTS_TRY(B.pin_top10.reserve(top_bytes));
    HIPTS_TRY(B.d_out.reserve(out_bytes));
    HIPTS_TRY(B.pin_out.reserve(out_bytes));
    memcpy(B.pin_top10.p, top10, top_bytes);
    HIPTS_HIP(hipMemcpyAsync(B.d_top10.p, B.pin_top10.p, top_bytes, hipMemcpyHostToDevice, s));
    char* d = B.d_out.as<char>();
    rerank_finish_kernel<<<nq, RF_THREADS, 0, s>>>(ranked_ids, ranked_vals, k, k == n ? 1 : 0, B.d_top10.as<int32_t>(), topn, cap,
                                                   reinterpret_cast<int32_t*>(d + off_docs), reinterpret_cast<double*>(d),
                                                   reinterpret_cast<int32_t*>(d + off_counts), reinterpret_cast<int32_t*>(d + off_status));
    HIPTS_LAUNCH_CHECK();
    HIPTS_HIP(hipMemcpyAsync(B.pin_out.p, d, out_bytes, hipMemcpyDeviceToHost, s));
    HIPTS_HIP(hipStreamSynchronize(s));          // the one synchronisation of the call
    const char* h = B.pin_out.as<char>();
    memcpy(counts_out, h + off_counts, (size_t)nq * 4);
    memcpy(status_out, h + off_status, (size_t)nq * 4);
    // only the emitted entries are defined; the caller's rows beyond counts_out[q] are left as they are
    for (int q = 0; q < nq; ++q) {
        const size_t c = (size_t)counts_out[q], o = (size_t)q * cap;
        memcpy(scores_out + o, h + o * 8, c * 8);
        memcpy(docs_out + o, h + off_docs + o * 4, c * 4);
    }
    return HIPTS_OK;
}
