// crerank.hip -- character-oriented rerank after the feature-index product: threshold, tag filter and ranking on the device.
//
// Reference behaviour followed (file:line relative to the reference repository):
//   difference < threshold, required / excluded tags    webui.py:311-328
//   sort by similarity, best first                      webui.py:330   (stable: ties keep ascending feature-row order)
//
// Per query three stages on one stream, no host synchronisation between them:
//   1. filter    one thread per feature row: threshold, then row_doc >= 0, then the row's tag ids against the query's required and
//                excluded ids in LDS; the wave's 64-bit ballot and the workgroup's survivor count are stored
//   2. compact   scan of the workgroup counts, then every survivor finds its place from the ballots (lane prefix inside the wave):
//                (row, ~order key of the float32 score) in ascending row order, plus the count
//   3. rank      by (score descending, row ascending): up to CR_SMALL survivors one workgroup sorts composite 64-bit keys in LDS;
//                more go through a stable LSD radix sort (four 8-bit digits of the inverted order key, so ascending = best first);
//                the last step writes doc id (int32) and score (float64)
// The product itself is hipts_index_query's (device output); this file is compiled with -ffp-contract=off and the two float32
// subtractions  diff = 1 - sim,  score = 1 - diff  are kept as two plain operations.
#include <algorithm>
#include <vector>

#include "common.h"
#include "rank_util.h"

using namespace hipts;

struct hipts_crerank {
    int device = 0;
    int64_t rows = 0, ntags = 0;
    DevBuf d_row_doc, d_row_tag_ptr, d_row_tags;      // int32 [rows], int64 [rows + 1], int32 [ntags]
    DevBuf ws_sim;                                    // float [nq][rows]: the index products
    DevBuf ws_args;                                   // per run: thresholds, tag-id CSR of the queries
    DevBuf ws_mask, ws_bcount;                        // uint64 [ceil(rows / 64)] ballots, uint32 [filter workgroups] counts -> offsets
    DevBuf ws_key[2], ws_row[2];                      // uint32 [rows] each: survivors, ping-pong of the radix passes
    DevBuf ws_hist;                                   // uint32 [256][radix workgroups]
    DevBuf d_count;                                   // uint32 [nq]
    DevBuf out_docs, out_scores;                      // int32 [nq][rows], float64 [nq][rows]: ranked survivors of the last run
    PinBuf pin_args, pin_count;
    std::vector<int64_t> counts;                      // of the last run
};

namespace {

constexpr int CR_FILTER_THREADS = 256;
constexpr int CR_SMALL = 2048;           // up to this many survivors: one workgroup, bitonic sort in LDS
constexpr int CR_TILE = 1024;            // survivors per workgroup of a radix pass (one per thread)

// ---------------------------------------------------------------------------------------------
// 1. filter
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CR_FILTER_THREADS) void crerank_filter_kernel(const float* __restrict__ sim, int64_t rows, const float* __restrict__ thresholds,
                                                                           int q, const int32_t* __restrict__ row_doc,
                                                                           const int64_t* __restrict__ row_tag_ptr, const int32_t* __restrict__ row_tags,
                                                                           const int32_t* __restrict__ req_ptr, const int32_t* __restrict__ req_ids,
                                                                           const int32_t* __restrict__ exc_ptr, const int32_t* __restrict__ exc_ids,
                                                                           uint64_t* __restrict__ masks, uint32_t* __restrict__ bcount) {
    __shared__ int32_t s_req[HIPTS_CRERANK_MAX_TAGS], s_exc[HIPTS_CRERANK_MAX_TAGS];
    __shared__ uint32_t s_wc[CR_FILTER_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rb = req_ptr[q], nreq = req_ptr[q + 1] - rb, eb = exc_ptr[q], nexc = exc_ptr[q + 1] - eb;     // <= HIPTS_CRERANK_MAX_TAGS (checked on the host)
    if (tid < nreq) s_req[tid] = req_ids[rb + tid];
    if (tid < nexc) s_exc[tid] = exc_ids[eb + tid];
    __syncthreads();
    const float thr = thresholds[q];
    const int64_t r = (int64_t)blockIdx.x * CR_FILTER_THREADS + tid;
    bool pass = false;
    if (r < rows) {
        const float diff = 1.0f - sim[r];
        pass = diff < thr;                                   // float32 comparison
        if (pass) pass = row_doc[r] >= 0;                    // the path occurs in the tag file
        if (pass && (nreq | nexc)) {
            const int64_t b = row_tag_ptr[r], e = row_tag_ptr[r + 1];
            uint64_t found = 0;
            bool excluded = false;
            for (int64_t i = b; i < e; ++i) {
                const int32_t t = row_tags[i];
                for (int j = 0; j < nreq; ++j)
                    if (s_req[j] == t) found |= 1ull << j;
                for (int j = 0; j < nexc; ++j)
                    if (s_exc[j] == t) excluded = true;
            }
            // a negative required id (a tag the file does not know) matches no row: its bit stays clear
            const uint64_t all = nreq == 64 ? ~0ull : ((1ull << nreq) - 1);
            pass = found == all && !excluded;
        }
    }
    const uint64_t m = __ballot(pass);
    if (lane == 0) {
        const int64_t w = (int64_t)blockIdx.x * (CR_FILTER_THREADS / 64) + wave;
        if (w * 64 < rows) masks[w] = m;
        s_wc[wave] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < CR_FILTER_THREADS / 64; ++w) c += s_wc[w];
        bcount[blockIdx.x] = c;
    }
}

// ---------------------------------------------------------------------------------------------
// 2. compaction: counts -> offsets (one workgroup), then the ordered scatter
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void crerank_offsets_kernel(uint32_t* __restrict__ bcount, int nblocks, uint32_t* __restrict__ count_out) {
    __shared__ uint32_t scratch[17];
    uint32_t carry = 0;
    for (int b0 = 0; b0 < nblocks; b0 += 1024) {
        const int b = b0 + threadIdx.x;
        const uint32_t c = b < nblocks ? bcount[b] : 0u;
        uint32_t total;
        const uint32_t ex = block_excl_scan(c, scratch, &total);
        if (b < nblocks) bcount[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *count_out = carry;
}

__global__ __launch_bounds__(CR_FILTER_THREADS) void crerank_compact_kernel(const float* __restrict__ sim, int64_t rows, const uint64_t* __restrict__ masks,
                                                                            const uint32_t* __restrict__ boff, uint32_t* __restrict__ rows_out,
                                                                            uint32_t* __restrict__ keys_out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = (int64_t)blockIdx.x * CR_FILTER_THREADS + tid;
    if (r >= rows) return;
    const int64_t w0 = (int64_t)blockIdx.x * (CR_FILTER_THREADS / 64);
    const uint64_t m = masks[w0 + wave];
    if (!((m >> lane) & 1)) return;
    uint32_t pos = boff[blockIdx.x];
    for (int w = 0; w < wave; ++w) pos += (uint32_t)__popcll(masks[w0 + w]);      // earlier waves of this workgroup (all inside `rows`)
    pos += (uint32_t)__popcll(m & ((1ull << lane) - 1));                          // lane prefix
    const float diff = 1.0f - sim[r];
    const float score = 1.0f - diff;
    rows_out[pos] = (uint32_t)r;
    keys_out[pos] = ~float_order_key(score);                                        // ascending key = descending score
}

// ---------------------------------------------------------------------------------------------
// 3a. ranking, small counts: one workgroup, composite keys (inverted score key, row) in LDS, bitonic sort
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void crerank_sort_small_kernel(const uint32_t* __restrict__ count_p, const uint32_t* __restrict__ rows_in,
                                                                  const uint32_t* __restrict__ keys_in, const int32_t* __restrict__ row_doc,
                                                                  int32_t* __restrict__ docs_out, double* __restrict__ scores_out) {
    __shared__ uint64_t ck[CR_SMALL];
    const int tid = threadIdx.x;
    const uint32_t n = *count_p;
    if (n == 0 || n > CR_SMALL) return;                     // uniform
    uint32_t P = 64;
    while (P < n) P <<= 1;
    for (uint32_t i = tid; i < P; i += 1024) ck[i] = i < n ? ((uint64_t)keys_in[i] << 32) | rows_in[i] : ~0ull;
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < P; i += 1024) {
                const uint32_t x = i ^ j;
                if (x > i) {
                    const uint64_t a = ck[i], b = ck[x];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) {
                        ck[i] = b;
                        ck[x] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = tid; i < n; i += 1024) {
        const uint64_t c = ck[i];
        docs_out[i] = row_doc[(uint32_t)c];
        scores_out[i] = (double)float_from_key(~(uint32_t)(c >> 32));
    }
}

// ---------------------------------------------------------------------------------------------
// 3b. ranking, large counts: stable LSD radix sort, 8-bit digits, CR_TILE survivors per workgroup
// ---------------------------------------------------------------------------------------------
// the lanes of this wave that hold the same digit (among the valid ones)
__device__ __forceinline__ uint64_t wave_peers(uint32_t d, bool valid) {
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const uint64_t m = __ballot((d >> b) & 1);
        peers &= ((d >> b) & 1) ? m : ~m;
    }
    return peers;
}

// hist[d][workgroup]: how many of the workgroup's survivors carry digit d
__global__ __launch_bounds__(CR_TILE) void crerank_radix_hist_kernel(const uint32_t* __restrict__ count_p, const uint32_t* __restrict__ keys, int shift,
                                                                     uint32_t* __restrict__ hist, int hist_ld) {
    __shared__ uint32_t h[256];
    const uint32_t n = *count_p;
    if (n <= CR_SMALL || (uint64_t)blockIdx.x * CR_TILE >= n) return;       // uniform
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 256) h[tid] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * CR_TILE + tid;
    const bool valid = i < n;
    const uint32_t d = valid ? (keys[i] >> shift) & 255u : 0u;
    const uint64_t peers = wave_peers(d, valid);
    if (valid && (peers & ((1ull << lane) - 1)) == 0) atomicAdd(&h[d], (uint32_t)__popcll(peers));      // the first lane of each group adds it
    __syncthreads();
    if (tid < 256) hist[(int64_t)tid * hist_ld + blockIdx.x] = h[tid];
}

// exclusive scan over (digit-major, workgroup-minor): where each workgroup's run of each digit starts
__global__ __launch_bounds__(1024) void crerank_radix_scan_kernel(const uint32_t* __restrict__ count_p, uint32_t* __restrict__ hist, int hist_ld) {
    __shared__ uint32_t scratch[17];
    const uint32_t n = *count_p;
    if (n <= CR_SMALL) return;                              // uniform
    const uint32_t nb = (n + CR_TILE - 1) / CR_TILE;
    const uint32_t total = 256u * nb, per = (total + 1023) / 1024;
    const uint32_t i0 = threadIdx.x * per, i1 = min(total, i0 + per);
    uint32_t sum = 0;
    for (uint32_t i = i0; i < i1; ++i) sum += hist[(int64_t)(i / nb) * hist_ld + (i % nb)];
    uint32_t all;
    uint32_t run = block_excl_scan(sum, scratch, &all);
    for (uint32_t i = i0; i < i1; ++i) {
        uint32_t* p = &hist[(int64_t)(i / nb) * hist_ld + (i % nb)];
        const uint32_t c = *p;
        *p = run;
        run += c;
    }
}

// FINAL: the last pass writes doc id and score instead of (key, row)
template <bool FINAL>
__global__ __launch_bounds__(CR_TILE) void crerank_radix_scatter_kernel(const uint32_t* __restrict__ count_p, const uint32_t* __restrict__ keys,
                                                                        const uint32_t* __restrict__ rows_in, int shift, const uint32_t* __restrict__ hist,
                                                                        int hist_ld, uint32_t* __restrict__ keys_out, uint32_t* __restrict__ rows_out,
                                                                        const int32_t* __restrict__ row_doc, int32_t* __restrict__ docs_out,
                                                                        double* __restrict__ scores_out) {
    __shared__ uint32_t wc[CR_TILE / 64][256];              // per wave and digit: count, then the count of the earlier waves
    __shared__ uint32_t base[256];
    const uint32_t n = *count_p;
    if (n <= CR_SMALL || (uint64_t)blockIdx.x * CR_TILE >= n) return;       // uniform
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < (CR_TILE / 64) * 256; i += CR_TILE) (&wc[0][0])[i] = 0;
    if (tid < 256) base[tid] = hist[(int64_t)tid * hist_ld + blockIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * CR_TILE + tid;
    const bool valid = i < n;
    const uint32_t key = valid ? keys[i] : 0u, row = valid ? rows_in[i] : 0u;
    const uint32_t d = (key >> shift) & 255u;
    const uint64_t peers = wave_peers(d, valid);
    const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1));
    if (valid && rank == 0) wc[wave][d] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (tid < 256) {
        uint32_t run = 0;
#pragma unroll
        for (int w = 0; w < CR_TILE / 64; ++w) {
            const uint32_t c = wc[w][tid];
            wc[w][tid] = run;
            run += c;
        }
    }
    __syncthreads();
    if (!valid) return;
    const uint32_t pos = base[d] + wc[wave][d] + rank;     // < n: the scanned histograms sum to n
    if (FINAL) {
        docs_out[pos] = row_doc[row];
        scores_out[pos] = (double)float_from_key(~key);
    } else {
        keys_out[pos] = key;
        rows_out[pos] = row;
    }
}

int copy_csr(const int32_t* ptr, const int32_t* ids, int nq, const char* what, int32_t* dst_ptr, int32_t* dst_ids) {
    HIPTS_REQUIRE(ptr[0] == 0, "hipts_crerank_run: %s_ptr[0] must be 0", what);
    for (int q = 0; q < nq; ++q) {
        const int n = ptr[q + 1] - ptr[q];
        HIPTS_REQUIRE(n >= 0, "hipts_crerank_run: %s_ptr is not ascending", what);
        HIPTS_REQUIRE(n <= HIPTS_CRERANK_MAX_TAGS, "hipts_crerank_run: query %d carries %d %s tags, more than HIPTS_CRERANK_MAX_TAGS = %d", q, n,
                      what, HIPTS_CRERANK_MAX_TAGS);
    }
    memcpy(dst_ptr, ptr, (size_t)(nq + 1) * 4);
    if (ptr[nq] > 0) {
        HIPTS_REQUIRE(ids, "hipts_crerank_run: %s_ids is null", what);
        memcpy(dst_ids, ids, (size_t)ptr[nq] * 4);
    }
    return HIPTS_OK;
}

}  // namespace

extern "C" {

int hipts_crerank_create(const int32_t* row_doc, const int64_t* row_tag_ptr, const int32_t* row_tags, int64_t rows, int device,
                         hipts_crerank_t** out) {
    HIPTS_REQUIRE(out, "hipts_crerank_create: null output");
    *out = nullptr;
    HIPTS_REQUIRE(row_doc && row_tag_ptr && rows >= 1 && rows < ((int64_t)1 << 31), "hipts_crerank_create: bad arguments");
    HIPTS_REQUIRE(row_tag_ptr[0] == 0, "hipts_crerank_create: row_tag_ptr[0] must be 0");
    for (int64_t r = 0; r < rows; ++r)
        HIPTS_REQUIRE(row_tag_ptr[r + 1] >= row_tag_ptr[r], "hipts_crerank_create: row_tag_ptr is not ascending at row %lld", (long long)r);
    const int64_t ntags = row_tag_ptr[rows];
    HIPTS_REQUIRE(ntags == 0 || row_tags, "hipts_crerank_create: null row_tags");
    HIPTS_TRY(use_device(device));
    hipts_crerank* h = new hipts_crerank();
    h->device = device;
    h->rows = rows;
    h->ntags = ntags;
    const int nfb = ceil_div(rows, CR_FILTER_THREADS), nrb = ceil_div(rows, CR_TILE);
    int st = HIPTS_OK;
    auto ok = [&](int s) { return st == HIPTS_OK && (st = s) == HIPTS_OK; };
    if (ok(h->d_row_doc.alloc((size_t)rows * 4)) && ok(h->d_row_tag_ptr.alloc((size_t)(rows + 1) * 8)) && ok(h->d_row_tags.alloc((size_t)ntags * 4)) &&
        ok(h->ws_mask.alloc((size_t)ceil_div(rows, 64) * 8)) && ok(h->ws_bcount.alloc((size_t)nfb * 4)) && ok(h->ws_hist.alloc((size_t)256 * nrb * 4)) &&
        ok(h->ws_key[0].alloc((size_t)rows * 4)) && ok(h->ws_key[1].alloc((size_t)rows * 4)) && ok(h->ws_row[0].alloc((size_t)rows * 4)) &&
        ok(h->ws_row[1].alloc((size_t)rows * 4)) && ok(upload(h->d_row_doc.p, row_doc, (size_t)rows * 4)) &&
        ok(upload(h->d_row_tag_ptr.p, row_tag_ptr, (size_t)(rows + 1) * 8)))
        ok(upload(h->d_row_tags.p, row_tags, (size_t)ntags * 4));
    if (st != HIPTS_OK) {
        delete h;
        return st;
    }
    *out = h;
    return HIPTS_OK;
}

int hipts_crerank_destroy(hipts_crerank_t* h) {
    if (h) {
        (void)use_device(h->device);
        delete h;
    }
    return HIPTS_OK;
}

int hipts_crerank_run(hipts_crerank_t* h, hipts_index_t* features, const float* queries, int queries_memspace, int nq, const float* thresholds,
                      const int32_t* req_ptr, const int32_t* req_ids, const int32_t* exc_ptr, const int32_t* exc_ids, int64_t* counts_out,
                      void* stream) {
    HIPTS_REQUIRE(h && features && queries && thresholds && req_ptr && exc_ptr && counts_out && nq >= 1, "hipts_crerank_run: bad arguments");
    int64_t len = 0;
    HIPTS_TRY(hipts_index_len(features, &len));
    HIPTS_REQUIRE(len == h->rows, "hipts_crerank_run: the tables were built for %lld rows, the feature index holds %lld", (long long)h->rows,
                  (long long)len);
    HIPTS_TRY(use_device(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int64_t R = h->rows;
    h->counts.clear();
    // the per-query arguments in one block: thresholds [nq] | req_ptr [nq + 1] | exc_ptr [nq + 1] | req_ids | exc_ids
    const size_t nreq = (size_t)req_ptr[nq], nexc = (size_t)exc_ptr[nq];
    const size_t words = (size_t)nq + 2 * ((size_t)nq + 1) + nreq + nexc;
    HIPTS_TRY(h->pin_args.reserve(words * 4));
    HIPTS_TRY(h->ws_args.reserve(words * 4));
    int32_t* pa = h->pin_args.as<int32_t>();
    memcpy(pa, thresholds, (size_t)nq * 4);
    const size_t o_rp = nq, o_ep = o_rp + nq + 1, o_ri = o_ep + nq + 1, o_ei = o_ri + nreq;
    HIPTS_TRY(copy_csr(req_ptr, req_ids, nq, "required", pa + o_rp, pa + o_ri));
    HIPTS_TRY(copy_csr(exc_ptr, exc_ids, nq, "excluded", pa + o_ep, pa + o_ei));
    HIPTS_TRY(h->ws_sim.reserve((size_t)nq * R * 4));
    HIPTS_TRY(h->out_docs.reserve((size_t)nq * R * 4));
    HIPTS_TRY(h->out_scores.reserve((size_t)nq * R * 8));
    HIPTS_TRY(h->d_count.reserve((size_t)nq * 4));
    HIPTS_TRY(h->pin_count.reserve((size_t)nq * 4));
    HIPTS_HIP(hipMemcpyAsync(h->ws_args.p, pa, words * 4, hipMemcpyHostToDevice, s));
    // the product, once for all queries
    HIPTS_TRY(hipts_index_query(features, queries, queries_memspace, nq, h->ws_sim.as<float>(), HIPTS_DEVICE, stream));
    const int32_t* da = h->ws_args.as<int32_t>();
    const float* d_thr = reinterpret_cast<const float*>(da);
    const int nfb = ceil_div(R, CR_FILTER_THREADS), nrb = ceil_div(R, CR_TILE);
    const int32_t* row_doc = h->d_row_doc.as<int32_t>();
    uint32_t* hist = h->ws_hist.as<uint32_t>();
    uint32_t *kA = h->ws_key[0].as<uint32_t>(), *kB = h->ws_key[1].as<uint32_t>(), *rA = h->ws_row[0].as<uint32_t>(), *rB = h->ws_row[1].as<uint32_t>();
    for (int q = 0; q < nq; ++q) {
        const float* sim = h->ws_sim.as<float>() + (int64_t)q * R;
        uint32_t* cnt = h->d_count.as<uint32_t>() + q;
        int32_t* docs = h->out_docs.as<int32_t>() + (int64_t)q * R;
        double* scores = h->out_scores.as<double>() + (int64_t)q * R;
        crerank_filter_kernel<<<nfb, CR_FILTER_THREADS, 0, s>>>(sim, R, d_thr, q, row_doc, h->d_row_tag_ptr.as<int64_t>(), h->d_row_tags.as<int32_t>(),
                                                                da + o_rp, da + o_ri, da + o_ep, da + o_ei, h->ws_mask.as<uint64_t>(),
                                                                h->ws_bcount.as<uint32_t>());
        HIPTS_LAUNCH_CHECK();
        crerank_offsets_kernel<<<1, 1024, 0, s>>>(h->ws_bcount.as<uint32_t>(), nfb, cnt);
        HIPTS_LAUNCH_CHECK();
        crerank_compact_kernel<<<nfb, CR_FILTER_THREADS, 0, s>>>(sim, R, h->ws_mask.as<uint64_t>(), h->ws_bcount.as<uint32_t>(), rA, kA);
        HIPTS_LAUNCH_CHECK();
        crerank_sort_small_kernel<<<1, 1024, 0, s>>>(cnt, rA, kA, row_doc, docs, scores);
        HIPTS_LAUNCH_CHECK();
        if (R > CR_SMALL) {                                  // the count can exceed CR_SMALL only then; the kernels return at once when it does not
            for (int pass = 0; pass < 4; ++pass) {
                const uint32_t *ki = (pass & 1) ? kB : kA, *ri = (pass & 1) ? rB : rA;
                uint32_t *ko = (pass & 1) ? kA : kB, *ro = (pass & 1) ? rA : rB;
                crerank_radix_hist_kernel<<<nrb, CR_TILE, 0, s>>>(cnt, ki, 8 * pass, hist, nrb);
                HIPTS_LAUNCH_CHECK();
                crerank_radix_scan_kernel<<<1, 1024, 0, s>>>(cnt, hist, nrb);
                HIPTS_LAUNCH_CHECK();
                if (pass < 3) crerank_radix_scatter_kernel<false><<<nrb, CR_TILE, 0, s>>>(cnt, ki, ri, 8 * pass, hist, nrb, ko, ro, row_doc, docs, scores);
                else crerank_radix_scatter_kernel<true><<<nrb, CR_TILE, 0, s>>>(cnt, ki, ri, 8 * pass, hist, nrb, ko, ro, row_doc, docs, scores);
                HIPTS_LAUNCH_CHECK();
            }
        }
    }
    HIPTS_HIP(hipMemcpyAsync(h->pin_count.p, h->d_count.p, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
    HIPTS_HIP(hipStreamSynchronize(s));                      // the one synchronisation of a run
    h->counts.resize(nq);
    for (int q = 0; q < nq; ++q) counts_out[q] = h->counts[q] = (int64_t)h->pin_count.as<uint32_t>()[q];
    return HIPTS_OK;
}

int hipts_crerank_read(hipts_crerank_t* h, int query, int64_t first, int64_t count, int32_t* docs_out, double* scores_out) {
    HIPTS_REQUIRE(h && query >= 0 && query < (int)h->counts.size(), "hipts_crerank_read: no such query in the last run");
    HIPTS_REQUIRE(first >= 0 && count >= 0 && first + count <= h->counts[query], "hipts_crerank_read: entries [%lld, %lld) out of range (%lld ranked)",
                  (long long)first, (long long)(first + count), (long long)h->counts[query]);
    if (count == 0) return HIPTS_OK;
    HIPTS_REQUIRE(docs_out && scores_out, "hipts_crerank_read: null output");
    HIPTS_TRY(use_device(h->device));
    const int64_t off = (int64_t)query * h->rows + first;
    HIPTS_HIP(hipMemcpy(docs_out, h->out_docs.as<int32_t>() + off, (size_t)count * 4, hipMemcpyDeviceToHost));
    HIPTS_HIP(hipMemcpy(scores_out, h->out_scores.as<double>() + off, (size_t)count * 8, hipMemcpyDeviceToHost));
    return HIPTS_OK;
}

}  // extern "C"
