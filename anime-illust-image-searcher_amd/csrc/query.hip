// query.hip -- query-scoring path: BM25, dense similarity index, combine, top-k, fused search.
//
// Reference behaviour followed (file:line relative to the reference repository):
//   BM25 statistics      genmodel.py:51-99
//   BM25 scoring         webui.py:119-172
//   index[query]         webui.py:205,352   (gensim Similarity / MatrixSimilarity, dense float32)
//   normalise + combine  webui.py:377-383
//   ranking              webui.py:191-192   (stable sort by -score: ties keep ascending doc id)
//
// All of it is HBM/L2-bound streaming work: coalesced reads, wave reductions,
// no GEMM reshaping except the index product, which uses the exact-f32 MFMA because its fixed
// k-ordered fma chain makes the float32 result bit-reproducible (and equal to the CPU oracle).
// This file is compiled with -ffp-contract=off: every float64 expression below evaluates in
// numpy's operation order with one rounding per operation.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <unordered_map>
#include <vector>

#include "bm25_index.h"
#include "common.h"
#include "query_plan.h"
#include "rank_util.h"
#include "topk.h"
#include "../../include/hip_tagsearch_debug.h"

using namespace hipts;

// =============================================================================================
// BM25
// =============================================================================================

namespace {

constexpr double BM25_K1 = 1.5;    // webui.py:126
constexpr double BM25_B = 0.75;    // webui.py:127
constexpr double REQUIRE_MAGIC = 1000.0;   // webui.py:60

// The BM25 arithmetic of webui.py:139-170, stated once (float64, one rounding per operation, the reference's operation order).
// webui.py:144  k1 * (1 - b + b * (dl / avgdl))   [(1-b) folds to 0.25 exactly]
__device__ __forceinline__ double bm25_length_norm(double dl, double avgdl) {
    return BM25_K1 * ((1.0 - BM25_B) + BM25_B * (dl / avgdl));
}
// webui.py:144-146  idf * (tf * (k1 + 1) / (tf + norm))
__device__ __forceinline__ double bm25_term_score(double idf, double tfd, double nrm) {
    const double denom = tfd + nrm;                          // :144
    const double numer = tfd * (BM25_K1 + 1.0);              // :145
    return idf * (numer / denom);                            // :146
}
// webui.py:154-170, one (document, query term) step of the document-major form: weight w, the term's tf in the document (0 = absent), its score sc
__device__ __forceinline__ void bm25_accumulate(double w, int32_t tfv, double sc, double& s, bool& masked) {
    if (w < 0.0) {                                           // :154-160 exclude
        if (tfv > 0) masked = true;
    } else if (w > REQUIRE_MAGIC) {                          // :161-168 required
        s += (w - REQUIRE_MAGIC) * sc;
        if (tfv == 0) masked = true;
    } else {                                                 // :169-170
        s += w * sc;
    }
}

// One thread per (document, query).  Document-major CSR: the ~20 (term, tf) pairs of a document
// are contiguous, consecutive threads own consecutive documents, so a wave sweeps one contiguous
// span of the postings arrays.
__global__ __launch_bounds__(256) void bm25_score_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ term,
                                                         const int32_t* __restrict__ tf, const int32_t* __restrict__ dl,
                                                         const double* __restrict__ idf, int32_t V, double avgdl, int64_t D,
                                                         const int32_t* __restrict__ q_terms, const double* __restrict__ q_weights,
                                                         const int32_t* __restrict__ q_ptr, double* __restrict__ out) {
    const int q = blockIdx.y;
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    const int qb = q_ptr[q], qe = q_ptr[q + 1];
    const int64_t b = ptr[d], e = ptr[d + 1];
    const double dlv = (double)dl[d];
    const double nrm = bm25_length_norm(dlv, avgdl);
    double s = 0.0;
    bool masked = false;
    for (int j = qb; j < qe; ++j) {
        const int32_t t = q_terms[j];
        const double w = q_weights[j];
        int32_t tfv = 0;
        for (int64_t i = b; i < e; ++i)
            if (term[i] == t) tfv = tf[i];
        const double idf_t = (t >= 0 && t < V) ? idf[t] : 0.0;   // bm25_idf.get(term_id, 0)   :140
        bm25_accumulate(w, tfv, bm25_term_score(idf_t, (double)tfv, nrm), s, masked);
    }
    out[(int64_t)q * D + d] = masked ? -INFINITY : s;
}

// Postings form of the same arithmetic (default): one workgroup per query walks the posting list
// of each query term IN THE QUERY'S TERM ORDER (a barrier between terms keeps the float64 additions
// of one document in the reference's order).  Documents that do not contain a term would add
// idf * (0 / denom) = +0.0, which leaves a non-negative score unchanged, so skipping them is exact.
// Reads sum(df) * 8 B + a few passes over D instead of the whole corpus per query.
// mark[d]: bit 7 = an excluded term is present, low bits = number of required terms present.
#ifdef HIPTS_X_TOPK_STAMPS
__device__ unsigned long long g_bm25_stamps[8];
#define BM25_STAMP(i) do { __syncthreads(); if (blockIdx.x == HIPTS_X_TOPK_STAMPS && threadIdx.x == 0) g_bm25_stamps[i] = wall_clock64(); } while (0)
#else
#define BM25_STAMP(i) do { } while (0)
#endif
// The walk itself, for the documents [lo, hi) of query q's row, by a workgroup of NT threads; term_range(t, b, e) gives the part of term
// t's posting list that lies in that range.  Returns this thread's maximum of the finished scores it read back (-inf when nothing
// asks for it: want_max false and no masking).  ROWS8: lo and hi are known to be multiples of 8 -- the 8-documents-per-step arms only;
// otherwise the row decides, and the scalar arms exist too.  STAMPS: the BM25_STAMP points of the measurement-only build.
template <int NT, bool ROWS8, bool STAMPS, typename TermRange>
__device__ __forceinline__ double bm25_postings_walk(int q, int64_t lo, int64_t hi, TermRange term_range, const int32_t* __restrict__ tdoc,
                                                     const int32_t* __restrict__ ttf, const int32_t* __restrict__ dl,
                                                     const double* __restrict__ idf, int32_t V, double avgdl, int64_t D,
                                                     const int32_t* __restrict__ q_terms, const double* __restrict__ q_weights,
                                                     const int32_t* __restrict__ q_ptr, double* __restrict__ out,
                                                     uint8_t* __restrict__ mark_all, bool want_max) {
    const int tid = threadIdx.x;
    const int qb = q_ptr[q], qe = q_ptr[q + 1];
    double* __restrict__ scores = out + (int64_t)q * D;
    uint8_t* __restrict__ mark = mark_all + (int64_t)q * D;
    int n_required = 0;
    bool masking = false;
    for (int j = qb; j < qe; ++j) {
        const double w = q_weights[j];
        if (w > REQUIRE_MAGIC) ++n_required;
        if (w > REQUIRE_MAGIC || w < 0.0) masking = true;
    }
    if constexpr (STAMPS) BM25_STAMP(0);
    // the query's term metadata (posting range, idf) is requested before the row is cleared: per term the dependent chain is then
    // posting -> {document length, score} instead of term -> range -> posting -> ... (~2 us per term of a workgroup's 60-135 us)
    constexpr int TPRE = 8;
    int64_t t_b[TPRE], t_e[TPRE];
    double t_idf[TPRE];
#pragma unroll
    for (int u = 0; u < TPRE; ++u) {
        const int j = qb + u;
        const int32_t t = j < qe ? q_terms[j] : -1;
        const bool ok = t >= 0 && t < V;
        t_b[u] = 0;
        t_e[u] = 0;
        if (ok) term_range(t, t_b[u], t_e[u]);
        t_idf[u] = ok ? idf[t] : 0.0;
    }
    // 8 documents per thread and step where the row allows it (64 B of scores, 8 B of marks per thread: the byte-wide mark accesses
    // made the masked rows' last pass 65-72 us against 15-29 us for unmasked ones -- tools/bm25_stamps.py)
    const bool vec8 = ROWS8 || ((lo | hi) & 7) == 0;
    const int64_t p0 = lo >> 1, p1 = hi >> 1;     // the range in pairs of documents (vec8)
    if (vec8) {
        // lane-contiguous 16-byte stores (1 KB per wave instruction; 64 B per lane at a 64 B stride wrote every line in four pieces: 59 us)
        const double2 z2 = make_double2(0.0, 0.0);
        for (int64_t g = p0 + tid; g < p1; g += NT) reinterpret_cast<double2*>(scores)[g] = z2;
        if (masking)
            for (int64_t g = (lo >> 3) + tid; g < (hi >> 3); g += NT) reinterpret_cast<uint64_t*>(mark)[g] = 0ull;
    } else {
#pragma unroll 8
        for (int64_t d = lo + tid; d < hi; d += NT) {
            scores[d] = 0.0;
            if (masking) mark[d] = 0;
        }
    }
    __syncthreads();
    if constexpr (STAMPS) BM25_STAMP(1);
    for (int j = qb; j < qe; ++j) {
        const int32_t t = q_terms[j];
        const double w = q_weights[j];
        if (t >= 0 && t < V) {
            double idf_t;
            int64_t b, e;
            const int u = j - qb;
            if (u < TPRE) {                       // uniform
                idf_t = t_idf[0]; b = t_b[0]; e = t_e[0];
#pragma unroll
                for (int x = 1; x < TPRE; ++x)
                    if (u == x) { idf_t = t_idf[x]; b = t_b[x]; e = t_e[x]; }
            } else {
                idf_t = idf[t];
                term_range(t, b, e);
            }
            // Eight postings per thread in flight: the documents of one term are distinct, but the compiler cannot know that a
            // load of scores[d'] may pass the store to scores[d], so an unrolled loop still ran its read-modify-writes one after
            // the other (~6 us per 1024 x 4 postings); here the gathers of a batch are all issued before the first store.
            constexpr int PU = 8;
            const bool req = w > REQUIRE_MAGIC;
            const double ww = req ? (w - REQUIRE_MAGIC) : w;
            for (int64_t i0 = b + tid; i0 < e; i0 += (int64_t)PU * NT) {
                int32_t dd[PU];
                double tfd[PU];
#pragma unroll
                for (int u2 = 0; u2 < PU; ++u2) {
                    const int64_t i = i0 + (int64_t)u2 * NT;
                    dd[u2] = i < e ? tdoc[i] : -1;
                    tfd[u2] = i < e ? (double)ttf[i] : 0.0;
                }
                if (w < 0.0) {                    // webui.py:154-160 exclude
#pragma unroll
                    for (int u2 = 0; u2 < PU; ++u2)
                        if (dd[u2] >= 0) mark[dd[u2]] |= 0x80;
                } else {                          // :161-170: a required term adds (w - REQUIRE_MAGIC) * score and counts its presence
                    double dlv[PU], sv[PU];
                    uint8_t mk[PU];
#pragma unroll
                    for (int u2 = 0; u2 < PU; ++u2) {
                        dlv[u2] = dd[u2] >= 0 ? (double)dl[dd[u2]] : 0.0;
                        sv[u2] = dd[u2] >= 0 ? scores[dd[u2]] : 0.0;
                        mk[u2] = (req && dd[u2] >= 0) ? mark[dd[u2]] : (uint8_t)0;
                    }
#pragma unroll
                    for (int u2 = 0; u2 < PU; ++u2) {
                        if (dd[u2] < 0) continue;
                        const double sc = bm25_term_score(idf_t, tfd[u2], bm25_length_norm(dlv[u2], avgdl));
                        scores[dd[u2]] = sv[u2] + ww * sc;
                        if (req) mark[dd[u2]] = (uint8_t)(mk[u2] + 1);
                    }
                }
            }
        }
        __syncthreads();
    }
    if constexpr (STAMPS) BM25_STAMP(2);
    double mx = -INFINITY;
    if (masking && vec8) {
        // two documents per lane and access (16 B of scores, 2 B of marks), four accesses in flight; every wave instruction covers a contiguous KB
        for (int64_t g0 = p0 + tid; g0 < p1; g0 += 4 * NT) {
            double2 v[4];
            uint32_t m2[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t g = g0 + u * NT;
                v[u] = g < p1 ? reinterpret_cast<const double2*>(scores)[g] : make_double2(-INFINITY, -INFINITY);
                m2[u] = g < p1 ? reinterpret_cast<const uint16_t*>(mark)[g] : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t g = g0 + u * NT;
                if (g >= p1) continue;
                const uint32_t ma = m2[u] & 0xffu, mb_ = m2[u] >> 8;
                const bool ka = (ma & 0x80u) || (int)(ma & 0x7fu) != n_required, kb = (mb_ & 0x80u) || (int)(mb_ & 0x7fu) != n_required;
                if (ka) v[u].x = -INFINITY;
                if (kb) v[u].y = -INFINITY;
                if (ka || kb) reinterpret_cast<double2*>(scores)[g] = v[u];
                mx = fmax(mx, fmax(v[u].x, v[u].y));
            }
        }
    } else if (masking) {
#pragma unroll 8
        for (int64_t d = lo + tid; d < hi; d += NT) {
            const uint8_t m = mark[d];
            double v = scores[d];
            if ((m & 0x80) || (m & 0x7f) != n_required) scores[d] = v = -INFINITY;
            mx = fmax(mx, v);
        }
    } else if (want_max && vec8) {
#pragma unroll 4
        for (int64_t g = p0 + tid; g < p1; g += NT) {
            const double2 a0 = reinterpret_cast<const double2*>(scores)[g];
            mx = fmax(mx, fmax(a0.x, a0.y));
        }
    } else if (want_max) {
#pragma unroll 8
        for (int64_t d = lo + tid; d < hi; d += NT) mx = fmax(mx, scores[d]);
    }
    if constexpr (STAMPS) BM25_STAMP(3);
    return mx;
}

// One workgroup per query, the whole row; max_out (optional): the row maximum for the normalisation of webui.py:379-380, fused here.
__global__ __launch_bounds__(1024) void bm25_postings_kernel(const int64_t* __restrict__ tptr, const int32_t* __restrict__ tdoc,
                                                             const int32_t* __restrict__ ttf, const int32_t* __restrict__ dl,
                                                             const double* __restrict__ idf, int32_t V, double avgdl, int64_t D,
                                                             const int32_t* __restrict__ q_terms, const double* __restrict__ q_weights,
                                                             const int32_t* __restrict__ q_ptr, double* __restrict__ out,
                                                             uint8_t* __restrict__ mark_all, double* __restrict__ max_out) {
    const int q = blockIdx.x;
    auto term_range = [=](int32_t t, int64_t& b, int64_t& e) {
        b = tptr[t];
        e = tptr[t + 1];
    };
    const double mx = bm25_postings_walk<1024, false, true>(q, 0, D, term_range, tdoc, ttf, dl, idf, V, avgdl, D, q_terms, q_weights, q_ptr,
                                                            out, mark_all, max_out != nullptr);
    if (max_out) {
        const double m = block_max<1024>(mx);
        if (threadIdx.x == 0) max_out[q] = m;
    }
}

// The same walk with the document range cut into slices (round 4).  One workgroup per query is one workgroup per CU for a batch of 256:
// 16 waves that clear, scatter into and re-read an 800 KB row at ~15 GB/s -- the kernel took 166 us for 620 MB, most of it latency.  A
// document's float64 additions only have to keep the QUERY'S TERM ORDER, and documents are independent, so a workgroup may take any
// document range: grid (query, part), each workgroup the postings of its range -- found through a table of every term's posting offsets
// at BM25_SLICES fixed document boundaries, built with the index -- and a partial row maximum; four 512-thread workgroups share a CU.
constexpr int BM25_SLICES = 8;
__global__ __launch_bounds__(512) void bm25_postings_sliced_kernel(const int64_t* __restrict__ tslice, const int32_t* __restrict__ tdoc,
                                                                   const int32_t* __restrict__ ttf, const int32_t* __restrict__ dl,
                                                                   const double* __restrict__ idf, int32_t V, double avgdl, int64_t D, int64_t slice_docs,
                                                                   int per_part, const int32_t* __restrict__ q_terms,
                                                                   const double* __restrict__ q_weights, const int32_t* __restrict__ q_ptr,
                                                                   double* __restrict__ out, uint8_t* __restrict__ mark_all, double* __restrict__ max_part) {
    const int q = blockIdx.x, part = blockIdx.y;
    const int s0 = part * per_part, s1 = s0 + per_part;                       // fixed slices [s0, s1)
    const int64_t lo = (int64_t)s0 * slice_docs, hi = s1 == BM25_SLICES ? D : (int64_t)s1 * slice_docs;      // lo, hi multiples of 8 (D % 8 == 0)
    auto term_range = [=](int32_t t, int64_t& b, int64_t& e) {
        b = tslice[(int64_t)t * (BM25_SLICES + 1) + s0];
        e = tslice[(int64_t)t * (BM25_SLICES + 1) + s1];
    };
    const double mx = bm25_postings_walk<512, true, false>(q, lo, hi, term_range, tdoc, ttf, dl, idf, V, avgdl, D, q_terms, q_weights, q_ptr,
                                                           out, mark_all, max_part != nullptr);
    if (max_part) {
        const double m = block_max<512>(mx);
        if (threadIdx.x == 0) max_part[(int64_t)q * gridDim.y + part] = m;
    }
}
__global__ void bm25_max_reduce_kernel(const double* __restrict__ parts, int nparts, double* __restrict__ max_out, int nq) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    double m = parts[(int64_t)q * nparts];
    for (int p = 1; p < nparts; ++p) m = fmax(m, parts[(int64_t)q * nparts + p]);
    max_out[q] = m;
}

// ---------------------------------------------------------------------------------------------
// row maxima (numpy .max(): NaN-free inputs assumed)
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(1024) void rowmax_kernel(const T* __restrict__ v, int64_t n, T* __restrict__ out) {
    const T* row = v + (int64_t)blockIdx.x * n;
    T m = -INFINITY;
    for (int64_t i = threadIdx.x; i < n; i += 1024) m = fmax(m, row[i]);
    m = block_max<1024>(m);
    if (threadIdx.x == 0) out[blockIdx.x] = m;
}

__global__ __launch_bounds__(256) void combine_kernel(const double* __restrict__ a, const float* __restrict__ b, int64_t n,
                                                      double wa, float wb, const double* __restrict__ max_a,
                                                      const float* __restrict__ max_b, const uint32_t* __restrict__ max_b_keys,
                                                      double* __restrict__ out) {
    const int q = blockIdx.y;
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= n) return;
    const double ma = max_a ? max_a[q] : 0.0;
    const float mb = max_b ? max_b[q] : (max_b_keys ? float_from_key(max_b_keys[q]) : 0.0f);
    out[(int64_t)q * n + d] = combine_score(a[(int64_t)q * n + d], b[(int64_t)q * n + d], ma, mb, wa, wb);
}

// =============================================================================================
// Dense similarity: scores[q][d] = chain_k fma(row[d][k], query[q][k], acc)
// v_mfma_f32_32x32x2_f32: A = 32 queries x 2 k, B = 2 k x 32 documents, D[query][document].
// Per wave: a 32-document tile, the whole K; up to 32 queries per pass for the price of one
// (the kernel is HBM-bound: 32 x 1200 B per 150 MFMAs per wave).
// =============================================================================================
typedef float f32x16 __attribute__((ext_vector_type(16)));


// TILED: `index` is the tile-major copy of the rows, float4 tl[((T * K/4 + kq) * 32 + c)] = row[32 T + c][4 kq .. 4 kq + 3]:
// the 32 lanes of a half-wave read 512 contiguous bytes per load.  With the plain row-major matrix every lane
// walks its own 1200 B row -- 32 different cache lines per load instruction, each revisited four times -- and the
// kernel ran at 2 TB/s of algorithmic traffic (61 us per pass over 100k x 300); K % 4 != 0 keeps that path.
template <bool TILED>
__global__ __launch_bounds__(SIM_THREADS) void sim_mfma_kernel(const float* __restrict__ index, int64_t D, int K, int64_t ld,
                                                       const float* __restrict__ q, int nq, float* __restrict__ out,
                                                       int64_t out_ld) {
    extern __shared__ __attribute__((aligned(16))) float qT[];   // [K][32]: qT[k*32 + j] = q[j][k]
    const int tid = threadIdx.x;
    for (int i = tid; i < K * 32; i += SIM_THREADS) {
        const int k = i >> 5, j = i & 31;
        qT[i] = j < nq ? q[(int64_t)j * K + k] : 0.0f;
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t ntiles = (D + 31) / 32;
    for (int64_t tile = (int64_t)blockIdx.x * (SIM_THREADS / 64) + wave; tile < ntiles; tile += (int64_t)gridDim.x * (SIM_THREADS / 64)) {
        int64_t doc = tile * 32 + r;
        const int64_t docc = doc < D ? doc : D - 1;
        const float* __restrict__ row = index + docc * ld;
        const float4* __restrict__ trow = reinterpret_cast<const float4*>(index) + tile * (K >> 2) * 32 + r;    // TILED
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
        int k = 0;
#pragma unroll 2
        for (; k + 8 <= K; k += 8) {
            const float4 v0 = TILED ? trow[(k >> 2) * 32] : *reinterpret_cast<const float4*>(row + k);
            const float4 v1 = TILED ? trow[((k >> 2) + 1) * 32] : *reinterpret_cast<const float4*>(row + k + 4);
            const float b0 = h ? v0.y : v0.x, b1 = h ? v0.w : v0.z, b2 = h ? v1.y : v1.x, b3 = h ? v1.w : v1.z;
            const float* qk = qT + (k + h) * 32 + r;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qk[0], b0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qk[64], b1, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qk[128], b2, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qk[192], b3, acc, 0, 0, 0);
        }
        for (; k + 2 <= K; k += 2) {   // K % 8 tail (K is even, checked on the host)
            float b0;
            if (TILED) {
                const float4 t4 = trow[(k >> 2) * 32];
                const int e = (k & 3) + h;                      // k is even here: e in {0,1} or {2,3}
                b0 = e == 0 ? t4.x : (e == 1 ? t4.y : (e == 2 ? t4.z : t4.w));
            } else {
                b0 = row[k + h];
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qT[(k + h) * 32 + r], b0, acc, 0, 0, 0);
        }
        // D layout: column = lane & 31 = document, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5) = query
        if (doc < D) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int qi = (reg & 3) + 8 * (reg >> 2) + 4 * h;
                if (qi < nq) out[(int64_t)qi * out_ld + doc] = acc[reg];
            }
        }
    }
}

// Up to 256 queries per pass over the index (round 3).  The kernel above streams the whole index once per 32 queries -- 8 passes of
// 120 MB for the bench's 256-query batch, HBM-bound at 41 us each -- although a 32-document tile already in registers can be multiplied
// against every query block for the price of the (exact-f32) MFMAs alone.  Here a workgroup of 8 waves takes 8 document tiles and walks K
// in chunks of 8: the chunk of the query matrix ([8 k][256 queries], 9 KB) is staged in LDS by all threads (double-buffered, one barrier
// per chunk), each wave multiplies its documents' 8 k-values against NQB query blocks (4 NQB MFMAs) and keeps NQB accumulator tiles.
// Per (query, document) the MFMA sequence -- operands and order -- is the one of the kernel above: the same bits.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {      // v of the lane the DPP control names (all rows and banks enabled)
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false);
}
constexpr int SIMW_QS = 288;       // floats per k-row of the LDS chunk: 256 queries + 32, so that the two half-waves (k, k + 1) use different banks
template <int NQB>
__global__ __launch_bounds__(512) void sim_mfma_wide_kernel(const float4* __restrict__ tiled, int64_t D, int K, const float* __restrict__ q, int nq,
                                                            float* __restrict__ out, int64_t out_ld, float* __restrict__ part_max) {
    // part_max (round 4, optional): [gridDim.x][256] -- this workgroup's maximum of every query's products, taken from the accumulators
    // (the row maximum webui.py:377-380 divides by; a second pass over the 100 MB of stored products took 24 us per 256 queries).  The
    // consumer takes the maximum over the workgroups: max is exact, so the value is rowmax_kernel's bit for bit.
    __shared__ float qs[2][8][SIMW_QS];
    __shared__ uint32_t wmax[256];               // float_order_key images; 0 = nothing seen
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 256) wmax[tid] = 0u;               // (published by the first barrier of the first walk)
    const int r = lane & 31, h = lane >> 5;
    const int64_t ntiles = (D + 31) / 32;
    const int KQ = K >> 2;                       // float4 per document row
    const int nchunks = (KQ + 1) >> 1;           // 8 k per chunk; the last one holds 4 when K % 8 == 4
    const int sj = tid >> 1, sh = tid & 1;       // staging role: query sj, k-half sh of the chunk
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto load_q = [&](int c) {
        const int kq = 2 * c + sh;
        return (sj < nq && kq < KQ) ? *reinterpret_cast<const float4*>(q + (int64_t)sj * K + 4 * kq) : zero4;
    };
    auto store_q = [&](int buf, float4 v) {
        qs[buf][4 * sh + 0][sj] = v.x;
        qs[buf][4 * sh + 1][sj] = v.y;
        qs[buf][4 * sh + 2][sj] = v.z;
        qs[buf][4 * sh + 3][sj] = v.w;
    };
    // One walk over K for this wave: document tile `tile` (tv: the wave has one) against NB query blocks starting at block qb0.
    auto walk = [&](auto nb_c, int64_t tile, bool tv, int qb0) __attribute__((always_inline)) {
        constexpr int NB = decltype(nb_c)::value;
        const float4* __restrict__ trow = tiled + (tv ? tile : ntiles - 1) * KQ * 32 + r;
        f32x16 acc[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[b][i] = 0.0f;
        float4 d0 = trow[0], d1 = 1 < KQ ? trow[32] : zero4;
        store_q(0, load_q(0));                   // buffer 0 was last read before the final barrier of the previous walk
        __syncthreads();
        const int nfull = KQ >> 1;               // chunks of 8 k; K % 8 == 4 leaves a chunk of 4 behind them
        for (int c = 0; c < nfull; ++c) {
            const bool more = c + 1 < nchunks;
            float4 qn = zero4, e0 = zero4, e1 = zero4;
            if (more) {                          // the next chunk's loads are in flight under this chunk's MFMAs
                qn = load_q(c + 1);
                e0 = trow[(2 * c + 2) * 32];
                e1 = 2 * c + 3 < KQ ? trow[(2 * c + 3) * 32] : zero4;
            }
            const float b0 = h ? d0.y : d0.x, b1 = h ? d0.w : d0.z, b2 = h ? d1.y : d1.x, b3 = h ? d1.w : d1.z;
            const float* qrow = &qs[c & 1][h][qb0 * 32 + r];
            // k-pair by k-pair across the blocks: consecutive MFMAs are independent (per block the k order is unchanged)
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow[b * 32], b0, acc[b], 0, 0, 0);
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow[b * 32 + 2 * SIMW_QS], b1, acc[b], 0, 0, 0);
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow[b * 32 + 4 * SIMW_QS], b2, acc[b], 0, 0, 0);
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow[b * 32 + 6 * SIMW_QS], b3, acc[b], 0, 0, 0);
            if (more) {
                store_q((c + 1) & 1, qn);
                d0 = e0;
                d1 = e1;
            }
            __syncthreads();
        }
        if (KQ & 1) {                            // the chunk of 4 (staged by the last iteration above, or by the prologue when K == 4)
            const float b0 = h ? d0.y : d0.x, b1 = h ? d0.w : d0.z;
            const float* qrow = &qs[nfull & 1][h][qb0 * 32 + r];
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const float* qk = qrow + b * 32;
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(qk[0], b0, acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(qk[2 * SIMW_QS], b1, acc[b], 0, 0, 0);
            }
            __syncthreads();                     // the next walk's prologue writes buffer 0 again
        }
        const int64_t doc = tile * 32 + r;
        if (tv && doc < D) {
            // D layout: column = lane & 31 = document, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) = query of the block.  One per-lane
            // pointer, the row offsets as scalar products of a stride the compiler may not hoist (left to itself it keeps 16 NQB 64-bit
            // offsets and as many lane masks alive across the whole tile loop: 256 VGPRs and 190 spilled for NQB = 8)
            int64_t old = out_ld;
            int nqv = nq;
            asm volatile("" : "+s"(old), "+s"(nqv));
            float* __restrict__ base = out + (int64_t)(qb0 * 32 + 4 * h) * old + doc;
            const int nleft = nqv - qb0 * 32;    // queries from this wave's first block on
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                if (b * 32 + 32 <= nleft) {                     // uniform: a whole block of queries, no per-lane test
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) base[(int64_t)(b * 32 + (reg & 3) + 8 * (reg >> 2)) * old] = acc[b][reg];
                } else if (b * 32 < nleft) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int cqi = b * 32 + (reg & 3) + 8 * (reg >> 2);
                        if (cqi + 4 * h < nleft) base[(int64_t)cqi * old] = acc[b][reg];
                    }
                }
            }
        }
        if (part_max) {                          // uniform
            // Row maxima out of the accumulators (stored above, so the registers are free): the 32 documents of a half-wave share the
            // query.  Per value five DPP steps on the ORDER KEY -- unsigned max fuses with the DPP move into one v_max_u32_dpp: within
            // the quad, the half row, the row of 16, then row_bcast15 hands row 0's result to row 1 (rows 1 and 3 enabled) -- and no LDS
            // instruction at all; lanes 16 and 48 then hold the half-waves' maxima and add them to the workgroup's table with LDS
            // atomics issued back to back under ONE branch.  (Measured against the 24.6 us of the second pass this replaces: five
            // __shfl_xor per value +53 us on the kernel, float DPP steps + a swizzle +31 us, key DPP steps + a swizzle +27 us -- every
            // swizzle / shuffle is an LDS round trip the next value's waits for.)
            const bool live = tv && doc < D;     // padding documents of the last tile and idle waves do not take part
#pragma unroll
            for (int b = 0; b < NB; ++b) {       // sixteen values at a time: 128 keys beside the accumulators spilled
                uint32_t kv[16];
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    uint32_t k = live ? float_order_key(acc[b][reg]) : 0u;
                    k = max(k, dpp_u32<0xB1>(k));       // quad_perm [1, 0, 3, 2]
                    k = max(k, dpp_u32<0x4E>(k));       // quad_perm [2, 3, 0, 1]
                    k = max(k, dpp_u32<0x141>(k));      // row_half_mirror
                    k = max(k, dpp_u32<0x140>(k));      // row_mirror
                    k = max(k, (uint32_t)__builtin_amdgcn_update_dpp((int)k, (int)k, 0x142, 0xA, 0xF, false));      // row_bcast15 into rows 1 and 3
                    kv[reg] = k;
                }
                if (r == 16) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) atomicMax(&wmax[(qb0 + b) * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h], kv[reg]);
                }
            }
        }
    };
    // Full rounds: every wave of every workgroup one tile against all NQB blocks.  What is left over (fewer tiles than wave slots) may be
    // split f ways across the query blocks (f waves per tile, NQB / f blocks each) when that shortens the tail.  A walk costs about
    // a + b NB with a = 2.5 b (measured at 100 k x 300, 256 queries: 114 us for NB = 8, 38 us for NB = 1 -- the per-chunk load -> LDS ->
    // barrier chain does not shrink with the MFMAs), so the split pays for small indices that would leave most workgroups without a tile
    // (32 tiles: one walk of 1 block on 32 workgroups instead of 8 blocks on 4), not for 3125 tiles on 2048 slots (measured: 302 us with
    // f = 8 against 228 us unsplit).
    const int64_t G = gridDim.x, slots = 8 * G;
    const int64_t full_rounds = ntiles / slots;
    for (int64_t rd = 0; rd < full_rounds; ++rd) walk(std::integral_constant<int, NQB>{}, (rd * G + blockIdx.x) * 8 + wave, true, 0);
    const int64_t base_tile = full_rounds * slots, rem = ntiles - base_tile;
    if (rem > 0) {
        int f = 1;
        int64_t best = (rem + slots - 1) / slots * (5 + 2 * NQB);        // walks x (a + b NB), a : b = 5 : 2
        for (int c = 2; c <= NQB; c *= 2) {
            const int64_t len = (rem * c + slots - 1) / slots * (5 + 2 * (NQB / c));
            if (len < best) {
                best = len;
                f = c;
            }
        }
        const int64_t jobs = rem * f, walks = (jobs + slots - 1) / slots;
        for (int64_t w = 0; w < walks; ++w) {
            const int64_t J = (w * G + blockIdx.x) * 8 + wave;
            const bool tv = J < jobs;
            const int64_t tile = base_tile + (tv ? J / f : 0);
            const int grp = (int)(J % f);
            if (f == 1) walk(std::integral_constant<int, NQB>{}, tile, tv, 0);
            if constexpr (NQB >= 2) { if (f == 2) walk(std::integral_constant<int, NQB / 2>{}, tile, tv, grp * (NQB / 2)); }
            if constexpr (NQB >= 4) { if (f == 4) walk(std::integral_constant<int, NQB / 4>{}, tile, tv, grp * (NQB / 4)); }
            if constexpr (NQB >= 8) { if (f == 8) walk(std::integral_constant<int, NQB / 8>{}, tile, tv, grp * (NQB / 8)); }
        }
    }
    if (part_max) {
        __syncthreads();
        if (tid < 256) part_max[(int64_t)blockIdx.x * 256 + tid] = wmax[tid] ? float_from_key(wmax[tid]) : -INFINITY;
    }
}

// (re)build tiles [t0, t1) of the tile-major copy from the row-major rows; rows >= len read as zero
__global__ __launch_bounds__(256) void retile_kernel(const float* __restrict__ rows, float4* __restrict__ tl, int64_t len, int K,
                                                     int64_t t0, int64_t t1) {
    const int KQ = K >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (t1 - t0) * KQ * 32;
    if (idx >= total) return;
    const int c = (int)(idx & 31);
    const int kq = (int)((idx >> 5) % KQ);
    const int64_t T = t0 + (idx >> 5) / KQ;
    const int64_t doc = T * 32 + c;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (doc < len) v = *reinterpret_cast<const float4*>(rows + doc * K + 4 * kq);
    tl[(T * KQ + kq) * 32 + c] = v;
}

// =============================================================================================
// One query at a time -- the reference's real call (webui.py:586: find_similar_documents(query, topn=800)).
// The batched kernels above give one workgroup to a query for BM25, the row maxima and the top-k: at nq = 1 that is
// one CU of 256 busy for ~120 of the ~170 us a query took.  Here every step runs over the whole chip, thread per
// document, and the query itself travels in the kernel arguments (no staging copy):
//   search1_score    BM25 in the reference's own shape (webui.py:139-170: for each query term a pass over the documents,
//                    here the document's own (term, tf) list, document-major CSR) + the index product as the k-ordered
//                    fmaf chain (bit-equal to the exact-f32 MFMA chain of sim_mfma_kernel and to the oracle) from the
//                    tile-major copy; per-workgroup maxima into 256 slots
//   search1_combine  webui.py:377-383 with the global maxima; the maximum of every group of 64 * gw documents
//   search1_collect  threshold digit = digit of the k-th largest group maximum; candidates (score digit >= threshold) into
//                    the workgroup's own slots
//   topk_kernel      gathers the candidates and ranks them (by counting when few, bitonic sort otherwise); fills up with -inf
//                    ties when a required / excluded term left fewer than k finite scores; if the candidates overflow their
//                    buffers the exact radix select runs instead -- same kernel, same results
// No global atomics on shared addresses after the score kernel: same-address atomics serialise at ~50-60 ns each on this part
// (measured: 1563 histogram adds over ~100 bins cost 5 us, ~100 adds on one counter 6 us).
// Algorithmic bytes per query: D * dim * 4 (index) + nnz * 8 + D * 12 (CSR) + D * (8 + 4) * 2 + D * 8 * 2 (scores, final).
// =============================================================================================
constexpr int S1_MAX_TERMS = 16;
constexpr int S1_SLOTS = 256;
constexpr int S1_LDS_TERMS = 6144;   // term ids of one workgroup's 128 documents staged in LDS (48 per document)

struct Search1Query {            // passed by value: 3.3 KB of the 4 KB kernel-argument segment
    int32_t nt, dim;
    int32_t terms[S1_MAX_TERMS];
    double weights[S1_MAX_TERMS];
    float q[S1_MAX_DIM];
};

struct Search1State {            // device resident; the maxima slots are all zero between queries (the last kernel clears them)
    unsigned long long max_a[S1_SLOTS];      // order_key images of the per-workgroup BM25 maxima
    uint32_t max_b[S1_SLOTS];                // float_order_key images of the index-product maxima
    uint32_t dbg[4];                         // NOT cleared: {candidates, took the candidate path, 0, 0} of the last query (hiptsdbg_search1_last)
};

struct Search1Witness {          // 32 B per wave of search1_score_kernel (64 documents)
    double bm_a;                 // the wave's largest BM25 score ...
    float sim_a, pad0;           // ... and that document's index product
    double bm_b;                 // the BM25 score of the document with ...
    float sim_b, pad1;           // ... the wave's largest index product
};

// PIPE (round 5, the default; HIPTS_S1_PIPE=0 runs the sequential form): the BM25 part is a chain of dependent round trips -- the span's
// bounds, its term ids (up to 12 passes of four loads -> LDS, each a round trip of its own), the matches' tf, the idf values -- about 12 of
// the kernel's 32 us during which only ONE round of the index stream was in flight.  Here the rounds of the stream are dealt between the
// chain's steps (two rounds in flight throughout, every consume waits only for loads older than the chain's), the term ids are requested 16
// per lane at once, and the idf values go through LDS, requested with the first round.  Same operations per document in the same order.
template <bool PIPE>
__global__ __launch_bounds__(S1_THREADS) void search1_score_kernel(const Search1Query Q, const float4* __restrict__ tiled, int64_t D,
                                                                   const int64_t* __restrict__ ptr, const int32_t* __restrict__ term,
                                                                   const int32_t* __restrict__ tf, const int32_t* __restrict__ dl,
                                                                   const double* __restrict__ idf, int32_t V, double avgdl,
                                                                   double* __restrict__ bm_out, float* __restrict__ sim_out,
                                                                   Search1State* __restrict__ st, Search1Witness* __restrict__ wit) {
    __shared__ int32_t sterm[S1_LDS_TERMS];
    __shared__ int sptr[S1_THREADS + 1];
    __shared__ int32_t stf[S1_MAX_TERMS][S1_THREADS];          // tf of query term j in this thread's document (0 = absent)
    const int tid = threadIdx.x;
    const int64_t d = (int64_t)blockIdx.x * S1_THREADS + tid;
    const bool valid = d < D;
    const int64_t dd = valid ? d : D - 1;
    // ---- index product: acc = fmaf(row[k], q[k], acc), k ascending (the order of sim_mfma_kernel's chain and of the oracle).
    // The kernel is a stream of D * dim * 4 bytes: two register buffers of U float4 per lane, the loads of round r + 1 are issued
    // before round r is consumed, and the first round is requested before the BM25 part below so that it flies meanwhile.
    // Rounds past the last k re-read the last float4 (a cache hit) against Q.q's zero padding: fmaf(x, +0, acc) = acc exactly.
    // (Measured: U = 8 or 16 and 128- or 256-thread workgroups make no difference; 64-thread workgroups are 40 % slower.)
    const int KQ = Q.dim >> 2;
    const float4* __restrict__ p = tiled + ((dd >> 5) * KQ) * 32 + (dd & 31);
    constexpr int U = 8;
    static_assert(S1_MAX_DIM % (4 * U) == 0, "Q.q must cover whole rounds");
    float4 va[U], vb[U], vc[U];      // (vc: the PIPE form keeps THREE rounds in flight -- the chain's LDS phases are longer than a round)
    auto request = [&](float4(&v)[U], int kq0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kq = kq0 + u < KQ ? kq0 + u : KQ - 1;
            v[u] = p[(int64_t)kq * 32];
        }
    };
    float acc = 0.0f;
    auto consume = [&](const float4(&v)[U], int kq0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float* qq = Q.q + 4 * (kq0 + u);
            acc = fmaf(v[u].x, qq[0], acc);
            acc = fmaf(v[u].y, qq[1], acc);
            acc = fmaf(v[u].z, qq[2], acc);
            acc = fmaf(v[u].w, qq[3], acc);
        }
    };
    const int rounds = (KQ + U - 1) / U;
    // one step of the stream: round r is consumed, round r + 2 requested into its buffer (past the end: a clamped re-read nobody consumes)
    constexpr int AHEAD = PIPE ? 3 : 2;
    auto step_a = [&](int r) {
        if (r < rounds) {
            consume(va, r * U);
            request(va, (r + AHEAD) * U);
        }
    };
    auto step_b = [&](int r) {
        if (r < rounds) {
            consume(vb, r * U);
            request(vb, (r + AHEAD) * U);
        }
    };
    auto step_c = [&](int r) {
        if (r < rounds) {
            consume(vc, r * U);
            request(vc, (r + AHEAD) * U);
        }
    };
    request(va, 0);
    // ---- BM25 (webui.py:139-170), the arithmetic of bm25_score_kernel.  The (term, tf) lists of a workgroup's documents are one
    // contiguous span of the document-major CSR: its term ids are staged in LDS with coalesced loads, then walked ONCE, coalesced:
    // a lane compares its entry with the (scalar) query terms; on a match -- at most nt per document -- it finds the entry's
    // document by bisection of the 128 start offsets and records the entry's tf in the slot of (query term, document).
    // (Also measured without gain: the BM25 part on two waves of its own beside two index-stream waves (32.7 us); the tf staged
    // with the term id so that a match needs no global load (35.5 us).  The index stream alone runs at 6 TB/s -- sim1_kernel back to
    // back, 20 us for these 120 MB -- so ~12 us of this kernel are the BM25 part's dependent chain, not bandwidth.)
    // (Measured alternatives, all within 2 us of each other at ~33 us for the kernel: every thread walking its own list from memory
    // or from LDS; a staged entry -> document map with 16-bit LDS stores was slower, 50 us.)
    const int64_t d_first = (int64_t)blockIdx.x * S1_THREADS;
    const int64_t d_last = d_first + S1_THREADS < D ? d_first + S1_THREADS : D;
    const int64_t b0 = ptr[d_first], e0 = ptr[d_last];
    const bool staged = e0 - b0 <= S1_LDS_TERMS;
    const int nspan = staged ? (int)(e0 - b0) : 0;
    __shared__ double sidf[S1_MAX_TERMS];
    const int64_t b = ptr[dd], e = ptr[dd + 1];
    const double dlv = (double)dl[dd];
    double s = 0.0;
    bool masked = false;
    if constexpr (PIPE) {
        double idf_mine = 0.0;
        if (tid < Q.nt) {
            const int32_t t = Q.terms[tid];
            idf_mine = (t >= 0 && t < V) ? idf[t] : 0.0;
        }
        request(vb, U);
        request(vc, 2 * U);
        __builtin_amdgcn_sched_barrier(0);
        step_a(0);
        // the span's term ids, 16 per lane in flight (2048 ids per pass: most spans in one)
        constexpr int TU = 16;
        int32_t t16[TU];
        auto req_terms = [&](int i0) {
#pragma unroll
            for (int u = 0; u < TU; ++u) {
                const int i = i0 + u * S1_THREADS + tid;
                t16[u] = i < nspan ? term[b0 + i] : 0;
            }
        };
        auto put_terms = [&](int i0) {
#pragma unroll
            for (int u = 0; u < TU; ++u) {
                const int i = i0 + u * S1_THREADS + tid;
                if (i < nspan) sterm[i] = t16[u];
            }
        };
        if (nspan > 0) req_terms(0);
        __builtin_amdgcn_sched_barrier(0);
        step_b(1);
        __builtin_amdgcn_sched_barrier(0);
        if (nspan > 0) put_terms(0);
        for (int i0 = TU * S1_THREADS; i0 < nspan; i0 += TU * S1_THREADS) {
            req_terms(i0);
            put_terms(i0);
        }
        for (int j = 0; j < Q.nt; ++j) stf[j][tid] = 0;
        sptr[tid] = valid ? (int)(b - b0) : (int)(e0 - b0);
        if (tid == 0) sptr[S1_THREADS] = (int)(e0 - b0);
        if (tid < Q.nt) sidf[tid] = idf_mine;
        __syncthreads();
        step_c(2);
        __builtin_amdgcn_sched_barrier(0);
        if (staged) {
            for (int i = tid; i < nspan; i += S1_THREADS) {
                const int32_t ti = sterm[i];
                for (int j = 0; j < Q.nt; ++j)
                    if (ti == Q.terms[j]) {
                        int lo = 0, hi = S1_THREADS;
                        while (hi - lo > 1) {
                            const int mid = (lo + hi) >> 1;
                            if (sptr[mid] <= i) lo = mid;
                            else hi = mid;
                        }
                        stf[j][lo] = tf[b0 + i];
                    }
            }
            __syncthreads();
        } else {
            for (int64_t i = b; i < e; ++i) {
                const int32_t ti = term[i];
                for (int j = 0; j < Q.nt; ++j)
                    if (ti == Q.terms[j]) stf[j][tid] = tf[i];
            }
        }
        step_a(3);
        __builtin_amdgcn_sched_barrier(0);
        const double nrm = bm25_length_norm(dlv, avgdl);
        for (int j = 0; j < Q.nt; ++j) {
            const double w = Q.weights[j];
            const int32_t tfv = stf[j][tid];
            const double idf_t = sidf[j];
            bm25_accumulate(w, tfv, bm25_term_score(idf_t, (double)tfv, nrm), s, masked);
        }
        if (masked) s = -INFINITY;
        // ---- the rest of the index stream
        step_b(4);
        step_c(5);
        for (int r = 6; r < rounds; r += 3) {
            step_a(r);
            step_b(r + 1);
            step_c(r + 2);
        }
    } else {
    for (int i0 = 0; i0 < nspan; i0 += 4 * S1_THREADS) {
        int32_t t4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * S1_THREADS + tid;
            t4[u] = i < nspan ? term[b0 + i] : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * S1_THREADS + tid;
            if (i < nspan) sterm[i] = t4[u];
        }
    }
    for (int j = 0; j < Q.nt; ++j) stf[j][tid] = 0;
    sptr[tid] = valid ? (int)(b - b0) : (int)(e0 - b0);         // where this thread's document starts inside the staged span (threads past D: nowhere)
    if (tid == 0) sptr[S1_THREADS] = (int)(e0 - b0);
    __syncthreads();
    if (staged) {
        for (int i = tid; i < nspan; i += S1_THREADS) {
            const int32_t ti = sterm[i];
            for (int j = 0; j < Q.nt; ++j)
                if (ti == Q.terms[j]) {
                    int lo = 0, hi = S1_THREADS;            // largest lo with sptr[lo] <= i (an empty document shares its start with the next)
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (sptr[mid] <= i) lo = mid;
                        else hi = mid;
                    }
                    stf[j][lo] = tf[b0 + i];
                }
        }
        __syncthreads();
    } else {        // a span too long for LDS (documents with hundreds of tags): every thread walks its own list in memory
        for (int64_t i = b; i < e; ++i) {
            const int32_t ti = term[i];
            for (int j = 0; j < Q.nt; ++j)
                if (ti == Q.terms[j]) stf[j][tid] = tf[i];
        }
    }
    const double nrm = bm25_length_norm(dlv, avgdl);
    for (int j = 0; j < Q.nt; ++j) {
        const int32_t t = Q.terms[j];
        const double w = Q.weights[j];
        const int32_t tfv = stf[j][tid];
        const double idf_t = (t >= 0 && t < V) ? idf[t] : 0.0;
        bm25_accumulate(w, tfv, bm25_term_score(idf_t, (double)tfv, nrm), s, masked);
    }
    if (masked) s = -INFINITY;
    // ---- the index stream
    int r = 0;
    for (; r + 2 <= rounds; r += 2) {
        request(vb, (r + 1) * U);
        consume(va, r * U);
        request(va, (r + 2) * U);               // past the end: a clamped re-read that nobody consumes
        consume(vb, (r + 1) * U);
    }
    if (r < rounds) consume(va, r * U);
    }
    if (valid) {
        bm_out[d] = s;
        sim_out[d] = acc;
    }
    // ---- per-workgroup maxima -> one of 256 slots (atomicMax on order-preserving images; 0 is below every value): ~3 adds per slot
    double ma = valid ? s : -INFINITY;
    float mb = valid ? acc : -INFINITY;
    const double s_own = ma;
    const float acc_own = mb;
    for (int o = 32; o >= 1; o >>= 1) {
        ma = fmax(ma, __shfl_xor(ma, o));
        mb = fmaxf(mb, __shfl_xor(mb, o));
    }
    if (wit) {
        // Two WITNESS documents per wave for search1_finish_kernel's threshold: the one with the wave's largest BM25 score and the one with
        // its largest index product, each with BOTH of its scores.  Whatever the global maxima turn out to be, the combined score of a real
        // document is a lower bound of its wave's best combined score -- and the wave's best is, in practice, one of these two.
        const unsigned long long ba = __ballot(s_own == ma), bb = __ballot(acc_own == mb);
        const int la = ba ? __ffsll(ba) - 1 : 0, lb = bb ? __ffsll(bb) - 1 : 0;      // (an all-NaN wave: any lane; its witness then scores NaN = digit 0)
        const float sim_at_a = __shfl(acc_own, la);
        const double bm_at_b = __shfl(s_own, lb);
        if ((tid & 63) == 0) {
            Search1Witness w;
            w.bm_a = ma; w.sim_a = sim_at_a; w.bm_b = bm_at_b; w.sim_b = mb; w.pad0 = 0.f; w.pad1 = 0.f;
            wit[d >> 6] = w;                        // d of lane 0 = the wave's first document (D rounded up to whole waves is allocated)
        }
    }
    __shared__ double pa[S1_THREADS / 64];
    __shared__ float pb[S1_THREADS / 64];
    if ((tid & 63) == 0) {
        pa[tid >> 6] = ma;
        pb[tid >> 6] = mb;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < S1_THREADS / 64; ++w) {
            ma = fmax(ma, pa[w]);
            mb = fmaxf(mb, pb[w]);
        }
        atomicMax(&st->max_a[blockIdx.x % S1_SLOTS], (unsigned long long)order_key(ma));
        atomicMax(&st->max_b[blockIdx.x % S1_SLOTS], float_order_key(mb));
    }
}

__device__ __forceinline__ void search1_maxima(const Search1State* __restrict__ st, double* ma, float* mb) {
    // every wave folds the slots itself (3 KB from L2)
    const int lane = threadIdx.x & 63;
    unsigned long long ka = 0;
    uint32_t kb = 0;
#pragma unroll
    for (int i = 0; i < S1_SLOTS / 64; ++i) {
        const unsigned long long a = st->max_a[i * 64 + lane];
        const uint32_t b = st->max_b[i * 64 + lane];
        ka = a > ka ? a : ka;
        kb = b > kb ? b : kb;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long oa = __shfl_xor(ka, o);
        const uint32_t ob = __shfl_xor(kb, o);
        ka = oa > ka ? oa : ka;
        kb = ob > kb ? ob : kb;
    }
    *ma = ka ? key_value(ka) : -INFINITY;
    *mb = kb ? float_from_key(kb) : -INFINITY;
}


// index[query] for ONE query (webui.py:205: the rerank product; webui.py:306-309 restated: the character-feature differences):
// the index-stream half of search1_score_kernel alone -- thread per document, k-ordered fmaf chain from the tile-major copy,
// the query in the kernel arguments.  Same bits as sim_mfma_kernel's chain; one pass costs the same bytes but no LDS query
// tile, no 32-wide MFMA for one useful column: 100k x 768 in ~60 us instead of ~270 us per call.
struct Sim1Query {
    int32_t dim, pad[3];
    float q[S1_MAX_DIM];
};

__global__ __launch_bounds__(128) void sim1_kernel(const Sim1Query Q, const float4* __restrict__ tiled, int64_t D, float* __restrict__ out) {
    const int64_t d = (int64_t)blockIdx.x * 128 + threadIdx.x;
    const int64_t dd = d < D ? d : D - 1;
    const int KQ = Q.dim >> 2;
    const float4* __restrict__ p = tiled + ((dd >> 5) * KQ) * 32 + (dd & 31);
    constexpr int U = 8;
    float4 va[U], vb[U];
    auto request = [&](float4(&v)[U], int kq0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kq = kq0 + u < KQ ? kq0 + u : KQ - 1;
            v[u] = p[(int64_t)kq * 32];
        }
    };
    float acc = 0.0f;
    auto consume = [&](const float4(&v)[U], int kq0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float* qq = Q.q + 4 * (kq0 + u);
            acc = fmaf(v[u].x, qq[0], acc);
            acc = fmaf(v[u].y, qq[1], acc);
            acc = fmaf(v[u].z, qq[2], acc);
            acc = fmaf(v[u].w, qq[3], acc);
        }
    };
    request(va, 0);
    const int rounds = (KQ + U - 1) / U;
    int r = 0;
    for (; r + 2 <= rounds; r += 2) {
        request(vb, (r + 1) * U);
        consume(va, r * U);
        request(va, (r + 2) * U);
        consume(vb, (r + 1) * U);
    }
    if (r < rounds) consume(va, r * U);
    if (d < D) out[d] = acc;
}

// Threshold without sampling: the documents are cut into G <= 4096 groups of 64 * gw consecutive documents (one wave of this
// kernel each); the k-th largest of the G group maxima is a LOWER bound of the k-th largest score (k groups hold a score at
// least that large), so "every score whose digit is >= the digit of that bound" always contains the top k -- about
// G * -ln(1 - k/G) of them, a few percent more than k (measured, 100k documents: 100-110 candidates for k = 100, 1630-1710 for
// k = 1024).  Each wave stores its maximum in its own slot: no atomics.
__global__ __launch_bounds__(256) void search1_combine_kernel(const double* __restrict__ bm, const float* __restrict__ sim, int64_t D, double wa,
                                                              float wb, double* __restrict__ final_out, const Search1State* __restrict__ st,
                                                              unsigned long long* __restrict__ wmax, int gw, int gl) {
    double ma;
    float mb;
    search1_maxima(st, &ma, &mb);
    const int lane = threadIdx.x & 63;
    const int64_t group = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    double m = -INFINITY;
    for (int c = 0; c < gw; ++c) {
        const int64_t d = (group * gw + c) * 64 + lane;
        if (d < D) {
            const double f = combine_score(bm[d], sim[d], ma, mb, wa, wb);
            final_out[d] = f;
            m = fmax(m, f);
        }
    }
    // gl < 64 (only with gw == 1): the wave's 64 documents form 64 / gl groups of gl consecutive ones -- when k is a large part of a
    // small index there must be several times k groups for the k-th largest group maximum to be a useful bound
    for (int o = (gl >> 1); o >= 1; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    if ((lane & (gl - 1)) == 0) wmax[group * (64 / gl) + lane / gl] = (unsigned long long)order_key(m);      // a group past the last document stores the image of -inf
}

struct S1HandOn {                // LDS of one workgroup of search1_collect_kernel / search1_finish_kernel
    uint32_t hist[4096];
    int scan[17];
    uint32_t n, other;
};

// Threshold digit = the digit of the k-th largest of `groups` values; group_digit(g) is value_digit of group g's value.  Every
// workgroup finds it itself (the values come from L2).  Digit 0 is everything below -2: combined scores are >= -1 unless a required /
// excluded term made them -inf, so with fewer than k groups above it the threshold is digit 1 -- every finite score is a candidate and
// the ranking fills up with -inf ties.  Also clears the candidate counter and the flag s1_hand_on uses.
template <typename F>
__device__ __forceinline__ uint32_t s1_threshold_digit(S1HandOn& sh, int groups, int k, F group_digit) {
    const int tid = threadIdx.x;
    for (int i = tid; i < 4096; i += S1_COLLECT_THREADS) sh.hist[i] = 0;
    if (tid == 0) {
        sh.n = 0;
        sh.other = 0;
    }
    __syncthreads();
    for (int g0 = 0; g0 < groups; g0 += S1_COLLECT_THREADS) {
        const int g = g0 + tid;
        const uint32_t dg = g < groups ? group_digit(g) : 0u;
        hist_add(sh.hist, dg, dg != 0u);
    }
    __syncthreads();
    const int digit = find_bin_from_top(sh.hist, k, sh.scan, 1).digit;
    return digit < 0 ? 1u : (uint32_t)digit;
}

// Document d (score f) is a candidate if its digit is at or above the threshold: the candidates go to this workgroup's own slots (LDS
// counter, one add per wave), their number and "a finite score stayed behind" to bcnt / bflag.
__device__ __forceinline__ void s1_hand_on(S1HandOn& sh, double f, int64_t d, int64_t D, uint32_t dmin, uint32_t* __restrict__ bcnt,
                                           uint32_t* __restrict__ bflag, unsigned long long* __restrict__ bkey, uint32_t* __restrict__ bid, int bcap) {
    const int tid = threadIdx.x, lane = tid & 63;
    const bool take = d < D && value_digit(f) >= dmin;
    if (d < D && !take && f != -INFINITY) sh.other = 1u;
    const uint64_t m = __ballot(take);
    if (m != 0) {
        uint32_t base = 0;
        const int leader = __ffsll((unsigned long long)m) - 1;
        if (lane == leader) base = atomicAdd(&sh.n, (uint32_t)__popcll(m));
        base = __shfl(base, leader);
        if (take) {
            const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1));
            if (slot < (uint32_t)bcap) {
                bkey[(int64_t)blockIdx.x * bcap + slot] = order_key(f);
                bid[(int64_t)blockIdx.x * bcap + slot] = (uint32_t)d;
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        bcnt[blockIdx.x] = sh.n;                    // may exceed the cap: the ranking kernel then takes the exact path
        bflag[blockIdx.x] = sh.other;
    }
}

// The group values are the group maxima search1_combine_kernel stored; the scores are its combined scores.
__global__ __launch_bounds__(S1_COLLECT_THREADS) void search1_collect_kernel(const double* __restrict__ final_in, int64_t D, int k,
                                                                             const unsigned long long* __restrict__ wmax, int groups,
                                                                             uint32_t* __restrict__ bcnt, uint32_t* __restrict__ bflag,
                                                                             unsigned long long* __restrict__ bkey, uint32_t* __restrict__ bid, int bcap) {
    __shared__ S1HandOn sh;
    const uint32_t dmin = s1_threshold_digit(sh, groups, k, [&](int g) { return value_digit(key_value(wmax[g])); });
    const int64_t d = (int64_t)blockIdx.x * S1_COLLECT_THREADS + threadIdx.x;
    const double f = d < D ? final_in[d] : -INFINITY;
    s1_hand_on(sh, f, d, D, dmin, bcnt, bflag, bkey, bid, bcap);
}

// search1_combine_kernel + search1_collect_kernel in ONE launch (round 4): the threshold no longer comes from the group maxima of the
// combined scores (which only exist after a pass over all documents, hence the launch boundary between the two kernels) but from the
// WITNESS documents the score kernel left behind, two per wave: a workgroup combines the 2 G witnesses itself (G x 32 B from L2),
// takes per wave the larger of its two, and uses the digit of the k-th largest of those G values -- still a lower bound of the k-th
// largest combined score, because every value belongs to a real document and no two waves share one.  Then it combines its own 1024
// documents (combine_score), stores them for the fallback paths and the caller, and hands on the candidates.  Used when a group is a
// whole wave (gl == 64, gw == 1: 160 k <= D <= 262 k documents at k = 100); other sizes keep the two kernels.
__global__ __launch_bounds__(S1_COLLECT_THREADS) void search1_finish_kernel(const double* __restrict__ bm, const float* __restrict__ sim, int64_t D, int k,
                                                                            double wa, float wb, double* __restrict__ final_out,
                                                                            const Search1State* __restrict__ st, const Search1Witness* __restrict__ wit,
                                                                            int groups, uint32_t* __restrict__ bcnt, uint32_t* __restrict__ bflag,
                                                                            unsigned long long* __restrict__ bkey, uint32_t* __restrict__ bid, int bcap) {
    __shared__ S1HandOn sh;
    double ma;
    float mb;
    search1_maxima(st, &ma, &mb);
    const uint32_t dmin = s1_threshold_digit(sh, groups, k, [&](int g) {
        const Search1Witness w = wit[g];
        return value_digit(fmax(combine_score(w.bm_a, w.sim_a, ma, mb, wa, wb), combine_score(w.bm_b, w.sim_b, ma, mb, wa, wb)));
    });
    const int64_t d = (int64_t)blockIdx.x * S1_COLLECT_THREADS + threadIdx.x;
    double f = -INFINITY;
    if (d < D) {
        f = combine_score(bm[d], sim[d], ma, mb, wa, wb);
        final_out[d] = f;
    }
    s1_hand_on(sh, f, d, D, dmin, bcnt, bflag, bkey, bid, bcap);
}

// Handle-less entry points (hipts_combine / hipts_topk) keep their small scratch here: one slot
// per (device, purpose), intentionally never freed (freeing at static-destruction time would
// race the HIP runtime's own teardown).  Callers are single-threaded per device by contract.
DevBuf& scratch_buf(int device, int which) {
    static DevBuf* bufs = new DevBuf[64 * 4];
    return bufs[(device & 63) * 4 + (which & 3)];
}

int copy_out(void* dst, const void* src_dev, size_t bytes, int memspace, hipStream_t s) {
    if (!dst || bytes == 0) return HIPTS_OK;
    if (memspace == HIPTS_DEVICE) {
        if (dst != src_dev) HIPTS_HIP(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToDevice, s));
    } else {
        HIPTS_HIP(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, s));
        HIPTS_HIP(hipStreamSynchronize(s));
    }
    return HIPTS_OK;
}

enum QueryProfCat { QP_BM25 = 0, QP_SIM, QP_ROWMAX, QP_COMBINE, QP_TOPK, QP_S1_SCORE, QP_S1_COMBINE, QP_S1_COLLECT, QP_S1_TOPK, QP_COUNT };
static_assert(QP_COUNT == HIPTS_QUERY_PROF_CATEGORIES, "category count");
const char* const kQueryProfNames[QP_COUNT] = {"bm25_postings_kernel", "sim_mfma_kernel", "rowmax_kernel<float>", "combine_kernel", "topk_kernel",
                                               "search1_score_kernel", "search1_combine_kernel", "search1_collect_kernel | search1_finish_kernel", "topk_kernel<candidates>"};

struct QueryProfScope : EventProfile<QP_COUNT>::Scope {
    QueryProfScope(hipts_bm25* h, hipStream_t s, int cat, double bytes) : Scope(h && h->prof ? &h->ep : nullptr, s, cat, 0.0, bytes) {}
};

// rows of kk results each (ids hi, scores hv) as rows of k >= kk: the places past kk hold id -1, score -inf
void pad_topk_rows(const int32_t* hi, const double* hv, int nq, int kk, int k, int32_t* ids_out, double* vals_out) {
    if (kk == k) {
        memcpy(ids_out, hi, (size_t)nq * k * 4);
        memcpy(vals_out, hv, (size_t)nq * k * 8);
        return;
    }
    for (int q = 0; q < nq; ++q)
        for (int i = 0; i < k; ++i) {
            ids_out[(size_t)q * k + i] = i < kk ? hi[(size_t)q * kk + i] : -1;
            vals_out[(size_t)q * k + i] = i < kk ? hv[(size_t)q * kk + i] : -INFINITY;
        }
}

static_assert(S1_STATE_BYTES == sizeof(Search1State) && S1_WITNESS_BYTES == sizeof(Search1Witness), "search1_plan lays these out");
}  // namespace

const QueryKnobs& hipts::query_knobs() {
    static const QueryKnobs knobs = [] {
        auto is = [](const char* name, const char* value) { const char* e = getenv(name); return e && strcmp(e, value) == 0; };
        auto zero = [](const char* name) { const char* e = getenv(name); return e && atoi(e) == 0; };
        QueryKnobs k;
        k.sim_tiled = !is("HIPTS_SIM", "rows");
        k.sim_wide = !zero("HIPTS_SIM_WIDE");
        k.sim_parts = !zero("HIPTS_SIM_PARTS");
        k.bm25_scan = is("HIPTS_BM25", "scan");
        k.bm25_parts = getenv("HIPTS_BM25_PARTS") ? atoi(getenv("HIPTS_BM25_PARTS")) : 0;
        k.search1 = !is("HIPTS_SEARCH1", "0");
        k.s1_finish = !zero("HIPTS_SEARCH1_FINISH");
        k.s1_d2h = is("HIPTS_SEARCH1_D2H", "1");
        k.s1_flag = !is("HIPTS_SEARCH1_FLAG", "0");
        k.s1_pipe = !zero("HIPTS_S1_PIPE");
        k.fused_topk = !zero("HIPTS_SEARCH_FUSED_TOPK");
        k.overlap = getenv("HIPTS_SEARCH_OVERLAP") && atoi(getenv("HIPTS_SEARCH_OVERLAP")) != 0;
        return k;
    }();
    return knobs;
}

// =============================================================================================
// Dense index handle
// =============================================================================================
struct hipts_index {
    int device = 0;
    int dim = 0;
    int64_t len = 0, cap = 0;
    DevBuf rows;      // float [cap][dim]
    DevBuf tiled;     // tile-major copy for the query kernel (dim % 4 == 0): float4 [ceil(cap/32)][dim/4][32]
    DevBuf ws_q, ws_out;
};

namespace {

// The launches of sim_plan() (query_plan.h).  p.parts_grid > 0: the wide kernel's per-workgroup row maxima are left in parts ([query group
// of 256][SIM_PARTS_MAX_GRID][256] floats, p.parts_bytes); otherwise the caller runs rowmax_kernel over the stored products.
int launch_sim(const SimPlan& p, const float* index, const float* tiled, int64_t D, int K, const float* q_dev, int nq, float* out_dev,
               int64_t out_ld, hipStream_t s, float* parts = nullptr) {
    const size_t lds = (size_t)K * 32 * sizeof(float);
    HIPTS_REQUIRE(lds <= 160 * 1024, "index dim %d too large for the query tile in LDS", K);
    static PerDevice attr_set;
    {
        int dev = 0;
        HIPTS_HIP(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(attr_set.mu);
        if (!attr_set.done(dev)) {
            HIPTS_HIP(hipFuncSetAttribute((const void*)sim_mfma_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            HIPTS_HIP(hipFuncSetAttribute((const void*)sim_mfma_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            attr_set.mark(dev);
        }
    }
    HIPTS_REQUIRE(p.parts_grid == 0 || parts, "launch_sim: the plan wants a buffer for the row maxima");
    const float4* t4 = reinterpret_cast<const float4*>(tiled);
    for (int i = 0; i < p.wide_passes; ++i) {
        const SimPass w = sim_wide_pass(p, i);
        float* pm = p.parts_grid > 0 ? parts + (int64_t)i * SIM_PARTS_GROUP_FLOATS : nullptr;
        const float* qp = q_dev + (int64_t)w.q0 * K;
        float* op = out_dev + (int64_t)w.q0 * out_ld;
        if (w.nqb == 2) sim_mfma_wide_kernel<2><<<w.grid, 512, 0, s>>>(t4, D, K, qp, w.n, op, out_ld, pm);
        else if (w.nqb == 4) sim_mfma_wide_kernel<4><<<w.grid, 512, 0, s>>>(t4, D, K, qp, w.n, op, out_ld, pm);
        else sim_mfma_wide_kernel<8><<<w.grid, 512, 0, s>>>(t4, D, K, qp, w.n, op, out_ld, pm);
        HIPTS_LAUNCH_CHECK();
    }
    for (int i = 0; i < p.tail_passes; ++i) {
        const int q0 = p.tail_q0 + i * 32, n = std::min(32, nq - q0);
        if (p.tail_tiled) sim_mfma_kernel<true><<<p.tail_grid, SIM_THREADS, lds, s>>>(tiled, D, K, K, q_dev + (int64_t)q0 * K, n, out_dev + (int64_t)q0 * out_ld, out_ld);
        else sim_mfma_kernel<false><<<p.tail_grid, SIM_THREADS, lds, s>>>(index, D, K, K, q_dev + (int64_t)q0 * K, n, out_dev + (int64_t)q0 * out_ld, out_ld);
        HIPTS_LAUNCH_CHECK();
    }
    return HIPTS_OK;
}

int launch_bm25(hipts_bm25* h, const int32_t* qt_dev, const double* qw_dev, const int32_t* qp_dev, int nq, double* out_dev,
                hipStream_t s, double* max_out = nullptr) {
    const Bm25Plan plan = bm25_plan(nq, h->slice_docs, query_knobs());
    if (plan.kernel == Bm25Plan::SLICED) {
        HIPTS_TRY(h->ws_mark.reserve((size_t)nq * h->D));
        if (max_out) HIPTS_TRY(h->ws_maxpart.reserve((size_t)nq * plan.parts * 8));
        bm25_postings_sliced_kernel<<<dim3(nq, plan.parts), 512, 0, s>>>(h->d_tslice.as<int64_t>(), h->d_tdoc.as<int32_t>(), h->d_ttf.as<int32_t>(),
                                                                     h->d_dl.as<int32_t>(), h->d_idf.as<double>(), h->V, h->avgdl, h->D, h->slice_docs,
                                                                     BM25_SLICES / plan.parts, qt_dev, qw_dev, qp_dev, out_dev, h->ws_mark.as<uint8_t>(),
                                                                     max_out ? h->ws_maxpart.as<double>() : nullptr);
        HIPTS_LAUNCH_CHECK();
        if (max_out) {
            bm25_max_reduce_kernel<<<ceil_div(nq, 256), 256, 0, s>>>(h->ws_maxpart.as<double>(), plan.parts, max_out, nq);
            HIPTS_LAUNCH_CHECK();
        }
        return HIPTS_OK;
    }
    if (plan.kernel == Bm25Plan::POSTINGS) {
        HIPTS_TRY(h->ws_mark.reserve((size_t)nq * h->D));
        bm25_postings_kernel<<<nq, 1024, 0, s>>>(h->d_tptr.as<int64_t>(), h->d_tdoc.as<int32_t>(), h->d_ttf.as<int32_t>(),
                                                 h->d_dl.as<int32_t>(), h->d_idf.as<double>(), h->V, h->avgdl, h->D, qt_dev, qw_dev,
                                                 qp_dev, out_dev, h->ws_mark.as<uint8_t>(), max_out);
        HIPTS_LAUNCH_CHECK();
        return HIPTS_OK;
    }
    dim3 grid(ceil_div(h->D, 256), nq);
    bm25_score_kernel<<<grid, 256, 0, s>>>(h->d_ptr.as<int64_t>(), h->d_term.as<int32_t>(), h->d_tf.as<int32_t>(),
                                           h->d_dl.as<int32_t>(), h->d_idf.as<double>(), h->V, h->avgdl, h->D, qt_dev, qw_dev,
                                           qp_dev, out_dev);
    HIPTS_LAUNCH_CHECK();
    if (max_out) {
        rowmax_kernel<double><<<nq, 1024, 0, s>>>(out_dev, h->D, max_out);
        HIPTS_LAUNCH_CHECK();
    }
    return HIPTS_OK;
}

// The packed queries of a batch (query_pack): fills the host image `hin`; returns where its parts lie once it is copied to `dev`
struct PackedQueries { const int32_t* qt; const double* qw; const int32_t* qp; const float* qvec; };
PackedQueries pack_queries(const QueryPack& pk, char* hin, const void* dev, const int32_t* q_terms, const double* q_weights, const int32_t* q_ptr,
                           const float* q_vectors, int nt, int nq, int dim) {
    if (nt) {
        memcpy(hin, q_terms, (size_t)nt * 4);
        memcpy(hin + pk.off_w, q_weights, (size_t)nt * 8);
    }
    memcpy(hin + pk.off_p, q_ptr, (size_t)(nq + 1) * 4);
    if (dim) memcpy(hin + pk.off_v, q_vectors, (size_t)nq * dim * 4);
    const char* d = static_cast<const char*>(dev);
    return PackedQueries{reinterpret_cast<const int32_t*>(d), reinterpret_cast<const double*>(d + pk.off_w), reinterpret_cast<const int32_t*>(d + pk.off_p),
                         reinterpret_cast<const float*>(d + pk.off_v)};
}

// stage the CSR query description in the handle's workspace; returns device pointers
int stage_queries(hipts_bm25* h, const int32_t* q_terms, const double* q_weights, const int32_t* q_ptr, int nq, PackedQueries* q, hipStream_t s) {
    const int nt = q_ptr[nq];
    HIPTS_REQUIRE(q_ptr[0] == 0 && nt >= 0, "q_ptr must start at 0 and be non-decreasing");
    const QueryPack pack = query_pack(nt, nq, 0);
    HIPTS_TRY(h->ws_q.reserve(pack.bytes));
    std::vector<char> host(pack.bytes, 0);
    *q = pack_queries(pack, host.data(), h->ws_q.p, q_terms, q_weights, q_ptr, nullptr, nt, nq, 0);
    HIPTS_HIP(hipMemcpyAsync(h->ws_q.p, host.data(), pack.bytes, hipMemcpyHostToDevice, s));
    HIPTS_HIP(hipStreamSynchronize(s));   // `host` goes out of scope
    return HIPTS_OK;
}

// hipts_search for ONE query (webui.py:345-383 + the ranking of :191-192): four launches, no staging copy, results written by the
// last kernel straight into pinned host memory and published by a sequence number the host spins on.
int search_one(hipts_bm25* bm25, hipts_index* index, const int32_t* q_terms, const double* q_weights, int nt, const float* q_vector,
               double w_bm25, double w_sim, int k, int32_t* ids_out, double* vals_out, double* final_out_device, hipStream_t s) {
    const int64_t D = bm25->D;
    Search1Query Q;
    memset(&Q, 0, sizeof(Q));
    Q.nt = nt;
    Q.dim = index->dim;
    for (int j = 0; j < nt; ++j) {
        Q.terms[j] = q_terms[j];
        Q.weights[j] = q_weights[j];
    }
    memcpy(Q.q, q_vector, (size_t)index->dim * 4);
    HIPTS_TRY(bm25->ws_scores.reserve((size_t)D * 8));
    HIPTS_TRY(bm25->ws_sims.reserve((size_t)D * 4));
    if (!final_out_device) HIPTS_TRY(bm25->ws_final.reserve((size_t)D * 8));
    double* final_dev = final_out_device ? final_out_device : bm25->ws_final.as<double>();
    const QueryKnobs& knobs = query_knobs();
    const Search1Plan P = search1_plan(D, k, knobs);
    const int kk = P.kk, blocks3 = P.blocks3;
    if (bm25->s1_state.bytes < P.ws_bytes) {
        HIPTS_TRY(bm25->s1_state.alloc(P.ws_bytes));
        bm25->s1_dirty = true;
    }
    char* ws = bm25->s1_state.as<char>();
    Search1State* st = reinterpret_cast<Search1State*>(ws);
    if (bm25->s1_dirty) HIPTS_HIP(hipMemsetAsync(st, 0, sizeof(Search1State), s));
    bm25->s1_dirty = true;                    // until the last kernel (which clears the maxima slots) has been enqueued
    unsigned long long* wmax = reinterpret_cast<unsigned long long*>(ws + P.off_wmax);
    uint32_t* bcnt = reinterpret_cast<uint32_t*>(ws + P.off_bcnt);
    uint32_t* bflag = reinterpret_cast<uint32_t*>(ws + P.off_bflag);
    unsigned long long* bkey = reinterpret_cast<unsigned long long*>(ws + P.off_bkey);
    uint32_t* bid = reinterpret_cast<uint32_t*>(ws + P.off_bid);
    Search1Witness* wit = P.finish ? reinterpret_cast<Search1Witness*>(ws + P.off_wit) : nullptr;
    HIPTS_TRY(bm25->pin_out.reserve(P.out_bytes + 192));
    double* hv = bm25->pin_out.as<double>();                  // pinned + mapped: the last kernel stores the results here
    int32_t* hi = reinterpret_cast<int32_t*>(hv + kk);
    const bool via_copy = knobs.s1_d2h, use_flag = knobs.s1_flag && !via_copy && !bm25->prof;
    uint32_t* flag = reinterpret_cast<uint32_t*>(bm25->pin_out.as<char>() + P.off_flag);       // its own cache line behind the results
    if (++bm25->s1_seq == 0) bm25->s1_seq = 1;
    const uint32_t seq = bm25->s1_seq;
    if (use_flag) __atomic_store_n(flag, 0u, __ATOMIC_RELAXED);          // (fresh pinned memory is not zeroed)
    if (via_copy) HIPTS_TRY(bm25->ws_out.reserve(P.out_bytes + 64));
    double* ov = via_copy ? bm25->ws_out.as<double>() : hv;            // where the last kernel stores: scores, then ids
    int32_t* oi = reinterpret_cast<int32_t*>(ov + kk);
    {
        QueryProfScope ps(bm25, s, QP_S1_SCORE, (double)D * index->dim * 4.0 + (double)bm25->nnz * 8.0 + (double)D * (8 + 4 + 8 + 4));
        auto* score = knobs.s1_pipe ? search1_score_kernel<true> : search1_score_kernel<false>;       // HIPTS_S1_PIPE=0: the sequential form
        score<<<P.grid_score, S1_THREADS, 0, s>>>(Q, index->tiled.as<float4>(), D, bm25->d_ptr.as<int64_t>(), bm25->d_term.as<int32_t>(),
                                                  bm25->d_tf.as<int32_t>(), bm25->d_dl.as<int32_t>(), bm25->d_idf.as<double>(), bm25->V, bm25->avgdl,
                                                  bm25->ws_scores.as<double>(), bm25->ws_sims.as<float>(), st, wit);
        HIPTS_LAUNCH_CHECK();
    }
    if (P.finish) {
        QueryProfScope ps(bm25, s, QP_S1_COLLECT, (double)D * 20.0 + (double)blocks3 * (double)P.waves * 32.0);
        search1_finish_kernel<<<blocks3, S1_COLLECT_THREADS, 0, s>>>(bm25->ws_scores.as<double>(), bm25->ws_sims.as<float>(), D, kk, w_bm25, (float)w_sim,
                                                                     final_dev, st, wit, (int)P.waves, bcnt, bflag, bkey, bid, P.bcap);
        HIPTS_LAUNCH_CHECK();
    } else {
        {
            QueryProfScope ps(bm25, s, QP_S1_COMBINE, (double)D * 20.0);
            search1_combine_kernel<<<P.blocks2, 256, 0, s>>>(bm25->ws_scores.as<double>(), bm25->ws_sims.as<float>(), D, w_bm25, (float)w_sim, final_dev,
                                                           st, wmax, P.gw, P.gl);
            HIPTS_LAUNCH_CHECK();
        }
        {
            QueryProfScope ps(bm25, s, QP_S1_COLLECT, (double)D * 8.0);
            search1_collect_kernel<<<blocks3, S1_COLLECT_THREADS, 0, s>>>(final_dev, D, kk, wmax, P.groups, bcnt, bflag, bkey, bid, P.bcap);
            HIPTS_LAUNCH_CHECK();
        }
    }
    {
        QueryProfScope ps(bm25, s, QP_S1_TOPK, (double)kk * 24.0);
        uint32_t* clear = reinterpret_cast<uint32_t*>(st);             // the maxima slots, up to dbg
        const int clear_words = (int)(offsetof(Search1State, dbg) / 4);
        const TopkHandOn hand{clear, clear_words, clear + clear_words, bcnt, bflag, bkey, bid, blocks3, P.bcap};
        const TopkPublish pub{use_flag ? flag : nullptr, seq};
        topk_kernel<<<1, 1024, 0, s>>>(TopkScores{final_dev}, D, kk, oi, ov, hand, pub);
        HIPTS_LAUNCH_CHECK();
    }
    bm25->s1_dirty = false;
    if (via_copy) HIPTS_HIP(hipMemcpyAsync(hv, ov, P.out_bytes, hipMemcpyDeviceToHost, s));
    bool seen = false;
    if (use_flag) {
        // spin on the sequence number the last kernel releases after its result stores (bounded: then the ordinary synchronise)
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t spins = 0;; ++spins) {
            if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) {
                seen = true;
                break;
            }
            if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
        }
    }
    if (!seen) HIPTS_HIP(hipStreamSynchronize(s));
    pad_topk_rows(hi, hv, 1, kk, k, ids_out, vals_out);
    return HIPTS_OK;
}

}  // namespace

extern "C" {

int hipts_query_profile_enable(hipts_bm25_t* h, int enable) {
    HIPTS_REQUIRE(h, "null handle");
    h->prof = enable != 0;
    if (enable) h->ep.reset();
    return HIPTS_OK;
}

int hipts_query_profile_read(hipts_bm25_t* h, int category, double* total_ms, int64_t* launches, double* total_bytes) {
    HIPTS_REQUIRE(h && category >= 0 && category < QP_COUNT, "hipts_query_profile_read: bad arguments");
    HIPTS_TRY(use_device(h->device));
    HIPTS_TRY(h->ep.resolve());
    if (total_ms) *total_ms = h->ep.ms[category];
    if (launches) *launches = h->ep.n[category];
    if (total_bytes) *total_bytes = h->ep.bytes[category];
    return HIPTS_OK;
}

int hiptsdbg_topk_stamps(unsigned long long* host16) {
#ifdef HIPTS_X_TOPK_STAMPS
    HIPTS_HIP(hipMemcpyFromSymbol(host16, HIP_SYMBOL(g_topk_stamps), 16 * 8));
    if (getenv("HIPTS_DBG_BM25_STAMPS"))      // slots 8..11 <- the BM25 kernel's clear / postings / mask+max (tools/bm25_stamps.py)
        HIPTS_HIP(hipMemcpyFromSymbol(host16 + 8, HIP_SYMBOL(g_bm25_stamps), 4 * 8));
    return HIPTS_OK;
#else
    (void)host16;
    return set_error(HIPTS_ERR_STATE, "built without HIPTS_X_TOPK_STAMPS");
#endif
}

int hiptsdbg_search1_last(hipts_bm25_t* h, uint32_t* candidates, uint32_t* took_candidate_path) {
    HIPTS_REQUIRE(h && h->s1_state.p && candidates && took_candidate_path, "hiptsdbg_search1_last: no one-query search has run on this handle");
    HIPTS_TRY(use_device(h->device));
    uint32_t dbg[4];
    HIPTS_HIP(hipMemcpy(dbg, reinterpret_cast<const char*>(h->s1_state.p) + offsetof(Search1State, dbg), sizeof(dbg), hipMemcpyDeviceToHost));
    *candidates = dbg[0];
    *took_candidate_path = dbg[1];
    return HIPTS_OK;
}

int hiptsdbg_search1_plan(int64_t D, int k, unsigned knob_bits, hiptsdbg_search1_plan_t* out) {
    HIPTS_REQUIRE(out && D >= 1 && D < (1ll << 32) && k >= 1 && k <= TOPK_MAX_K, "hiptsdbg_search1_plan: bad argument");
    QueryKnobs kn;
    kn.s1_finish = (knob_bits & HIPTSDBG_QUERY_FINISH) != 0;
    *out = search1_plan(D, k, kn);
    return HIPTS_OK;
}

int hiptsdbg_sim_plan(int have_tiled, int64_t D, int K, int nq, int want_parts, unsigned knob_bits, hiptsdbg_sim_plan_t* out) {
    HIPTS_REQUIRE(out && D >= 1 && K >= 1 && nq >= 1, "hiptsdbg_sim_plan: bad argument");
    QueryKnobs kn;
    kn.sim_wide = (knob_bits & HIPTSDBG_QUERY_WIDE) != 0;
    kn.sim_tiled = (knob_bits & HIPTSDBG_QUERY_TILED) != 0;
    kn.sim_parts = (knob_bits & HIPTSDBG_QUERY_PARTS) != 0;
    *out = sim_plan(have_tiled != 0, D, K, nq, want_parts != 0, kn);
    return HIPTS_OK;
}

int hipts_query_profile_name(int category, char* buf, size_t n) {
    HIPTS_REQUIRE(buf && n > 0 && category >= 0 && category < QP_COUNT, "hipts_query_profile_name: bad arguments");
    snprintf(buf, n, "%s", kQueryProfNames[category]);
    return HIPTS_OK;
}

// ---------------------------------------------------------------------------------------------
int hipts_bm25_build(const int64_t* doc_ptr, const int32_t* term_ids, int64_t num_docs, int32_t vocab, int device,
                     hipts_bm25_t** out) {
    HIPTS_REQUIRE(doc_ptr && out && num_docs >= 0 && vocab >= 0, "hipts_bm25_build: bad arguments");
    HIPTS_REQUIRE(term_ids || doc_ptr[num_docs] == 0, "hipts_bm25_build: term_ids is NULL");
    HIPTS_TRY(use_device(device));
    auto* h = new hipts_bm25();
    h->device = device;
    h->D = num_docs;
    h->V = vocab;
    h->h_ptr.assign(1, 0);
    h->h_df.assign((size_t)vocab, 0);
    h->h_dl.reserve((size_t)num_docs);
    std::unordered_map<int32_t, int32_t> slot;   // term -> position in this document's list (dict insertion order)
    int64_t sum_dl = 0;
    for (int64_t d = 0; d < num_docs; ++d) {     // genmodel.py:57-73
        slot.clear();
        const size_t base = h->h_term.size();
        int64_t dl = 0;
        for (int64_t i = doc_ptr[d]; i < doc_ptr[d + 1]; ++i) {
            const int32_t t = term_ids[i];
            if (t < 0 || t >= vocab) continue;   // tag not in dictionary (:59)
            ++dl;
            auto it = slot.find(t);
            if (it == slot.end()) {
                slot.emplace(t, (int32_t)(h->h_term.size() - base));
                h->h_term.push_back(t);
                h->h_tf.push_back(1);
            } else {
                h->h_tf[base + it->second] += 1;
            }
        }
        for (size_t i = base; i < h->h_term.size(); ++i) h->h_df[h->h_term[i]] += 1;
        h->h_dl.push_back(dl);
        sum_dl += dl;
        h->h_ptr.push_back((int64_t)h->h_term.size());
    }
    h->nnz = (int64_t)h->h_term.size();
    // np.mean of an int64 array: exact integer sum (< 2^53) then one division          genmodel.py:76
    h->avgdl = num_docs > 0 ? (double)sum_dl / (double)num_docs : std::numeric_limits<double>::quiet_NaN();
    h->h_idf.assign((size_t)vocab, 0.0);
    for (int32_t t = 0; t < vocab; ++t) {        // genmodel.py:80-82
        const int64_t df = h->h_df[t];
        if (df > 0) h->h_idf[t] = std::log(1 + ((double)(num_docs - df) + 0.5) / ((double)df + 0.5));
    }
    std::vector<int32_t> dl32((size_t)num_docs);
    for (int64_t d = 0; d < num_docs; ++d) dl32[d] = (int32_t)h->h_dl[d];
    // term-major postings (documents ascending inside a term) for the postings kernel
    std::vector<int64_t> tptr((size_t)vocab + 1, 0);
    for (int32_t t = 0; t < vocab; ++t) tptr[t + 1] = tptr[t] + h->h_df[t];
    std::vector<int32_t> tdoc((size_t)h->nnz), ttf((size_t)h->nnz);
    {
        std::vector<int64_t> fill(tptr.begin(), tptr.end() - 1);
        for (int64_t d = 0; d < num_docs; ++d)
            for (int64_t i = h->h_ptr[d]; i < h->h_ptr[d + 1]; ++i) {
                const int64_t pos = fill[h->h_term[i]]++;
                tdoc[pos] = (int32_t)d;
                ttf[pos] = h->h_tf[i];
            }
    }
    // every term's posting offsets at BM25_SLICES fixed document boundaries (bm25_postings_sliced_kernel); the boundaries are multiples
    // of 8 documents so that a slice of a score row starts on a 64-byte line
    std::vector<int64_t> tslice;
    h->slice_docs = (num_docs % 8 == 0 && num_docs >= 8192) ? (num_docs / 8 / BM25_SLICES) * 8 : 0;
    if (h->slice_docs > 0) {
        tslice.resize((size_t)vocab * (BM25_SLICES + 1));
        for (int32_t t = 0; t < vocab; ++t) {
            const int32_t* first = tdoc.data() + tptr[t];
            const int32_t* last = tdoc.data() + tptr[t + 1];
            for (int sl = 0; sl <= BM25_SLICES; ++sl) {
                const int64_t bound = sl == BM25_SLICES ? num_docs : (int64_t)sl * h->slice_docs;
                tslice[(size_t)t * (BM25_SLICES + 1) + sl] = tptr[t] + (std::lower_bound(first, last, (int32_t)std::min<int64_t>(bound, INT32_MAX)) - first);
            }
        }
    }
    int st = HIPTS_OK;
    if (h->slice_docs > 0 && ((st = h->d_tslice.alloc(tslice.size() * 8)) || (st = upload(h->d_tslice.p, tslice.data(), tslice.size() * 8)))) {
        delete h;
        return st;
    }
    if ((st = h->d_ptr.alloc((size_t)(num_docs + 1) * 8)) || (st = h->d_term.alloc((size_t)h->nnz * 4)) ||
        (st = h->d_tf.alloc((size_t)h->nnz * 4)) || (st = h->d_dl.alloc((size_t)num_docs * 4)) ||
        (st = h->d_idf.alloc((size_t)vocab * 8)) || (st = upload(h->d_ptr.p, h->h_ptr.data(), (size_t)(num_docs + 1) * 8)) ||
        (st = upload(h->d_term.p, h->h_term.data(), (size_t)h->nnz * 4)) ||
        (st = upload(h->d_tf.p, h->h_tf.data(), (size_t)h->nnz * 4)) || (st = upload(h->d_dl.p, dl32.data(), (size_t)num_docs * 4)) ||
        (st = upload(h->d_idf.p, h->h_idf.data(), (size_t)vocab * 8)) || (st = h->d_tptr.alloc((size_t)(vocab + 1) * 8)) ||
        (st = h->d_tdoc.alloc((size_t)h->nnz * 4)) || (st = h->d_ttf.alloc((size_t)h->nnz * 4)) ||
        (st = upload(h->d_tptr.p, tptr.data(), (size_t)(vocab + 1) * 8)) || (st = upload(h->d_tdoc.p, tdoc.data(), (size_t)h->nnz * 4)) ||
        (st = upload(h->d_ttf.p, ttf.data(), (size_t)h->nnz * 4))) {
        delete h;
        return st;
    }
    *out = h;
    return HIPTS_OK;
}

int hipts_bm25_destroy(hipts_bm25_t* h) {
    if (h) {
        (void)hipSetDevice(h->device);
        if (h->side) {
            (void)hipStreamSynchronize(h->side);
            (void)hipStreamDestroy(h->side);
        }
        for (auto& sl : h->slot)
            if (sl.done) (void)hipEventDestroy(sl.done);
        if (h->ev_in) (void)hipEventDestroy(h->ev_in);
        if (h->ev_bm25) (void)hipEventDestroy(h->ev_bm25);
        for (auto& ev : h->rel_ev)
            if (ev) (void)hipEventDestroy(ev);
        delete h;
    }
    return HIPTS_OK;
}

int hipts_bm25_info(const hipts_bm25_t* h, int64_t* num_docs, int64_t* nnz, int32_t* vocab, double* avgdl) {
    HIPTS_REQUIRE(h, "null handle");
    if (num_docs) *num_docs = h->D;
    if (nnz) *nnz = h->nnz;
    if (vocab) *vocab = h->V;
    if (avgdl) *avgdl = h->avgdl;
    return HIPTS_OK;
}

int hipts_bm25_export(const hipts_bm25_t* h, int64_t* csr_ptr, int32_t* csr_term, int32_t* csr_tf, int64_t* doc_len,
                      int64_t* df, double* idf) {
    HIPTS_REQUIRE(h, "null handle");
    if (csr_ptr) memcpy(csr_ptr, h->h_ptr.data(), h->h_ptr.size() * 8);
    if (csr_term) memcpy(csr_term, h->h_term.data(), h->h_term.size() * 4);
    if (csr_tf) memcpy(csr_tf, h->h_tf.data(), h->h_tf.size() * 4);
    if (doc_len) memcpy(doc_len, h->h_dl.data(), h->h_dl.size() * 8);
    if (df) memcpy(df, h->h_df.data(), h->h_df.size() * 8);
    if (idf) memcpy(idf, h->h_idf.data(), h->h_idf.size() * 8);
    return HIPTS_OK;
}

int hipts_bm25_set_idf(hipts_bm25_t* h, const double* idf) {
    HIPTS_REQUIRE(h && idf, "null argument");
    HIPTS_TRY(use_device(h->device));
    h->h_idf.assign(idf, idf + h->V);
    return upload(h->d_idf.p, h->h_idf.data(), (size_t)h->V * 8);
}

int hipts_bm25_set_avgdl(hipts_bm25_t* h, double avgdl) {
    HIPTS_REQUIRE(h, "null argument");
    HIPTS_REQUIRE(avgdl > 0.0, "hipts_bm25_set_avgdl: avgdl must be positive");
    h->avgdl = avgdl;
    return HIPTS_OK;
}

int hipts_bm25_score(hipts_bm25_t* h, const int32_t* q_terms, const double* q_weights, const int32_t* q_ptr, int nq,
                     double* scores_out, int out_memspace, void* stream) {
    HIPTS_REQUIRE(h && q_ptr && scores_out && nq >= 1, "hipts_bm25_score: bad arguments");
    HIPTS_TRY(use_device(h->device));
    hipStream_t s = (hipStream_t)stream;
    PackedQueries q;
    HIPTS_TRY(stage_queries(h, q_terms, q_weights, q_ptr, nq, &q, s));
    double* out_dev = scores_out;
    if (out_memspace != HIPTS_DEVICE) {
        HIPTS_TRY(h->ws_scores.reserve((size_t)nq * h->D * 8));
        out_dev = h->ws_scores.as<double>();
    }
    HIPTS_TRY(launch_bm25(h, q.qt, q.qw, q.qp, nq, out_dev, s));
    return copy_out(scores_out, out_dev, (size_t)nq * h->D * 8, out_memspace, s);
}

// ---------------------------------------------------------------------------------------------
int hipts_index_create(int dim, int64_t capacity, int device, hipts_index_t** out) {
    HIPTS_REQUIRE(out && dim >= 4 && dim % 4 == 0 && dim <= 1280, "hipts_index_create: dim must be a multiple of 4 and <= 1280");
    HIPTS_TRY(use_device(device));
    auto* h = new hipts_index();
    h->device = device;
    h->dim = dim;
    h->cap = capacity > 0 ? capacity : 1024;
    int st = h->rows.alloc((size_t)h->cap * dim * 4);
    if (st) {
        delete h;
        return st;
    }
    *out = h;
    return HIPTS_OK;
}

int hipts_index_destroy(hipts_index_t* h) {
    if (h) {
        (void)hipSetDevice(h->device);
        delete h;
    }
    return HIPTS_OK;
}

int hipts_index_add(hipts_index_t* h, const float* rows, int64_t nrows, int rows_memspace) {
    HIPTS_REQUIRE(h && (rows || nrows == 0) && nrows >= 0, "hipts_index_add: bad arguments");
    HIPTS_TRY(use_device(h->device));
    if (h->len + nrows > h->cap) {
        int64_t ncap = std::max<int64_t>(h->cap * 2, h->len + nrows);
        DevBuf nb;
        HIPTS_TRY(nb.alloc((size_t)ncap * h->dim * 4));
        HIPTS_HIP(hipMemcpy(nb.p, h->rows.p, (size_t)h->len * h->dim * 4, hipMemcpyDeviceToDevice));
        std::swap(nb.p, h->rows.p);
        std::swap(nb.bytes, h->rows.bytes);
        h->cap = ncap;
    }
    HIPTS_HIP(hipMemcpy(h->rows.as<float>() + h->len * h->dim, rows, (size_t)nrows * h->dim * 4,
                        rows_memspace == HIPTS_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    const int64_t old_len = h->len;
    h->len += nrows;
    if (h->dim % 4 == 0 && nrows > 0) {
        // the tile-major copy the product kernel reads: size it like `rows`, then rewrite the tiles the new rows touch
        const size_t need = (size_t)((h->cap + 31) / 32) * 32 * h->dim * 4;
        if (h->tiled.bytes < need) {
            DevBuf nb;
            HIPTS_TRY(nb.alloc(need));
            if (h->tiled.p && old_len > 0)
                HIPTS_HIP(hipMemcpy(nb.p, h->tiled.p, (size_t)((old_len + 31) / 32) * 32 * h->dim * 4, hipMemcpyDeviceToDevice));
            std::swap(nb.p, h->tiled.p);
            std::swap(nb.bytes, h->tiled.bytes);
        }
        const int64_t t0 = old_len / 32, t1 = (h->len + 31) / 32;
        const int64_t total = (t1 - t0) * (h->dim / 4) * 32;
        retile_kernel<<<ceil_div(total, 256), 256>>>(h->rows.as<float>(), h->tiled.as<float4>(), h->len, h->dim, t0, t1);
        HIPTS_LAUNCH_CHECK();
        HIPTS_HIP(hipDeviceSynchronize());
    }
    return HIPTS_OK;
}

int hipts_index_len(const hipts_index_t* h, int64_t* nrows) {
    HIPTS_REQUIRE(h && nrows, "null argument");
    *nrows = h->len;
    return HIPTS_OK;
}

int hipts_index_vector_by_id(const hipts_index_t* h, int64_t id, float* out_host) {
    HIPTS_REQUIRE(h && out_host && id >= 0 && id < h->len, "hipts_index_vector_by_id: id out of range");
    HIPTS_TRY(use_device(h->device));
    HIPTS_HIP(hipMemcpy(out_host, h->rows.as<float>() + id * h->dim, (size_t)h->dim * 4, hipMemcpyDeviceToHost));
    return HIPTS_OK;
}

int hipts_index_export(const hipts_index_t* h, int64_t first, int64_t nrows, float* out_host) {
    HIPTS_REQUIRE(h && first >= 0 && nrows >= 0 && first + nrows <= h->len, "hipts_index_export: rows [%lld, %lld) out of range (len %lld)",
                  (long long)first, (long long)(first + nrows), (long long)h->len);
    if (nrows == 0) return HIPTS_OK;
    HIPTS_REQUIRE(out_host, "hipts_index_export: null output");
    HIPTS_TRY(use_device(h->device));
    HIPTS_HIP(hipMemcpy(out_host, h->rows.as<float>() + first * h->dim, (size_t)nrows * h->dim * 4, hipMemcpyDeviceToHost));
    return HIPTS_OK;
}

int hipts_index_data(const hipts_index_t* h, void** device_ptr) {
    HIPTS_REQUIRE(h && device_ptr, "null argument");
    *device_ptr = h->rows.p;
    return HIPTS_OK;
}

}  // extern "C"

int hipts::index_tiled_view(const hipts_index_t* h, const float4** tiled, int64_t* len, int* dim, int* device) {
    HIPTS_REQUIRE(h && tiled && len && dim && device, "null argument");
    *tiled = h->len > 0 ? h->tiled.as<float4>() : nullptr;
    *len = h->len;
    *dim = h->dim;
    *device = h->device;
    return HIPTS_OK;
}

extern "C" {

int hipts_index_query(hipts_index_t* h, const float* queries, int queries_memspace, int nq, float* scores_out,
                      int out_memspace, void* stream) {
    HIPTS_REQUIRE(h && queries && scores_out && nq >= 1, "hipts_index_query: bad arguments");
    HIPTS_REQUIRE(h->len > 0, "hipts_index_query: empty index");
    HIPTS_TRY(use_device(h->device));
    hipStream_t s = (hipStream_t)stream;
    float* out_dev = scores_out;
    if (out_memspace != HIPTS_DEVICE) {
        HIPTS_TRY(h->ws_out.reserve((size_t)nq * h->len * 4));
        out_dev = h->ws_out.as<float>();
    }
    const QueryKnobs& knobs = query_knobs();
    if (search1_eligible(nq, h->dim, h->tiled.p != nullptr, h->len, knobs) && queries_memspace != HIPTS_DEVICE) {
        Sim1Query Q;                      // a host query goes straight into the kernel arguments: no staging copy
        memset(&Q, 0, sizeof(Q));
        Q.dim = h->dim;
        memcpy(Q.q, queries, (size_t)h->dim * 4);
        sim1_kernel<<<ceil_div(h->len, 128), 128, 0, s>>>(Q, h->tiled.as<float4>(), h->len, out_dev);
        HIPTS_LAUNCH_CHECK();
        return copy_out(scores_out, out_dev, (size_t)h->len * 4, out_memspace, s);
    }
    const float* q_dev = queries;
    if (queries_memspace != HIPTS_DEVICE) {
        HIPTS_TRY(h->ws_q.reserve((size_t)nq * h->dim * 4));
        HIPTS_HIP(hipMemcpyAsync(h->ws_q.p, queries, (size_t)nq * h->dim * 4, hipMemcpyHostToDevice, s));
        q_dev = h->ws_q.as<float>();
    }
    HIPTS_TRY(launch_sim(sim_plan(h->tiled.p != nullptr, h->len, h->dim, nq, false, knobs), h->rows.as<float>(), h->tiled.as<float>(), h->len, h->dim, q_dev, nq,
                         out_dev, h->len, s));
    return copy_out(scores_out, out_dev, (size_t)nq * h->len * 4, out_memspace, s);
}

// ---------------------------------------------------------------------------------------------
int hipts_combine(const double* a, const float* b, int nq, int64_t n, double wa, double wb, int norm_a, int norm_b,
                  double* out, int device, void* stream) {
    HIPTS_REQUIRE(a && b && out && nq >= 1 && n >= 1, "hipts_combine: bad arguments");
    HIPTS_TRY(use_device(device));
    DevBuf& maxbuf = scratch_buf(device, 0);
    HIPTS_TRY(maxbuf.reserve((size_t)nq * 16));
    double* ma = norm_a ? maxbuf.as<double>() : nullptr;
    float* mb = norm_b ? reinterpret_cast<float*>(maxbuf.as<double>() + nq) : nullptr;
    HIPTS_TRY(hipts_rowmax(norm_a ? a : nullptr, norm_b ? b : nullptr, nq, n, ma, mb, device, stream));
    return hipts_combine_with_max(a, b, nq, n, wa, wb, ma, mb, out, device, stream);
}

int hipts_rowmax(const double* a, const float* b, int nq, int64_t n, double* max_a_out, float* max_b_out, int device,
                 void* stream) {
    HIPTS_REQUIRE(nq >= 1 && n >= 1 && (!a || max_a_out) && (!b || max_b_out), "hipts_rowmax: bad arguments");
    HIPTS_TRY(use_device(device));
    hipStream_t s = (hipStream_t)stream;
    if (a) {
        rowmax_kernel<double><<<nq, 1024, 0, s>>>(a, n, max_a_out);
        HIPTS_LAUNCH_CHECK();
    }
    if (b) {
        rowmax_kernel<float><<<nq, 1024, 0, s>>>(b, n, max_b_out);
        HIPTS_LAUNCH_CHECK();
    }
    return HIPTS_OK;
}

int hipts_combine_with_max(const double* a, const float* b, int nq, int64_t n, double wa, double wb, const double* max_a,
                           const float* max_b, double* out, int device, void* stream) {
    HIPTS_REQUIRE(a && b && out && nq >= 1 && n >= 1, "hipts_combine_with_max: bad arguments");
    HIPTS_TRY(use_device(device));
    dim3 grid(ceil_div(n, 256), nq);
    combine_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(a, b, n, wa, (float)wb, max_a, max_b, nullptr, out);
    HIPTS_LAUNCH_CHECK();
    return HIPTS_OK;
}

int hipts_topk(const double* vals, int nq, int64_t n, int k, int32_t* ids_out, double* vals_out, int out_memspace,
               int device, void* stream) {
    HIPTS_REQUIRE(vals && ids_out && vals_out && nq >= 1 && n >= 1, "hipts_topk: bad arguments");
    HIPTS_REQUIRE(k >= 1 && k <= TOPK_MAX_K, "hipts_topk: k must be in [1, %d]", TOPK_MAX_K);
    HIPTS_REQUIRE(n < (1ll << 32), "hipts_topk: n too large");
    HIPTS_TRY(use_device(device));
    hipStream_t s = (hipStream_t)stream;
    const int kk = (int)std::min<int64_t>(k, n);
    if (out_memspace == HIPTS_DEVICE) {
        HIPTS_REQUIRE(kk == k, "hipts_topk: k > n needs host outputs");
        topk_kernel<<<nq, 1024, 0, s>>>(TopkScores{vals}, n, k, ids_out, vals_out);
        HIPTS_LAUNCH_CHECK();
        return HIPTS_OK;
    }
    DevBuf& obuf = scratch_buf(device, 1);
    HIPTS_TRY(obuf.reserve((size_t)nq * kk * 12 + 64));
    double* ov = obuf.as<double>();
    int32_t* oi = reinterpret_cast<int32_t*>(ov + (size_t)nq * kk);
    topk_kernel<<<nq, 1024, 0, s>>>(TopkScores{vals}, n, kk, oi, ov);
    HIPTS_LAUNCH_CHECK();
    std::vector<int32_t> hi((size_t)nq * kk);
    std::vector<double> hv((size_t)nq * kk);
    HIPTS_HIP(hipMemcpyAsync(hi.data(), oi, hi.size() * 4, hipMemcpyDeviceToHost, s));
    HIPTS_HIP(hipMemcpyAsync(hv.data(), ov, hv.size() * 8, hipMemcpyDeviceToHost, s));
    HIPTS_HIP(hipStreamSynchronize(s));
    pad_topk_rows(hi.data(), hv.data(), nq, kk, k, ids_out, vals_out);
    return HIPTS_OK;
}

// scores ranked at or before (after_val, after_id) in the order (value descending, index ascending) become -inf: the top k of the
// result are the NEXT k of that order
__global__ __launch_bounds__(256) void mask_ranked_before_kernel(const double* __restrict__ vals, int64_t n, double after_val, int64_t after_id,
                                                                 double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = vals[i];
    const bool later = v < after_val || (v == after_val && i > after_id);
    out[i] = later ? v : -INFINITY;
}

int hipts_topk_after(const double* vals, int64_t n, int k, double after_val, int64_t after_id, int32_t* ids_out, double* vals_out,
                     int device, void* stream) {
    HIPTS_REQUIRE(vals && ids_out && vals_out && n >= 1 && k >= 1 && k <= TOPK_MAX_K, "hipts_topk_after: bad arguments");
    HIPTS_REQUIRE(after_val == after_val, "hipts_topk_after: after_val is NaN");
    HIPTS_TRY(use_device(device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf& mbuf = scratch_buf(device, 2);
    HIPTS_TRY(mbuf.reserve((size_t)n * 8));
    mask_ranked_before_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(vals, n, after_val, after_id, mbuf.as<double>());
    HIPTS_LAUNCH_CHECK();
    return hipts_topk(mbuf.as<double>(), 1, n, k, ids_out, vals_out, HIPTS_HOST, device, stream);
}

// One batch of queries: pack, copy, launch everything and the copy back into slot `sl`'s pinned buffer, record its event.  Does not wait.
static int search_submit_impl(hipts_bm25_t* bm25, hipts_index_t* index, const int32_t* q_terms, const double* q_weights, const int32_t* q_ptr,
                              const float* q_vectors, int nq, double w_bm25, double w_sim, int k, double* final_out_device, int sl, hipStream_t s) {
    HIPTS_REQUIRE(bm25 && index && q_ptr && q_vectors && nq >= 1, "hipts_search: bad arguments");
    HIPTS_REQUIRE(sl == 0 || sl == 1, "hipts_search_submit: slot must be 0 or 1");
    HIPTS_REQUIRE(bm25->device == index->device, "hipts_search: handles live on different devices");
    HIPTS_REQUIRE(bm25->D == index->len, "hipts_search: BM25 corpus has %lld documents, index has %lld rows",
                  (long long)bm25->D, (long long)index->len);
    HIPTS_TRY(use_device(bm25->device));
    hipts_bm25::SearchSlot& S = bm25->slot[sl];
    HIPTS_REQUIRE(!S.pending, "hipts_search_submit: slot %d still holds an uncollected batch", sl);
    // ws_q / ws_scores / ws_sims / ws_out are shared by the two slots: stream order is what keeps batch i + 1 off batch i's rows
    HIPTS_REQUIRE(!bm25->slot[sl ^ 1].pending || bm25->slot[sl ^ 1].stream == s,
                  "hipts_search_submit: slot %d holds a batch submitted on another stream (all batches of a handle use ONE stream)", sl ^ 1);
    S.stream = s;
    const int64_t D = bm25->D;
    HIPTS_REQUIRE(k >= 1 && k <= TOPK_MAX_K, "hipts_search: k must be in [1, %d]", TOPK_MAX_K);
    const int nt = q_ptr[nq];
    HIPTS_REQUIRE(q_ptr[0] == 0 && nt >= 0, "q_ptr must start at 0 and be non-decreasing");
    S.nq = nq;
    S.k = k;
    const QueryKnobs& knobs = query_knobs();
    if (search1_eligible(nq, index->dim, index->tiled.p != nullptr, D, knobs) && nt <= S1_MAX_TERMS) {
        // the one-query path completes inside the call (its last kernel stores into pinned memory and the host spins on a flag)
        S.ids1.resize((size_t)k);
        S.vals1.resize((size_t)k);
        HIPTS_TRY(search_one(bm25, index, q_terms, q_weights, nt, q_vectors, w_bm25, w_sim, k, S.ids1.data(), S.vals1.data(), final_out_device, s));
        S.host_result = true;
        S.pending = true;
        return HIPTS_OK;
    }
    S.host_result = false;
    if (!S.done) HIPTS_HIP(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
    // queries, weights, offsets and the query vectors travel as ONE packed copy from pinned memory (no bounce buffer, no
    // synchronisation before the kernels); the results come back the same way
    const QueryPack pack = query_pack(nt, nq, index->dim);
    HIPTS_TRY(S.pin_in.reserve(pack.bytes));
    HIPTS_TRY(bm25->ws_q.reserve(pack.bytes));
    const PackedQueries q = pack_queries(pack, S.pin_in.as<char>(), bm25->ws_q.p, q_terms, q_weights, q_ptr, q_vectors, nt, nq, index->dim);
    HIPTS_HIP(hipMemcpyAsync(bm25->ws_q.p, S.pin_in.p, pack.bytes, hipMemcpyHostToDevice, s));
    HIPTS_TRY(bm25->ws_scores.reserve((size_t)nq * D * 8));
    HIPTS_TRY(bm25->ws_sims.reserve((size_t)nq * D * 4));
    // Without a caller who wants the combined rows they are never written: the top-k kernel combines on the fly (TopkScores::a)
    const bool fused = knobs.fused_topk && final_out_device == nullptr;
    double* final_dev = final_out_device;
    if (!final_dev && !fused) {
        HIPTS_TRY(bm25->ws_final.reserve((size_t)nq * D * 8));
        final_dev = bm25->ws_final.as<double>();
    }
    // row maxima (webui.py:377-380): the BM25 workgroup reduces its own row while it still owns it; the
    // index product's maximum is a separate pass (folding it into the product with one atomicMax per
    // tile and query was measured 3.5x SLOWER: 200k atomics on 32 addresses).
    HIPTS_TRY(bm25->ws_max.reserve((size_t)nq * 16));
    double* ma = bm25->ws_max.as<double>();
    float* mb = reinterpret_cast<float*>(ma + nq);
    // BM25 and the index product share no data.  Round 4 measured them on two streams (HIPTS_SEARCH_OVERLAP=1): 396-398 k queries/s either
    // way -- side by side BM25 takes 234-336 us instead of 156-167 and the product 262-363 instead of 233: both fill the wave slots of
    // every CU, so they take turns rather than share.  One stream stays the default.
    const SimPlan sim = sim_plan(index->tiled.p != nullptr, D, index->dim, nq, fused, knobs);
    hipStream_t sb = s;
    if (knobs.overlap) {
        if (!bm25->side) {
            HIPTS_HIP(hipStreamCreateWithFlags(&bm25->side, hipStreamNonBlocking));
            HIPTS_HIP(hipEventCreateWithFlags(&bm25->ev_in, hipEventDisableTiming));
            HIPTS_HIP(hipEventCreateWithFlags(&bm25->ev_bm25, hipEventDisableTiming));
        }
        sb = bm25->side;
        HIPTS_HIP(hipEventRecord(bm25->ev_in, s));              // the packed queries are on the device
        HIPTS_HIP(hipStreamWaitEvent(sb, bm25->ev_in, 0));
    }
    {
        // algorithmic bytes: the posting lists of the queries' terms (8 B per entry + the document length gathered with it) and the
        // three passes over each query's score row (clear, mask / maximum) -- DESIGN.md section 4
        double pb = 0.0;
        for (int j = 0; j < nt; ++j)
            if (q_terms[j] >= 0 && q_terms[j] < bm25->V) pb += (double)bm25->h_df[q_terms[j]] * 12.0;
        QueryProfScope ps(bm25, sb, QP_BM25, pb + (double)nq * D * 8.0 * 3);
        HIPTS_TRY(launch_bm25(bm25, q.qt, q.qw, q.qp, nq, bm25->ws_scores.as<double>(), sb, ma));
    }
    if (knobs.overlap) HIPTS_HIP(hipEventRecord(bm25->ev_bm25, sb));
    {
        QueryProfScope ps(bm25, s, QP_SIM, (double)sim.index_passes * D * index->dim * 4.0 + (double)nq * D * 4.0);
        if (sim.parts_bytes) HIPTS_TRY(bm25->ws_parts.reserve(sim.parts_bytes));
        HIPTS_TRY(launch_sim(sim, index->rows.as<float>(), index->tiled.as<float>(), D, index->dim, q.qvec, nq, bm25->ws_sims.as<float>(), D, s,
                             sim.parts_bytes ? bm25->ws_parts.as<float>() : nullptr));
    }
    if (sim.parts_grid == 0) {       // (otherwise the maxima came out of the product kernel's accumulators: the top-k kernel reduces its workgroups' values)
        QueryProfScope ps(bm25, s, QP_ROWMAX, (double)nq * D * 4.0);
        rowmax_kernel<float><<<nq, 1024, 0, s>>>(bm25->ws_sims.as<float>(), D, mb);
        HIPTS_LAUNCH_CHECK();
    }
    if (knobs.overlap) HIPTS_HIP(hipStreamWaitEvent(s, bm25->ev_bm25, 0));      // BM25 rows and their maxima are complete
    if (!fused) {
        QueryProfScope ps(bm25, s, QP_COMBINE, (double)nq * D * 20.0);
        dim3 grid(ceil_div(D, 256), nq);
        combine_kernel<<<grid, 256, 0, s>>>(bm25->ws_scores.as<double>(), bm25->ws_sims.as<float>(), D, w_bm25, (float)w_sim, ma,
                                            mb, nullptr, final_dev);
        HIPTS_LAUNCH_CHECK();
    }
    const int kk = (int)std::min<int64_t>(k, D);
    S.kk = kk;
    const size_t out_bytes = (size_t)nq * kk * 12;
    HIPTS_TRY(bm25->ws_out.reserve(out_bytes + 64));
    HIPTS_TRY(S.pin_out.reserve(out_bytes + 64));
    double* ov = bm25->ws_out.as<double>();
    int32_t* oi = reinterpret_cast<int32_t*>(ov + (size_t)nq * kk);
    {
        QueryProfScope ps(bm25, s, QP_TOPK, (double)nq * D * (fused ? 12.0 : 8.0));
        if (fused) {
            TopkScores fz;                       // the two addends, combined where the kernel reads them
            fz.a = bm25->ws_scores.as<double>();
            fz.b = bm25->ws_sims.as<float>();
            fz.wa = w_bm25;
            fz.wb = (float)w_sim;
            fz.max_a = ma;
            fz.max_b = sim.parts_grid > 0 ? nullptr : mb;
            fz.max_b_parts = sim.parts_grid > 0 ? bm25->ws_parts.as<float>() : nullptr;      // the index product left its workgroups' row maxima
            fz.parts = sim.parts_grid;
            topk_kernel<<<nq, 1024, 0, s>>>(fz, D, kk, oi, ov);
        } else {
            topk_kernel<<<nq, 1024, 0, s>>>(TopkScores{final_dev}, D, kk, oi, ov);
        }
        HIPTS_LAUNCH_CHECK();
    }
    HIPTS_HIP(hipMemcpyAsync(S.pin_out.p, ov, out_bytes, hipMemcpyDeviceToHost, s));
    HIPTS_HIP(hipEventRecord(S.done, s));
    S.pending = true;
    return HIPTS_OK;
}

int hipts_search_collect(hipts_bm25_t* bm25, int sl, int32_t* ids_out, double* vals_out) {
    HIPTS_REQUIRE(bm25 && ids_out && vals_out && (sl == 0 || sl == 1), "hipts_search_collect: bad arguments");
    hipts_bm25::SearchSlot& S = bm25->slot[sl];
    HIPTS_REQUIRE(S.pending, "hipts_search_collect: slot %d holds no submitted batch", sl);
    S.pending = false;
    const int k = S.k;
    if (S.host_result) {
        memcpy(ids_out, S.ids1.data(), (size_t)k * 4);
        memcpy(vals_out, S.vals1.data(), (size_t)k * 8);
        return HIPTS_OK;
    }
    HIPTS_TRY(use_device(bm25->device));
    HIPTS_HIP(hipEventSynchronize(S.done));
    const int nq = S.nq, kk = S.kk;
    const double* hv = S.pin_out.as<double>();
    const int32_t* hi = reinterpret_cast<const int32_t*>(hv + (size_t)nq * kk);
    pad_topk_rows(hi, hv, nq, kk, k, ids_out, vals_out);
    return HIPTS_OK;
}

int hipts_search(hipts_bm25_t* bm25, hipts_index_t* index, const int32_t* q_terms, const double* q_weights,
                 const int32_t* q_ptr, const float* q_vectors, int nq, double w_bm25, double w_sim, int k, int32_t* ids_out,
                 double* vals_out, double* final_out_device, void* stream) {
    HIPTS_REQUIRE(bm25 && ids_out && vals_out, "hipts_search: bad arguments");
    HIPTS_REQUIRE(!bm25->slot[0].pending, "hipts_search: a submitted batch waits in slot 0 (hipts_search_collect it first)");
    HIPTS_TRY(search_submit_impl(bm25, index, q_terms, q_weights, q_ptr, q_vectors, nq, w_bm25, w_sim, k, final_out_device, 0, (hipStream_t)stream));
    return hipts_search_collect(bm25, 0, ids_out, vals_out);
}

int hipts_search_submit(hipts_bm25_t* bm25, hipts_index_t* index, const int32_t* q_terms, const double* q_weights, const int32_t* q_ptr,
                        const float* q_vectors, int nq, double w_bm25, double w_sim, int k, int slot, void* stream) {
    return search_submit_impl(bm25, index, q_terms, q_weights, q_ptr, q_vectors, nq, w_bm25, w_sim, k, nullptr, slot, (hipStream_t)stream);
}

}  // extern "C"
