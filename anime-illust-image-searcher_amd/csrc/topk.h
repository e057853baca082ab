// topk.h -- the ranking kernel of query.hip: top-k by (value descending, index ascending), one workgroup of 1024 per query.  Device code
// only, in an anonymous namespace (as rank_util.h).  Three callers: hipts_topk (plain score rows), the batched search (the two addends
// instead of their sum: TopkScores::a / b) and the one-query path (candidates handed on by search1_collect_kernel / search1_finish_kernel,
// results published to pinned host memory behind a sequence number).  The kernel body at the end of the file calls the phases in order.
// tests/topk_arms.py mirrors this file's constants and decisions (which arm a row reaches): keep the two in step.
#pragma once
#include <cstdint>
#include <type_traits>

#include <hip/hip_runtime.h>

#include "query_plan.h"
#include "rank_util.h"

namespace {

// =============================================================================================
// top-k by (value descending, index ascending): one workgroup per query.
// MSB-first radix select over an order-preserving u64 image of the float64 value (12-bit digits,
// LDS histogram), early exit once the survivors fit the LDS candidate buffer, then a bitonic
// sort of the candidates.  Exact for ties (ordered gather of the lowest indices).
// =============================================================================================
constexpr int TOPK_CAP = 2048;
constexpr int TOPK_MAX_K = 1024;

__device__ __forceinline__ uint64_t order_key(double x) {
    if (x == 0.0) x = 0.0;   // -0.0 and +0.0 compare equal in the reference's sort
    uint64_t u = (uint64_t)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(uint64_t k) {
    uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

// Monotone (non-decreasing) 12-bit digit of a score, uniform in VALUE over [-2, 2): the fast path of the
// top-k histograms on it.  Everything below -2 (and NaN) is digit 0, everything from 2 up is 4095.
__device__ __forceinline__ uint32_t value_digit(double x) {
    const double t = (x + 2.0) * 1024.0;
    return t >= 4095.0 ? 4095u : (t > 0.0 ? (uint32_t)t : 0u);
}

// Histogram increment that survives concentration: when many lanes of a wave hold the SAME digit (ties: every
// document a required term excludes scores -inf; exponent digits of like-sized scores) plain LDS atomics
// serialise on one address.  The lanes that share the first active lane's digit are counted with one ballot
// and added once; the remaining lanes add individually.
__device__ __forceinline__ void hist_add(uint32_t* hist, uint32_t d, bool active) {
    const uint64_t act = __ballot(active);
    if (act == 0) return;
    const int leader = __ffsll((unsigned long long)act) - 1;
    const uint32_t dl = __shfl(d, leader);
    const uint64_t same = __ballot(active && d == dl);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[dl], (uint32_t)__popcll(same));
    else if (active && d != dl) atomicAdd(&hist[d], 1u);
}

// A workgroup streams its query's scores several times; each pass is bound by load latency x loads in flight,
// so every thread keeps TOPK_U independent 8-byte loads outstanding (128 KB per workgroup).
constexpr int TOPK_U = 16;
constexpr int TOPK_SORT_TARGET = 256;

using hipts::S1_BLOCK_CAP;           // query_plan.h
constexpr int S1_GATHER_BLOCKS = 1024;  // up to this many workgroups' slots are gathered through an offset table in LDS

#ifdef HIPTS_X_TOPK_STAMPS          // measurement-only build (-DHIPTS_X_TOPK_STAMPS=<workgroup>; tools/topk_stamps.py): wall-clock stamps of that workgroup, 10 ns units
__device__ unsigned long long g_topk_stamps[16];
#define TOPK_STAMP(i) do { __syncthreads(); if (blockIdx.x == HIPTS_X_TOPK_STAMPS && threadIdx.x == 0) g_topk_stamps[i] = wall_clock64(); } while (0)
#else
#define TOPK_STAMP(i) do { } while (0)
#endif

// webui.py:377-383 (and :208 with norm flags off):
//   out = wa * (a / max_a) + (double)((float)wb * (b / max_b))
// The one statement of it: the batched combine, the fused top-k and the one-query kernels all call this.  A maximum <= 0 (or absent:
// pass 0) means "do not divide".
__device__ __forceinline__ double combine_score(double A, float B, double max_a, float max_b, double wa, float wb) {
    if (max_a > 0.0) A = A / max_a;               // webui.py:379-380
    if (max_b > 0.0f) B = B / max_b;              // webui.py:377-378
    const float wB = wb * B;                      // python float * float32 array stays float32
    return wa * A + (double)wB;                   // webui.py:383
}

// The score source.  Plain: score rows `v`.  Fused (`a` set): the score rows as the two addends of webui.py:377-383 instead of their sum;
// the kernel computes wa * (a / max_a) + (double)(wb * (b / max_b)) (combine_score) wherever it reads a score,
// and the batched search neither writes nor re-reads the combined rows (round 3: 20 B per score of traffic less, one launch less).
// TopkScores is what the host fills, all rows; TopkRow is one workgroup's row of it, which the phases read through at / at2.
struct TopkRow {
    const double* __restrict__ v;        // [n] scores, or
    const double* __restrict__ a;        // [n] BM25 scores
    const float* __restrict__ b;         // [n] index products
    double ma, wa;                       // their row maxima (normalise when > 0) and weights
    float mb, wb;

    __device__ __forceinline__ bool fused() const { return a != nullptr; }
    __device__ __forceinline__ double comb(double A, float B) const { return combine_score(A, B, ma, mb, wa, wb); }
    __device__ __forceinline__ double at(int64_t i) const { return fused() ? comb(a[i], b[i]) : v[i]; }
    __device__ __forceinline__ double2 at2(int64_t i) const {              // scores i, i + 1 (i even, rows 16-byte aligned: wide())
        if (fused()) {
            const double2 A = *reinterpret_cast<const double2*>(a + i);
            const float2 B = *reinterpret_cast<const float2*>(b + i);
            return make_double2(comb(A.x, B.x), comb(A.y, B.y));
        }
        return *reinterpret_cast<const double2*>(v + i);
    }
    // 16-byte loads where the row allows it (even length, 16-byte aligned): 8-byte loads reach about 0.6 of the 16-byte rate on this
    // part (MI355X_MICROARCH.md, "8-B accesses 0.54-0.70x the 16-B rate"), and both passes of the fast path are pure streams
    __device__ __forceinline__ bool wide(int64_t n) const {
        return (n & 1) == 0 && (fused() ? ((reinterpret_cast<uintptr_t>(a) & 15) == 0 && (reinterpret_cast<uintptr_t>(b) & 7) == 0)
                                        : (reinterpret_cast<uintptr_t>(v) & 15) == 0);
    }
};

struct TopkScores {
    const double* v = nullptr;       // [nq][n] scores, or
    const double* a = nullptr;       // [nq][n] BM25 scores
    const float* b = nullptr;        // [nq][n] index products
    double wa = 0.0;
    float wb = 0.f;
    const double* max_a = nullptr;   // [nq] row maxima (normalise when > 0)
    const float* max_b = nullptr;
    const float* max_b_parts = nullptr;      // instead of max_b: [query / 256][SIM_PARTS_MAX_GRID][256] (query_plan.h) per-workgroup maxima of sim_mfma_wide_kernel,
    int parts = 0;                           //   `parts` workgroups each

    // this workgroup's row; all threads of the workgroup call it (one barrier when the maxima come in parts)
    __device__ __forceinline__ TopkRow row(int64_t n) const {
        const int64_t off = (int64_t)blockIdx.x * n;
        if (!a) return TopkRow{v + off, nullptr, nullptr, 0.0, 0.0, 0.f, 0.f};
        float mb;
        if (max_b_parts) {        // the maximum over the product kernel's workgroups (exact: the same value rowmax_kernel finds in the stored row)
            const float* pp = max_b_parts + (int64_t)(blockIdx.x >> 8) * hipts::SIM_PARTS_GROUP_FLOATS + (blockIdx.x & 255);
            mb = block_max<1024>((int)threadIdx.x < parts ? pp[(int64_t)threadIdx.x * 256] : -INFINITY);
        } else {
            mb = max_b[blockIdx.x];
        }
        return TopkRow{nullptr, a + off, b + off, max_a[blockIdx.x], wa, mb, wb};
    }
};

// The one-query path's candidates (per-workgroup slots of search1_collect_kernel / search1_finish_kernel); counts == nullptr: absent.
struct TopkHandOn {
    uint32_t* clear = nullptr;                   // the one-query state's maxima slots, `clear_words` words: zero again for the next query
    int clear_words = 0;
    uint32_t* dbg = nullptr;                     // {candidates, took the candidate path} of this query (hiptsdbg_search1_last)
    const uint32_t* __restrict__ counts = nullptr;       // [blocks] candidates of each workgroup (may exceed cap: the exact path runs)
    const uint32_t* __restrict__ flags = nullptr;        // [blocks] a finite score stayed behind
    const unsigned long long* __restrict__ keys = nullptr;   // [blocks][cap] order keys
    const uint32_t* __restrict__ ids = nullptr;          // [blocks][cap] documents
    int blocks = 0;
    int cap = S1_BLOCK_CAP;
};

// Results in pinned host memory: the sequence number the host spins on; flag == nullptr: absent.
struct TopkPublish {
    uint32_t* flag = nullptr;
    uint32_t seq = 0;
};

constexpr int TOPK_WSLOTS = TOPK_CAP / 16;       // candidate slots a wave of the fast-path collect owns
constexpr int TOPK_OVCAP = 1024;                 // entries of the overflow list the waves share

// The candidates, up to TOPK_CAP: order key and index, in two LDS arrays of their own as the kernel had them before it was split into
// phases -- NOT members of TopkLds.  This holds the bitonic sort to its earlier instruction stream: addressed through one LDS struct, the
// sort's swap arm carried four more v_add / v_sub per stage, and the rows that rank ~1500 candidates (k = 1024) measured 0.1-0.5 us
// slower per launch (LABNOTES.md).  The phases get the two arrays as this view, by value.
struct TopkCand {
    uint64_t* key;
    uint32_t* id;
};

struct TopkLds {                 // LDS of one workgroup of topk_kernel (the candidates aside)
    unsigned long long z0;       // largest order key among the scores of digit 0 (fast path that has to dip into that bin)
    uint32_t hist[4096];
    int soff[S1_GATHER_BLOCKS];
    int scratch[17];
    int cnt;                     // candidates in TopkCand
    // the fast-path collect's overflow list lives in the histogram's memory (free by then): 8 KB of keys, 4 KB of indices behind them
    __device__ __forceinline__ uint64_t* ov_key() { return reinterpret_cast<uint64_t*>(hist); }
    __device__ __forceinline__ uint32_t* ov_id() { return hist + 2 * TOPK_OVCAP; }
};

// One pass over a row: thread t of the 1024 examines scores W t .. W t + W - 1 of every STRIDE-th block of 1024 W scores, TOPK_U / W
// loads of 8 W bytes in flight (W = 2 needs row.wide(n)).  body(score, index, index < n) runs for EVERY lane, past the end of the row too
// (the bodies hold ballots); what it is given there is 0.0.  AHEAD: the next step's loads are requested before this step's values are
// examined (two register sets).
template <int W, int STRIDE, bool AHEAD, typename Body>
__device__ __forceinline__ void topk_stream(const TopkRow& row, int64_t n, Body body) {
    constexpr int U = TOPK_U / W;
    constexpr int64_t UNIT = (int64_t)STRIDE * 1024 * W, STEP = U * UNIT;
    using X = std::conditional_t<W == 2, double2, double>;
    const int tid = threadIdx.x;
    auto load = [&](X (&x)[U], int64_t base) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = base + u * UNIT + W * tid;
            if constexpr (W == 2) x[u] = i < n ? row.at2(i) : make_double2(0.0, 0.0);
            else x[u] = i < n ? row.at(i) : 0.0;
        }
    };
    auto examine = [&](const X (&x)[U], int64_t base) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = base + u * UNIT + W * tid;
            if constexpr (W == 2) {
                body(x[u].x, i, i < n);
                body(x[u].y, i + 1, i < n);
            } else {
                body(x[u], i, i < n);
            }
        }
    };
    if constexpr (AHEAD) {
        X x[U], xn[U];
        load(x, 0);
        for (int64_t base = 0; base < n; base += STEP) {
            load(xn, base + STEP);
            examine(x, base);
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = xn[u];
        }
    } else {
        for (int64_t base = 0; base < n; base += STEP) {
            X x[U];
            load(x, base);
            examine(x, base);
        }
    }
}

// Walk the 4096 bins from the top (thread t owns reversed bins 4t .. 4t + 3; bins below `lowest_bin` count as empty): the bin where the
// running count first reaches `want`.  digit < 0: the bins hold fewer than `want`.  All threads of a workgroup of 1024 call it, with want >= 1, and get the same answer;
// `scratch` is [17] in LDS and free again on return.
struct TopkBin {
    int digit, above, size;      // the bin, the entries in the bins above it, the entries in it
};
__device__ __forceinline__ TopkBin find_bin_from_top(const uint32_t* hist, int want, int* scratch, int lowest_bin) {
    const int tid = threadIdx.x;
    int own[4], ssum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int bin = 4095 - (4 * tid + j);
        own[j] = bin >= lowest_bin ? (int)hist[bin] : 0;
        ssum += own[j];
    }
    int total;
    const int excl = block_excl_scan(ssum, scratch, &total);
    if (total < want) return TopkBin{-1, total, 0};
    if (excl < want && want <= excl + ssum) {
        int run = excl;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (run < want && want <= run + own[j]) {
                scratch[0] = 4095 - (4 * tid + j);
                scratch[1] = run;
                scratch[2] = own[j];
            }
            run += own[j];
        }
    }
    __syncthreads();
    const TopkBin hit{scratch[0], scratch[1], scratch[2]};
    __syncthreads();
    return hit;
}

// Ordered compaction: emit(j, i) for the j-th lowest index i in [0, n) with pred(i), j < limit; stops as soon as enough are found.
// Returns how many it found (at least `limit` if it stopped early).  All 1024 threads call it.
template <typename Pred, typename Emit>
__device__ __forceinline__ int take_lowest_indices(int64_t n, int limit, int* scratch, Pred pred, Emit emit) {
    int taken = 0;
    for (int64_t i0 = 0; i0 < n && taken < limit; i0 += 1024) {
        const int64_t i = i0 + threadIdx.x;
        const int flag = (i < n && pred(i)) ? 1 : 0;
        int total;
        const int excl = block_excl_scan(flag, scratch, &total);
        if (flag && taken + excl < limit) emit(taken + excl, i);
        taken += total;
    }
    return taken;
}

// op over the 64 lanes' 64-bit values, in every lane
template <typename Op>
__device__ __forceinline__ uint64_t wave_reduce_u64(uint64_t v, Op op) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = op(v, (uint64_t)__shfl_xor((unsigned long long)v, o));
    return v;
}
struct MinU64 {
    __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return b < a ? b : a; }
};
struct MaxU64 {
    __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return b > a ? b : a; }
};

// ---- phase 1: the candidates handed on by search1_collect_kernel (per-workgroup slots): every score whose digit is at or above a
// threshold digit, i.e. all scores >= a pivot.  With at least k and at most CAP of them the top k are among them.  With fewer than
// k, and nothing but -inf below the pivot, they are ALL results and the rest are -inf ties in index order (*fill_need).
// Returns whether the candidates are in cand.key / cand.id [0, s.cnt).
__device__ __forceinline__ bool topk_gather_handed_on(TopkLds& s, const TopkCand cand, const TopkHandOn& pre, int k, int* fill_need) {
    const int tid = threadIdx.x;
    int mine = 0, bad = 0, other = 0;
    for (int b = tid; b < pre.blocks; b += 1024) {
        const int cb = (int)pre.counts[b];
        bad |= cb > pre.cap;
        mine += cb > pre.cap ? pre.cap : cb;
        other |= (int)pre.flags[b];
    }
    int c;
    const int excl = block_excl_scan(mine, s.scratch, &c);
    bad = __syncthreads_or(bad);
    const bool only_inf_below = __syncthreads_or(other) == 0;
    const bool done_fast = !bad && c <= TOPK_CAP && (c >= k || only_inf_below);
    if (done_fast && pre.blocks <= S1_GATHER_BLOCKS) {
        // one thread per CANDIDATE: its workgroup by bisection of the offsets (a workgroup may hand on hundreds when k is a large
        // part of a small index; a thread per workgroup copying them one by one took a round trip each)
        if (tid < pre.blocks) s.soff[tid] = excl;
        __syncthreads();
        for (int j = tid; j < c; j += 1024) {
            int lo = 0, hi = pre.blocks - 1;                   // last block whose offset is <= j
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (s.soff[mid] <= j) lo = mid; else hi = mid - 1;
            }
            const int64_t src = (int64_t)lo * pre.cap + (j - s.soff[lo]);
            cand.key[j] = pre.keys[src];
            cand.id[j] = pre.ids[src];
        }
        if (tid == 0) s.cnt = c;
        if (c < k) *fill_need = k - c;
    } else if (done_fast) {
        int off = excl;
        for (int b = tid; b < pre.blocks; b += 1024) {
            const int cb = (int)pre.counts[b];
            for (int i = 0; i < cb; ++i) {
                cand.key[off + i] = pre.keys[(int64_t)b * pre.cap + i];
                cand.id[off + i] = pre.ids[(int64_t)b * pre.cap + i];
            }
            off += cb;
        }
        if (tid == 0) s.cnt = c;
        if (c < k) *fill_need = k - c;
    }
    __syncthreads();
    TOPK_STAMP(13);
    for (int i = tid; i < pre.clear_words; i += 1024) pre.clear[i] = 0;    // the maxima slots are zero again for the next query (search1_combine_kernel has read them)
    if (tid == 0) {
        pre.dbg[0] = (uint32_t)c;
        pre.dbg[1] = done_fast ? 1u : 0u;
    }
    return done_fast;
}

// ---- phase 2, the fast path (measured: the exact radix select below spends ~200 us of a 233 us single-query call in the
// LDS atomics of its first histogram, 100 k of them).  Estimate the threshold from a 1/8 sample instead:
// histogram the sample over a VALUE-uniform 12-bit digit (scores are normalised sums in about [-1, 1], so
// the bins spread and the atomics do not pile up on a few exponents), pick the digit below which the sample
// holds ~k/8 + 3 sigma entries, and collect every score with digit >= that one.  The digit is monotone in
// the score, so the collected set is exactly "all scores >= a pivot": if it has at least k and at most CAP
// members it contains the top k and the sort below finishes the job; otherwise the exact path runs.
//
// The sampled threshold: the digit to collect from; 0 when the sample holds fewer than `want` entries above digit 0.
__device__ __forceinline__ int topk_sampled_threshold(TopkLds& s, const TopkRow& row, int64_t n, int k, bool wide) {
    const int tid = threadIdx.x;
    for (int i = tid; i < 4096; i += 1024) s.hist[i] = 0;
    if (tid == 0) s.cnt = 0;                                    // the overflow list's counter (topk_collect_from_digit)
    __syncthreads();
    // the first 1024 of every 8192 scores (16-byte loads: the first 2048 of every 16384, the same 1/8 sample); TOPK_U loads per thread
    // in flight (one load per step made the sample a chain of ~13 dependent round trips for 100 k scores: ~25 us of the kernel's ~80 per
    // workgroup)
    uint32_t smax = 0u;
    bool shave = false;
    auto sample = [&](double x, int64_t, bool in_row) {
        if (in_row) {
            smax = max(smax, value_digit(x));
            shave = true;
        }
    };
    if (wide) topk_stream<2, 8, false>(row, n, sample);
    else topk_stream<1, 8, false>(row, n, sample);
    // ONE histogram entry per thread: the largest digit among its ~12 samples.  The number of samples at or above a digit is at least
    // the number of thread maxima there, so the digit chosen below still leaves >= `want` samples above it (a few more when two of a
    // thread's samples qualify: 0.6 expected at k = 100, +9 % at k = 1024) -- and the histogram takes 1 k LDS atomics instead of 12.5 k
    // spread over 4096 bins (12 us of the kernel's 77 at k = 100: tools/topk_k.py, tools/topk_cases.py).
    TOPK_STAMP(1);
    hist_add(s.hist, smax, shave);
    __syncthreads();
    TOPK_STAMP(2);
    const int want = k / 8 + 3 * (int)ceilf(sqrtf((float)k / 8.0f)) + 4;
    const int digit = find_bin_from_top(s.hist, want, s.scratch, 0).digit;
    return digit < 0 ? 0 : digit;                               // fewer sampled entries than `want`: take everything
}

// Every score with digit >= dmin becomes a candidate; with `dip`, s.z0 becomes the largest order key among the others.
// the next step's TOPK_U loads are requested before this step's values are examined (two register sets): the pass was a chain of
// load round trips, one per 16 k scores
// Candidates go into the wave's OWN 128 slots of ckey / cid, placed by ballot and a wave-uniform count -- no atomics: ~250 adds on
// one LDS counter were 14 us of the kernel at k = 100.  A wave whose slots are full (skewed rows, k = 1024) appends to an overflow
// list that lives in the histogram's memory (free now) through a shared counter; the lists are packed by topk_pack_wave_lists.
// Returns the entries in this wave's list (uncapped); s.cnt counts the appends to the overflow list.
__device__ __forceinline__ int topk_collect_from_digit(TopkLds& s, const TopkCand cand, const TopkRow& row, int64_t n, uint32_t dmin, bool dip, bool wide) {
    const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
    uint64_t* ovk = s.ov_key();
    uint32_t* ovi = s.ov_id();
    unsigned long long z0 = 0ull;
    int wcnt = 0;
    auto examine = [&](double xv, int64_t i, bool in_row) {
        const bool c = in_row && value_digit(xv) >= dmin;
        const unsigned long long m = __ballot(c);
        if (m) {
            if (c) {
                const int pos = wcnt + __popcll(m & ((1ull << ln) - 1ull));
                if (pos < TOPK_WSLOTS) {
                    cand.key[wv * TOPK_WSLOTS + pos] = order_key(xv);
                    cand.id[wv * TOPK_WSLOTS + pos] = (uint32_t)i;
                } else {
                    const int slot = atomicAdd(&s.cnt, 1);
                    if (slot < TOPK_OVCAP) {
                        ovk[slot] = order_key(xv);
                        ovi[slot] = (uint32_t)i;
                    }
                }
            }
            wcnt += __popcll(m);
        }
        if (!c && dip && in_row) {
            const unsigned long long kx = order_key(xv);
            z0 = kx > z0 ? kx : z0;
        }
    };
    if (wide) topk_stream<2, 1, true>(row, n, examine);
    else topk_stream<1, 1, true>(row, n, examine);
    if (dip) {
        z0 = wave_reduce_u64(z0, MaxU64());
        if (ln == 0) atomicMax(&s.z0, z0);
    }
    return wcnt;
}

// pack the sixteen wave lists and the overflow list into ckey / cid [0, total): through registers (source and destination overlap).
// s.cnt becomes the number of candidates (more than CAP: not a fast-path row).
__device__ __forceinline__ void topk_pack_wave_lists(TopkLds& s, const TopkCand cand, int wcnt) {
    const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
    if (ln == 0) s.scratch[wv] = wcnt < TOPK_WSLOTS ? wcnt : TOPK_WSLOTS;
    __syncthreads();
    const int nov = s.cnt;                                         // entries the waves tried to append to the overflow list
    int off[17];
    off[0] = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) off[w + 1] = off[w] + s.scratch[w];
    const int total = off[16] + (nov < TOPK_OVCAP ? nov : TOPK_OVCAP);
    uint64_t mk[3];
    uint32_t mi[3];
    int md[3];
#pragma unroll
    for (int e = 0; e < 2; ++e) {                                    // wave-list slots tid and tid + 1024
        const int sl = tid + e * 1024, w = sl / TOPK_WSLOTS, j = sl - w * TOPK_WSLOTS;
        md[e] = j < s.scratch[w] ? off[w] + j : -1;
        mk[e] = cand.key[sl];
        mi[e] = cand.id[sl];
    }
    md[2] = tid < nov && tid < TOPK_OVCAP ? off[16] + tid : -1;      // overflow slot tid
    mk[2] = s.ov_key()[tid];
    mi[2] = s.ov_id()[tid];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 3; ++e)
        if (md[e] >= 0 && md[e] < TOPK_CAP) {
            cand.key[md[e]] = mk[e];
            cand.id[md[e]] = mi[e];
        }
    __syncthreads();
    if (tid == 0) s.cnt = nov > TOPK_OVCAP ? TOPK_CAP + 1 : total;   // an overflowing overflow list: not a fast-path row
    __syncthreads();
}

// Sampled threshold + collect.  Returns whether cand.key / cand.id [0, s.cnt) hold the top k (or, with *fill_need, all finite scores).
__device__ __forceinline__ bool topk_fast_path(TopkLds& s, const TopkCand cand, const TopkRow& row, int64_t n, int k, int* fill_need) {
    const bool wide = row.wide(n);
    const int digit = topk_sampled_threshold(s, row, n, k, wide);
    // The sample holds fewer than `want` entries above digit 0 when a required term has left most of the row -inf (digit 0): the top k
    // then reach into that bin.  Round 2 took "everything", overflowed the candidate buffer and fell to the exact radix select -- six
    // passes, 130-200 us for a row with fewer than ~300 finite scores, and the slowest row sets the launch time (measured:
    // tools/topk_cases.py).  Now: collect everything ABOVE digit 0 and look at what the bin holds; if nothing but -inf (the common case),
    // the candidates are all results and the rest are -inf ties in index order (the ordered fill at the end of the kernel).
    TOPK_STAMP(3);
    const bool dip = digit == 0;
    if (threadIdx.x == 0) s.z0 = 0ull;
    __syncthreads();                                                    // every thread has read its bins of the histogram
    const int wcnt = topk_collect_from_digit(s, cand, row, n, dip ? 1u : (uint32_t)digit, dip, wide);
    TOPK_STAMP(4);
    topk_pack_wave_lists(s, cand, wcnt);
    bool done_fast;
    if (dip) {
        // digit 0 empty (z0 == 0: every score was collected) or nothing but -inf in it
        done_fast = s.cnt <= TOPK_CAP && (s.z0 == 0ull || s.z0 == order_key(-INFINITY));
        if (done_fast && s.cnt < k) *fill_need = k - s.cnt;
    } else {
        done_fast = s.cnt >= k && s.cnt <= TOPK_CAP;
    }
    __syncthreads();
    return done_fast;
}

// ---- phase 3: the exact radix select.  The pivot: the scores to take are those whose key is above `low`, and `need` of those in
// [low, low + 2^(64 - pbits)) -- all of them when `fits`.
struct TopkPivot {
    uint64_t low;
    int need;
    bool fits;               // false: pbits == 64 and more than CAP exact ties at the threshold
};

// A first bin with more members than the buffers hold is usually one value repeated (every document
// a required term rules out scores -inf).  One pass decides: if the smallest and the largest key
// in the bin agree, the remaining five digit passes are known in advance.
__device__ __forceinline__ bool topk_bin_is_one_value(TopkLds& s, const TopkCand cand, const TopkRow& row, int64_t n, uint64_t prefix, int pbits, uint64_t* value) {
    const int tid = threadIdx.x;
    uint64_t mn = ~0ull, mx = 0ull;
    for (int64_t i = tid; i < n; i += 1024) {
        const uint64_t key = order_key(row.at(i));
        if ((key >> (64 - pbits)) == prefix) {
            mn = key < mn ? key : mn;
            mx = key > mx ? key : mx;
        }
    }
    mn = wave_reduce_u64(mn, MinU64());
    mx = wave_reduce_u64(mx, MaxU64());
    if ((tid & 63) == 0) {
        cand.key[tid >> 6] = mn;
        cand.key[16 + (tid >> 6)] = mx;
    }
    __syncthreads();
    mn = cand.key[0];
    mx = cand.key[16];
    for (int w = 1; w < 16; ++w) {
        mn = cand.key[w] < mn ? cand.key[w] : mn;
        mx = cand.key[16 + w] > mx ? cand.key[16 + w] : mx;
    }
    __syncthreads();
    *value = mn;
    return mn == mx;
}

__device__ __forceinline__ TopkPivot topk_radix_select(TopkLds& s, const TopkCand cand, const TopkRow& row, int64_t n, int k) {
    const int tid = threadIdx.x;
    uint64_t prefix = 0;
    int pbits = 0;
    int need = k;            // how many of the keys matching `prefix` are still wanted
    bool fits = false;
    const int shifts[6] = {52, 40, 28, 16, 4, 0};
    for (int pass = 0; pass < 6 && !fits; ++pass) {
        const int shift = shifts[pass];
        const int dbits = pass == 5 ? 4 : 12;
        for (int i = tid; i < 4096; i += 1024) s.hist[i] = 0;
        __syncthreads();
        topk_stream<1, 1, false>(row, n, [&](double x, int64_t, bool in_row) {
            const uint64_t key = order_key(x);
            hist_add(s.hist, (uint32_t)(key >> shift) & ((1u << dbits) - 1), in_row && (pbits == 0 || (key >> (64 - pbits)) == prefix));
        });
        __syncthreads();
        const TopkBin hit = find_bin_from_top(s.hist, need, s.scratch, 0);
        prefix = (prefix << dbits) | (uint64_t)(hit.digit & ((1 << dbits) - 1));
        pbits += dbits;
        need -= hit.above;       // the keys strictly above the chosen bin are all wanted
        // stop refining once the candidate set is small enough to SORT cheaply: the final bitonic sort costs
        // log^2 barriers (2048 candidates = 66 stages ~ 100 us, 256 = 36), a further pass over the scores ~15 us;
        // past the last digit (64 bits) whatever fits the LDS buffers is taken
        fits = (k - need) + hit.size <= (pbits < 64 ? max(TOPK_SORT_TARGET, k + 64) : TOPK_CAP);
        if (pass == 0 && !fits && hit.size > TOPK_CAP) {
            uint64_t value;
            if (topk_bin_is_one_value(s, cand, row, n, prefix, pbits, &value)) {
                prefix = value;
                pbits = 64;
                break;              // fits stays false: the ordered tie compaction takes the `need` lowest indices
            }
        }
    }
    return TopkPivot{pbits == 64 ? prefix : (prefix << (64 - pbits)), need, fits};
}

// ---- phase 4: the scores at or above the pivot into cand.key / cand.id [0, s.cnt)
__device__ __forceinline__ void topk_exact_collect(TopkLds& s, const TopkCand cand, const TopkRow& row, int64_t n, const TopkPivot& p) {
    const int tid = threadIdx.x;
    const uint64_t low = p.low;
    if (tid == 0) s.cnt = 0;
    __syncthreads();
    if (p.fits) {
        topk_stream<1, 1, false>(row, n, [&](double x, int64_t i, bool in_row) {
            const uint64_t key = order_key(x);
            if (in_row && key >= low) {
                const int slot = atomicAdd(&s.cnt, 1);
                cand.key[slot] = key;
                cand.id[slot] = (uint32_t)i;
            }
        });
        __syncthreads();
    } else {
        // pbits == 64 and more than CAP exact ties at the threshold: everything above it, then the
        // `need` lowest indices among the ties (ordered compaction).
        for (int64_t i = tid; i < n; i += 1024) {
            const uint64_t key = order_key(row.at(i));
            if (key > low) {
                const int slot = atomicAdd(&s.cnt, 1);
                cand.key[slot] = key;
                cand.id[slot] = (uint32_t)i;
            }
        }
        __syncthreads();
        const int base = s.cnt;
        const int taken = take_lowest_indices(n, p.need, s.scratch, [&](int64_t i) { return order_key(row.at(i)) == low; },
                                              [&](int j, int64_t i) {
                                                  cand.key[base + j] = low;
                                                  cand.id[base + j] = (uint32_t)i;
                                              });
        __syncthreads();
        if (tid == 0) s.cnt = base + (taken < p.need ? taken : p.need);
        __syncthreads();
    }
}

// ---- phase 5: the first `kout` of the `cnt` candidates in (key descending, index ascending) order to ids_out / vals_out (this query's rows)
__device__ __forceinline__ void topk_rank_and_store(TopkLds& s, const TopkCand cand, int cnt, int kout, int32_t* __restrict__ ids_out, double* __restrict__ vals_out) {
    const int tid = threadIdx.x;
    if (cnt <= 640) {
        // few candidates: rank by counting -- rank(i) = #{j : j before i in (key desc, id asc)} -- no barriers, LDS broadcasts
        // P adjacent lanes (as many as 1024 threads allow) share a candidate, each counting over every P-th entry (one thread per candidate walked the whole list as a
        // chain of LDS round trips: 26 us of the workgroup's 67 at k = 100 -- tools/topk_stamps.py); partial ranks meet by lane swaps
        __syncthreads();
        const int P = cnt <= 64 ? 16 : cnt <= 128 ? 8 : cnt <= 256 ? 4 : cnt <= 512 ? 2 : 1;
        const int c = tid / P, part = tid - c * P;
        const bool live = c < cnt;
        const uint64_t ki = live ? cand.key[c] : 0ull;
        const uint32_t ii = live ? cand.id[c] : 0u;
        int rank = 0;
        if (live) {
#pragma unroll 4
            for (int j = part; j < cnt; j += P) {
                const uint64_t kj = cand.key[j];
                const uint32_t ij = cand.id[j];
                rank += (kj > ki || (kj == ki && ij < ii)) ? 1 : 0;
            }
        }
        if (P >= 2) rank += __shfl_xor(rank, 1);
        if (P >= 4) rank += __shfl_xor(rank, 2);
        if (P >= 8) rank += __shfl_xor(rank, 4);
        if (P >= 16) rank += __shfl_xor(rank, 8);
        if (live && part == 0 && rank < kout) {
            ids_out[rank] = (int32_t)ii;
            vals_out[rank] = key_value(ki);
        }
    } else {
        int np2 = 64;
        while (np2 < cnt) np2 <<= 1;
        for (int i = cnt + tid; i < np2; i += 1024) {
            cand.key[i] = 0;
            cand.id[i] = 0xffffffffu;
        }
        __syncthreads();
        // bitonic sort, "greater first": (key desc, id asc)
        for (int size = 2; size <= np2; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < (np2 >> 1); t += 1024) {
                    const int lo = ((t / stride) * stride * 2) + (t % stride);
                    const int hi = lo + stride;
                    const bool desc = ((lo & size) == 0);
                    const uint64_t ka = cand.key[lo], kb = cand.key[hi];
                    const uint32_t ia = cand.id[lo], ib = cand.id[hi];
                    const bool a_first = (ka > kb) || (ka == kb && ia < ib);
                    if (a_first != desc) {
                        cand.key[lo] = kb; cand.key[hi] = ka;
                        cand.id[lo] = ib; cand.id[hi] = ia;
                    }
                }
                __syncthreads();
            }
        }
        for (int i = tid; i < kout; i += 1024) {
            ids_out[i] = (int32_t)cand.id[i];
            vals_out[i] = key_value(cand.key[i]);
        }
    }
}

// ---- phase 7: the results above went to pinned host memory.  Publish them to the HOST without waiting for the runtime's completion
// signal (a hipStreamSynchronize wake-up costs ~10 us): every storing thread fences at system scope, the workgroup meets,
// one lane releases the sequence number the host is spinning on.
__device__ __forceinline__ void topk_publish(const TopkPublish& pub) {
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(pub.flag, pub.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ids_out / vals_out are [nq][min(k, n)].
__global__ __launch_bounds__(1024) void topk_kernel(const TopkScores scores, int64_t n, int k, int32_t* __restrict__ ids_out,
                                                    double* __restrict__ vals_out, const TopkHandOn pre = TopkHandOn(),
                                                    const TopkPublish pub = TopkPublish()) {
    __shared__ TopkLds s;
    __shared__ uint64_t ckey[TOPK_CAP];
    __shared__ uint32_t cid[TOPK_CAP];
    const TopkCand cand{ckey, cid};
    const TopkRow row = scores.row(n);
    if ((int64_t)k > n) k = (int)n;
    ids_out += (int64_t)blockIdx.x * k;
    vals_out += (int64_t)blockIdx.x * k;
    bool done_fast = false;
    int fill_need = 0;        // results still missing after the candidates: the lowest-index -inf scores
    TOPK_STAMP(12);
    if (pre.counts) done_fast = topk_gather_handed_on(s, cand, pre, k, &fill_need);
    TOPK_STAMP(0);
    if (!done_fast && n >= 8192) done_fast = topk_fast_path(s, cand, row, n, k, &fill_need);
    TOPK_STAMP(5);
    if (!done_fast) topk_exact_collect(s, cand, row, n, topk_radix_select(s, cand, row, n, k));
    const int cnt = s.cnt;
    TOPK_STAMP(6);
    topk_rank_and_store(s, cand, cnt, cnt < k ? cnt : k, ids_out, vals_out);
    TOPK_STAMP(7);
    if (fill_need > 0) {
        // phase 6: the remaining results are -inf scores in ascending index order (ordered compaction; stops as soon as enough are found)
        const uint64_t ninf = order_key(-INFINITY);
        take_lowest_indices(n, fill_need, s.scratch, [&](int64_t i) { return order_key(row.at(i)) == ninf; },
                            [&](int j, int64_t i) {
                                ids_out[cnt + j] = (int32_t)i;
                                vals_out[cnt + j] = -INFINITY;
                            });
    }
    TOPK_STAMP(14);
    if (pub.flag) topk_publish(pub);
    TOPK_STAMP(15);
}

}  // namespace
