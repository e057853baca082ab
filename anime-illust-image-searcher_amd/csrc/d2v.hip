// d2v.hip -- Doc2Vec PV-DBOW inference, one wavefront per document.
//
// Replaces gensim Doc2Vec.infer_vector as the reference calls it (genmodel.py:169 for every
// document, webui.py:106,185 per query tag / per reranked document; model built at
// genmodel.py:159 with dm=0, vector_size=300, negative=5, hs=0, sample=1e-3).
// Algorithm restated from gensim 4.3.3 (doc2vec.py::infer_vector, doc2vec_inner.pyx::
// train_document_dbow / fast_document_dbow_neg, word2vec_inner.pyx: 48-bit LCG, EXP_TABLE,
// bisect_left over cum_table).  gensim itself is not available: parity is against
// oracle/csrc/oracle.c, which restates the same algorithm with the same explicit inputs
// (start vector v0, per-document seed -> per-epoch LCG state via splitmix64).
//
// A document is a serial chain of ~epochs*words*(1+negative) dot/axpy steps on one 300-d vector,
// so the parallelism is across documents: the vector lives in 5 VGPRs per lane (element i on lane
// i%64), dot products are 5 fused multiply-adds + a 6-step xor butterfly, control flow is
// wave-uniform.  Bound by dependent-load latency (syn1neg row gather, cum_table search), not by
// HBM or MFMA.
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "common.h"

using namespace hipts;

struct hipts_d2v {
    int device = 0;
    int64_t V = 0;
    int dim = 0, negative = 5;
    double exp_scale = 83.0;
    bool has_sample = false;
    DevBuf syn1neg, syn_lane, cum_table, sample_int, exp_table, word_vectors;      // word_vectors: PV-DM inference only (hipts_d2v_set_word_vectors)
    // syn_lane: the lane-major copy the planned kernel gathers (below)
    DevBuf ws_ptr, ws_words, ws_v0, ws_seeds, ws_out;
};

namespace {

constexpr int EXP_TABLE_SIZE = 1000;
constexpr int MAX_EXP = 6;
constexpr uint64_t LCG_MOD = 281474976710655ULL;   // 2^48 - 1

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

__device__ __forceinline__ uint64_t uniform64(uint64_t x) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// The dot product's cross-lane sum: p[l] + p[l ^ 32], then ^16, ^8, ^4, ^2, ^1 -- the order oracle/csrc/oracle.c::dot_wave64
// defines.  Every stage adds each lane's value and its partner's (a + b on one side, b + a on the other: the same float), so any
// way of fetching the partner gives the same bits; __shfl_xor fetches it through the LDS crossbar (ds_bpermute, ~100 cycles a
// stage with its wait), these forms stay in the vector ALU: v_permlane32_swap / v_permlane16_swap for the two widest stages
// (swap with a copy: one register then holds the lower, the other the upper partner of every pair), DPP for the rest
// (row_ror:8; row_shl:4 | row_shr:4 under bank masks; quad_perm).  ~0.55 -> 0.3 us per step of the serial chain.
__device__ __forceinline__ float wave_sum_butterfly(float p) {
    {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(p), __float_as_uint(p), false, false);
        p = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(p), __float_as_uint(p), false, false);
        p = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    const int pi = __float_as_int(p);
    p = p + __int_as_float(__builtin_amdgcn_update_dpp(pi, pi, 0x128, 0xf, 0xf, false));                 // row_ror:8  = lane ^ 8
    {
        const int qi = __float_as_int(p);
        int t = __builtin_amdgcn_update_dpp(qi, qi, 0x104, 0xf, 0x5, false);                               // row_shl:4: lanes 0-3, 8-11 of a row read lane + 4
        t = __builtin_amdgcn_update_dpp(t, qi, 0x114, 0xf, 0xa, false);                                    // row_shr:4: lanes 4-7, 12-15 read lane - 4
        p = p + __int_as_float(t);
    }
    {
        const int qi = __float_as_int(p);
        p = p + __int_as_float(__builtin_amdgcn_update_dpp(qi, qi, 0x4e, 0xf, 0xf, false));              // quad_perm [2,3,0,1] = lane ^ 2
    }
    {
        const int qi = __float_as_int(p);
        p = p + __int_as_float(__builtin_amdgcn_update_dpp(qi, qi, 0xb1, 0xf, 0xf, false));              // quad_perm [1,0,3,2] = lane ^ 1
    }
    return p;
}

// bisect_left(a, x, 0, n): smallest i with a[i] >= x.  64-ary search: each lane probes the last
// element of its chunk, the ballot tells which chunk holds the answer (3 rounds for n = 10k).
__device__ __forceinline__ uint32_t bisect_left_wave(const uint32_t* __restrict__ a, uint32_t x, uint32_t n, int lane) {
    uint32_t lo = 0;
    while (n > 0) {
        const uint32_t step = (n + 63) >> 6;
        uint32_t idx = lo + (uint32_t)(lane + 1) * step - 1;
        const uint32_t last = lo + n - 1;
        idx = idx < last ? idx : last;
        const bool below = a[idx] < x;
        const uint64_t mask = __ballot(below);
        const uint32_t c = (uint32_t)__popcll(mask);
        if (c == 64) return lo + n;
        const uint32_t nlo = lo + c * step;
        uint32_t chunk_last = nlo + step - 1;
        chunk_last = chunk_last < last ? chunk_last : last;
        lo = nlo;
        n = chunk_last - nlo;     // a[chunk_last] >= x is known
    }
    return lo;
}

// ---------------------------------------------------------------------------------------------
// What every kernel below must compute alike, bit for bit with oracle/csrc/oracle.c, stated once.
// ---------------------------------------------------------------------------------------------
// Kernel arguments of the three walking kernels (the planned kernel keeps plain parameters, see there).  Pointers inside a struct are
// not __restrict__: the helpers below take the rows they touch as __restrict__ parameters.
struct Model {
    float* syn;                     // syn1neg [V][dim]; the planned kernel is handed the lane-major copy; only training writes it
    const uint32_t* cum_table;
    const uint32_t* sample_int;     // nullptr: no sub-sampling
    const float* exp_table;         // EXP_TABLE_SIZE floats, copied to LDS by every workgroup
    int64_t V;
    int dim, negative;
    double exp_scale;
};
struct Docs {                       // inference: CSR of word ids, start vector and seed per document, the result
    const int64_t* doc_ptr;
    const int32_t* words;
    int64_t ndocs;
    const float* v0;
    const uint64_t* seeds;
    float* out;
};
struct Schedule {
    int epochs;
    float alpha0, min_alpha;
};

// word2vec_inner.pyx's 48-bit LCG.  A draw is the state's upper 32 bits; every draw advances the state once.
__device__ __forceinline__ void lcg_next(uint64_t& state) { state = (state * 25214903917ULL + 11) & LCG_MOD; }
__device__ __forceinline__ uint64_t lcg_draw(uint64_t& state) {
    const uint64_t r = state >> 16;
    lcg_next(state);
    return r;
}
// the state a document starts epoch (or training pass) k with, wave-uniform
__device__ __forceinline__ uint64_t epoch_lcg(uint64_t seed, uint64_t k) { return uniform64(splitmix64(seed + k) & LCG_MOD); }

// infer_vector's alpha: alpha0 in the first epoch, then one double subtraction of (alpha0 - min_alpha) / max(epochs - 1, 1) per epoch
struct InferAlpha {
    double alpha, delta;
    __device__ explicit InferAlpha(const Schedule& s)
        : alpha((double)s.alpha0), delta(((double)s.alpha0 - (double)s.min_alpha) / (double)(s.epochs - 1 > 1 ? s.epochs - 1 : 1)) {}
    __device__ float next() {
        const float a = (float)alpha;
        alpha -= delta;
        return a;
    }
};

// Sub-sampling: one draw per in-vocabulary word, the word stays unless its threshold is below the draw.  Callers guard with
// `sample_int != nullptr`: without sub-sampling nothing is drawn.
__device__ __forceinline__ bool subsample_keeps(uint32_t threshold, uint64_t& state) { return !((uint64_t)threshold < lcg_draw(state)); }

// A vector in registers: the lane owns elements lane, lane + 64, ... of a row of `dim` floats, zero past the end.  (One address per
// row, `row + lane`, and constant offsets from it.)
template <int EPL>
__device__ __forceinline__ void load_vec(float (&x)[EPL], const float* __restrict__ row, int dim, int lane) {
    row += lane;
#pragma unroll
    for (int c = 0; c < EPL; ++c) x[c] = (lane + 64 * c < dim) ? row[64 * c] : 0.0f;
}
template <int EPL>
__device__ __forceinline__ void store_vec(float* __restrict__ row, const float (&x)[EPL], int dim, int lane) {
    row += lane;
#pragma unroll
    for (int c = 0; c < EPL; ++c)
        if (lane + 64 * c < dim) row[64 * c] = x[c];
}
template <int EPL>
__device__ __forceinline__ void atomic_add_vec(float* __restrict__ row, const float (&x)[EPL], int dim, int lane) {
    row += lane;
#pragma unroll
    for (int c = 0; c < EPL; ++c)
        if (lane + 64 * c < dim) unsafeAtomicAdd(&row[64 * c], x[c]);
}

// (the caller's __syncthreads() follows; `threads` is the workgroup size, a constant wherever the launch fixes it)
__device__ __forceinline__ void load_exp_table(float* lds, const float* __restrict__ table, int threads) {
    for (int i = threadIdx.x; i < EXP_TABLE_SIZE; i += threads) lds[i] = table[i];
}

// g = (label - sigmoid(f)) * a through EXP_TABLE; false (and no step) outside (-MAX_EXP, MAX_EXP).  The index is word2vec_inner.pyx's:
// float add, widened to double, times exp_scale, truncated.  (The planned kernel takes the window test and the index apart: it looks
// the whole group of a word up before it branches.)
__device__ __forceinline__ bool sigmoid_in_window(float f) { return !(f <= -(float)MAX_EXP || f >= (float)MAX_EXP); }
__device__ __forceinline__ int sigmoid_index(float f, double exp_scale) { return (int)((double)(f + (float)MAX_EXP) * exp_scale); }
__device__ __forceinline__ bool sigmoid_grad(float f, float label, float a, const float* exp_table, double exp_scale, float& g) {
    if (!sigmoid_in_window(f)) return false;
    g = (label - exp_table[sigmoid_index(f, exp_scale)]) * a;
    return true;
}

// The (1 + negative) targets of one word w against the input vector `in` (the document vector; PV-DM: the context mean / sum): the word
// itself with label 1, then `negative` draws from cum_table with label 0.  The draw order is the oracle's contract: one draw per negative
// sample, advanced BEFORE the sample that hit the word itself is skipped.  work = sum of g * syn1neg[target] in target order.
// Hidden: what happens to syn1neg[target] -- nothing (inference), += g * in by a plain store (sequential training; the row was just read,
// so it is fmaf(g, in, row)) or by float atomics (parallel training: concurrent documents lose no update).
enum class Hidden { none, store, atomic };

template <int EPL, Hidden H>
__device__ __forceinline__ void ns_word_step(const float (&in)[EPL], int32_t w, uint64_t& state, const Model& m, uint32_t cum_last, float a,
                                             const float* exp_table, int lane, float (&work)[EPL]) {
    float rw[EPL];
#pragma unroll
    for (int c = 0; c < EPL; ++c) work[c] = 0.0f;
    for (int d = 0; d < m.negative + 1; ++d) {
        uint32_t target = (uint32_t)w;
        if (d > 0) {
            const uint32_t x = (uint32_t)lcg_draw(state) % cum_last;
            target = __builtin_amdgcn_readfirstlane(bisect_left_wave(m.cum_table, x, (uint32_t)m.V, lane));
            if (target == (uint32_t)w) continue;
        }
        float* row = m.syn + (int64_t)target * m.dim;
        load_vec<EPL>(rw, row, m.dim, lane);
        float p = 0.0f;
#pragma unroll
        for (int c = 0; c < EPL; ++c) p = fmaf(in[c], rw[c], p);
        float g;
        if (!sigmoid_grad(wave_sum_butterfly(p), d == 0 ? 1.0f : 0.0f, a, exp_table, m.exp_scale, g)) continue;
#pragma unroll
        for (int c = 0; c < EPL; ++c) {
            work[c] = fmaf(g, rw[c], work[c]);
            if (H == Hidden::store) rw[c] = fmaf(g, in[c], rw[c]);
            if (H == Hidden::atomic) rw[c] = g * in[c];
        }
        if (H == Hidden::store) store_vec<EPL>(row, rw, m.dim, lane);
        if (H == Hidden::atomic) atomic_add_vec<EPL>(row, rw, m.dim, lane);
    }
}

template <int EPL>
__global__ __launch_bounds__(256) void d2v_infer_kernel(Model m, Docs docs, Schedule sched) {
    __shared__ float exp_table[EXP_TABLE_SIZE];
    load_exp_table(exp_table, m.exp_table, 256);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t doc = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (doc >= docs.ndocs) return;                  // whole wave exits together
    float v[EPL], work[EPL];
    load_vec<EPL>(v, docs.v0 + doc * m.dim, m.dim, lane);
    const int64_t wb = docs.doc_ptr[doc], we = docs.doc_ptr[doc + 1];
    const uint64_t seed = docs.seeds[doc];
    const uint32_t cum_last = m.cum_table[m.V - 1];
    InferAlpha alpha(sched);
    for (int e = 0; e < sched.epochs; ++e) {
        uint64_t next_random = epoch_lcg(seed, (uint64_t)e);
        const float a = alpha.next();
        for (int64_t i = wb; i < we; ++i) {
            const int32_t w = __builtin_amdgcn_readfirstlane(docs.words[i]);
            if (w < 0 || w >= m.V) continue;
            if (m.sample_int && !subsample_keeps(m.sample_int[w], next_random)) continue;
            ns_word_step<EPL, Hidden::none>(v, w, next_random, m, cum_last, a, exp_table, lane, work);
#pragma unroll
            for (int c = 0; c < EPL; ++c) v[c] = v[c] + work[c];
        }
    }
    store_vec<EPL>(docs.out + doc * m.dim, v, m.dim, lane);
}

// ---------------------------------------------------------------------------------------------
// PV-DM inference (dm = 1, sum or mean; BASELINE.json's north_star names it, the reference runs dm = 0): gensim's
// train_document_dm with frozen word vectors and hidden layer -- oracle/csrc/oracle.c::orc_d2v_infer_dm is the restatement this
// follows operation for operation.  A wave per document as d2v_infer_kernel; per epoch the kept words (in vocabulary, surviving
// sub-sampling) and their reduced windows go into the wave's LDS lists (written by lane 0 from the scalar LCG walk), then every
// kept position builds l1 = (context word vectors, ascending position, + the document vector) [* 1 / count] and runs the
// (1 + negative) targets against it.  The same lane owns element lane + 64 c of every vector, so sums and the dot product have
// the oracle's order.
// ---------------------------------------------------------------------------------------------
constexpr int DM_CAP = 512;        // kept words of one document (host-checked against the raw length)

template <int EPL>
__global__ __launch_bounds__(256) void d2v_infer_dm_kernel(Model m, const float* __restrict__ wv, Docs docs, Schedule sched, int window, int dm_mean) {
    __shared__ float exp_table[EXP_TABLE_SIZE];
    __shared__ int32_t s_kept[4][DM_CAP];
    __shared__ int32_t s_red[4][DM_CAP];
    load_exp_table(exp_table, m.exp_table, 256);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t doc = (int64_t)blockIdx.x * 4 + wid;
    if (doc >= docs.ndocs) return;                  // whole wave exits together
    int32_t* kept = s_kept[wid];
    int32_t* red = s_red[wid];
    float v[EPL], work[EPL], rw[EPL], l1[EPL];
    load_vec<EPL>(v, docs.v0 + doc * m.dim, m.dim, lane);
    const int64_t wb = docs.doc_ptr[doc], we = docs.doc_ptr[doc + 1];
    const uint64_t seed = docs.seeds[doc];
    const uint32_t cum_last = m.cum_table[m.V - 1];
    InferAlpha alpha(sched);
    for (int e = 0; e < sched.epochs; ++e) {
        uint64_t next_random = epoch_lcg(seed, (uint64_t)e);
        const float a = alpha.next();
        int n = 0;
        for (int64_t i = wb; i < we; ++i) {
            const int32_t w = __builtin_amdgcn_readfirstlane(docs.words[i]);
            if (w < 0 || w >= m.V) continue;
            if (m.sample_int && !subsample_keeps(m.sample_int[w], next_random)) continue;
            if (lane == 0) kept[n] = w;
            ++n;
        }
        for (int i = 0; i < n; ++i) {
            const uint32_t b = (uint32_t)lcg_draw(next_random) % (uint32_t)window;
            if (lane == 0) red[i] = (int32_t)b;
        }
        // lane 0's LDS writes are read by every lane of this wave below: LDS operations of one wave execute in order, the fence
        // only keeps the compiler from moving them
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int i = 0; i < n; ++i) {
            const int b = __builtin_amdgcn_readfirstlane(red[i]);
            int j = i - window + b, k = i + window + 1 - b;
            j = j < 0 ? 0 : j;
            k = k > n ? n : k;
#pragma unroll
            for (int c = 0; c < EPL; ++c) l1[c] = 0.0f;
            float count = 0.0f;
            for (int mm = j; mm < k; ++mm) {
                if (mm == i) continue;
                count += 1.0f;
                const int32_t wm = __builtin_amdgcn_readfirstlane(kept[mm]);
                load_vec<EPL>(rw, wv + (int64_t)wm * m.dim, m.dim, lane);
#pragma unroll
                for (int c = 0; c < EPL; ++c) l1[c] = l1[c] + rw[c];
            }
            count += 1.0f;                                  // the document tag
#pragma unroll
            for (int c = 0; c < EPL; ++c) l1[c] = l1[c] + v[c];
            const float inv_count = 1.0f / count;
            if (dm_mean) {
#pragma unroll
                for (int c = 0; c < EPL; ++c) l1[c] = l1[c] * inv_count;
            }
            const int32_t w = __builtin_amdgcn_readfirstlane(kept[i]);
            ns_word_step<EPL, Hidden::none>(l1, w, next_random, m, cum_last, a, exp_table, lane, work);
            if (!dm_mean) {
#pragma unroll
                for (int c = 0; c < EPL; ++c) work[c] = work[c] * inv_count;
            }
#pragma unroll
            for (int c = 0; c < EPL; ++c) v[c] = v[c] + work[c];
        }
        // the next epoch's list writes must not overtake this epoch's list reads (same wave, in order; compiler fence only)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    store_vec<EPL>(docs.out + doc * m.dim, v, m.dim, lane);
}

// ---------------------------------------------------------------------------------------------
// Planned inference (default).  d2v_infer_kernel above pays, per dot/axpy step, a 64-ary search of cum_table (three dependent
// rounds of loads) and a dependent gather of the target row: ~2 us per step, ~30 ms for one document of 100 epochs -- the
// latency of find_similar_documents' rerank (webui.py:198-199: ten documents re-inferred per query).  But the random stream does
// not depend on the vector being trained: which words survive sub-sampling and which rows the negative samples hit follows
// from the LCG alone.  So per epoch and chunk of words a wave
//   1. walks the LCG (uniform, scalar): one entry per positive target, one raw draw per negative sample, into LDS;
//   2. resolves all draws of the chunk AT ONCE, a lane per draw: modulo, bisect_left over cum_table (its first levels from a
//      1024-entry coarse table in LDS), drops the samples that hit their own word, compacts;
//   3. runs the serial chain over the compacted plan a WORD at a time: the (1 + negative) dot products of a word are
//      independent (the vector changes only after the word), the next word's rows are already requested.
// The arithmetic of a step and its order are those of d2v_infer_kernel: results are bit-identical (same tests).
// ---------------------------------------------------------------------------------------------
constexpr int PLAN_WORDS = 32;            // words per chunk
constexpr int PLAN_MAX_NEG = 5;             // a word's group: 1 positive + up to 5 negative samples (gensim's default negative = 5)
constexpr int PLAN_GROUP = 1 + PLAN_MAX_NEG;
constexpr int PLAN_CAP = PLAN_WORDS * (1 + PLAN_MAX_NEG);     // 32 x 6 = 192 plan entries per wave
constexpr int PLAN_COARSE = 1024;
constexpr uint32_t PLAN_POS = 0x80000000u;

__device__ __forceinline__ uint32_t bisect_left_coarse(const uint32_t* __restrict__ a, const uint32_t* coarse, uint32_t x, uint32_t n, uint32_t stride) {
    // coarse[c] = a[min((c + 1) * stride, n) - 1]: the last element of block c.  Smallest block whose last element is >= x, then
    // the smallest element >= x inside it: exactly bisect_left (a is non-decreasing); x above every element returns n.
    const uint32_t nblk = (n + stride - 1) / stride;
    uint32_t lo = 0, hi = nblk;
    while (hi > lo) {
        const uint32_t mid = (lo + hi) >> 1;
        if (coarse[mid] >= x) hi = mid;
        else lo = mid + 1;
    }
    if (lo == nblk) return n;
    uint32_t b = lo * stride, e = b + stride < n ? b + stride : n;
    while (e > b) {
        const uint32_t mid = (b + e) >> 1;
        if (a[mid] >= x) e = mid;
        else b = mid + 1;
    }
    return b;
}

// Lane-major copy of syn1neg for the planned kernel.  A lane owns elements lane, lane + 64, ... of a row (that is what fixes the bits
// of the dot product), so in the row-major matrix its EPL values are 256 B apart: EPL global_load_dword per row and lane, 30 vector-
// memory instructions per word at negative = 5 -- and the wave's time went into ISSUING them (~50-75 cycles each).  Here a row is
// stored as [64 lanes][4] blocks for c = 0..3, 4..7, ... followed by one [64][tw] block for the remaining EPL % 4 values (tw = 1, 2,
// or 4 with padding for 3): the same values in the same registers from EPL / 4 dwordx4 loads plus at most one more (300-d: 2 loads
// per row instead of 5, 1 280 B per row).
__host__ __device__ inline int lane_tail_width(int epl) { return (epl & 3) == 3 ? 4 : (epl & 3); }
__host__ __device__ inline int lane_row_floats(int epl) { return 64 * (4 * (epl >> 2) + lane_tail_width(epl)); }

__global__ __launch_bounds__(256) void d2v_lane_major_kernel(const float* __restrict__ syn1neg, float* __restrict__ out, int64_t V, int dim, int epl) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= V) return;
    const int n4 = epl >> 2, tw = lane_tail_width(epl);
    float* __restrict__ row = out + w * lane_row_floats(epl);
    const float* __restrict__ src = syn1neg + w * dim;
    for (int q = 0; q < n4; ++q)
        for (int i = 0; i < 4; ++i) {
            const int e = lane + 64 * (4 * q + i);
            row[(q * 64 + lane) * 4 + i] = e < dim ? src[e] : 0.0f;
        }
    for (int i = 0; i < tw; ++i) {
        const int e = lane + 64 * (4 * n4 + i);
        row[n4 * 256 + lane * tw + i] = (4 * n4 + i < epl && e < dim) ? src[e] : 0.0f;
    }
}

template <int EPL>
__global__ __launch_bounds__(256) void d2v_infer_plan_kernel(const float* __restrict__ syn1neg, const uint32_t* __restrict__ cum_table,
                                                             const uint32_t* __restrict__ sample_int, int64_t V, int dim,
                                                             const int64_t* __restrict__ doc_ptr, const int32_t* __restrict__ words,
                                                             int64_t ndocs, const float* __restrict__ v0, const uint64_t* __restrict__ seeds,
                                                             int epochs, float alpha0, float min_alpha, int negative, double exp_scale,
                                                             const float* __restrict__ exp_table_g, float* __restrict__ out) {
    // This kernel is held to its measured instruction stream.  Plain parameters, not Model / Docs / Schedule: with the structs it (and
    // only it) needed 4-6 VGPRs more and lost a wave of occupancy at 2 elements per lane.  Its start-vector load, result store and alpha
    // schedule are written out instead of load_vec / store_vec / InferAlpha: with those the prologue was four instructions longer and a
    // 100-epoch document took 4 % longer (LABNOTES).  syn1neg is the LANE-MAJOR copy (d2v_lane_major_kernel).
    __shared__ float exp_table[EXP_TABLE_SIZE];
    __shared__ uint32_t coarse[PLAN_COARSE];
    __shared__ uint32_t plan_raw[4][PLAN_CAP], plan_own[4][PLAN_CAP], plan[4][PLAN_CAP];
    __shared__ int32_t cw[4][PLAN_WORDS];
    __shared__ uint32_t csi[4][PLAN_WORDS];
    const uint32_t stride = (uint32_t)((V + PLAN_COARSE - 1) / PLAN_COARSE);
    load_exp_table(exp_table, exp_table_g, 256);
    for (uint32_t c = threadIdx.x; c * stride < (uint32_t)V; c += 256) {
        const uint32_t last = (c + 1) * stride < (uint32_t)V ? (c + 1) * stride : (uint32_t)V;
        coarse[c] = cum_table[last - 1];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t doc = (int64_t)blockIdx.x * 4 + wv;
    if (doc >= ndocs) return;                       // whole wave exits together (no barrier below)
    float v[EPL];
#pragma unroll
    for (int c = 0; c < EPL; ++c) v[c] = (lane + 64 * c < dim) ? v0[doc * dim + lane + 64 * c] : 0.0f;
    const int64_t wb = doc_ptr[doc], we = doc_ptr[doc + 1];
    const uint64_t seed = seeds[doc];
    const uint32_t cum_last = cum_table[V - 1];
    double alpha = (double)alpha0;
    const double alpha_delta = ((double)alpha0 - (double)min_alpha) / (double)(epochs - 1 > 1 ? epochs - 1 : 1);
    uint32_t* praw = plan_raw[wv];
    uint32_t* pown = plan_own[wv];
    uint32_t* pl = plan[wv];
    constexpr int N4 = EPL >> 2, TW = (EPL & 3) == 3 ? 4 : (EPL & 3), ROWF = 64 * (4 * N4 + TW);
    auto load_row = [&](uint32_t e, float (&rw)[EPL]) {
        const float* __restrict__ row = syn1neg + (int64_t)(e & ~PLAN_POS) * ROWF;
#pragma unroll
        for (int q = 0; q < N4; ++q) {
            const float4 x = *reinterpret_cast<const float4*>(row + (q * 64 + lane) * 4);
            rw[4 * q] = x.x; rw[4 * q + 1] = x.y; rw[4 * q + 2] = x.z; rw[4 * q + 3] = x.w;
        }
        if constexpr (TW == 1) {
            rw[4 * N4] = row[N4 * 256 + lane];
        } else if constexpr (TW == 2) {
            const float2 x = *reinterpret_cast<const float2*>(row + N4 * 256 + lane * 2);
            rw[4 * N4] = x.x; rw[4 * N4 + 1] = x.y;
        } else if constexpr (TW == 4) {
            const float4 x = *reinterpret_cast<const float4*>(row + N4 * 256 + lane * 4);
            rw[4 * N4] = x.x; rw[4 * N4 + 1] = x.y; rw[4 * N4 + 2] = x.z;
        }
    };
    for (int e = 0; e < epochs; ++e) {
        uint64_t next_random = epoch_lcg(seed, (uint64_t)e);
        const float a = (float)alpha;
        for (int64_t c0 = wb; c0 < we; c0 += PLAN_WORDS) {
            const int nc = (int)(we - c0 < PLAN_WORDS ? we - c0 : PLAN_WORDS);
            // the chunk's words and their sub-sampling thresholds: one coalesced load, then uniform reads from LDS
            if (lane < nc) {
                const int32_t w = words[c0 + lane];
                cw[wv][lane] = w;
                csi[wv][lane] = (sample_int && w >= 0 && w < V) ? sample_int[w] : 0xffffffffu;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // wave-level LDS fence: the phases hand data from lane to lane
            // ---- 1. the random walk (uniform)
            int n = 0;
            for (int i = 0; i < nc; ++i) {
                const int32_t w = __builtin_amdgcn_readfirstlane(cw[wv][i]);
                if (w < 0 || w >= V) continue;
                if (sample_int && !subsample_keeps((uint32_t)__builtin_amdgcn_readfirstlane(csi[wv][i]), next_random)) continue;
                if (lane == 0) {
                    praw[n] = (uint32_t)w;
                    pown[n] = 0xffffffffu;          // marks a positive target (a raw draw may have any of its 32 bits set)
                }
                for (int d = 1; d <= negative; ++d) {
                    const uint32_t r = (uint32_t)lcg_draw(next_random);
                    if (lane == 0) {
                        praw[n + d] = r;
                        pown[n + d] = (uint32_t)w;
                    }
                }
                n += 1 + negative;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // wave-level LDS fence: the phases hand data from lane to lane
            // ---- 2. resolve every draw of the chunk, a lane per entry; drop samples that hit their own word; compact in order
            int m = 0;
            for (int j0 = 0; j0 < n; j0 += 64) {
                const int j = j0 + lane;
                uint32_t entry = 0;
                bool keep = false;
                if (j < n) {
                    const uint32_t r = praw[j], own = pown[j];
                    if (own == 0xffffffffu) {
                        entry = PLAN_POS | r;
                        keep = true;
                    } else {
                        const uint32_t t = bisect_left_coarse(cum_table, coarse, r % cum_last, (uint32_t)V, stride);
                        entry = t;
                        keep = t != own;
                    }
                }
                const uint64_t mask = __ballot(keep);
                if (keep) pl[m + __popcll(mask & ((1ull << lane) - 1))] = entry;
                m += __popcll(mask);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // wave-level LDS fence: the phases hand data from lane to lane
            // ---- 3. the serial chain, a WORD at a time.  The (1 + negative) dot products of a word all use the document vector as it
            // stood before the word (v changes only after it), so they are independent: their rows are requested together, the dots,
            // the cross-lane sums and the sigmoid look-ups of the group overlap in the pipeline, and only the accumulation of `work`
            // keeps the reference's order.  The next word's rows are requested before this word is computed.
            if (m == 0) continue;
            constexpr int G = PLAN_GROUP;
            auto read_group = [&](int j, uint32_t (&ge)[G], int& gs) {
                const uint32_t x = (lane <= G && j + lane < m) ? pl[j + lane] : PLAN_POS;      // past the end counts as "next word"
                const uint64_t rest = __ballot((x & PLAN_POS) != 0) >> 1;                       // entry j itself is a positive target
                const int nxt = rest ? (int)__ffsll((unsigned long long)rest) : G;
                gs = nxt < G ? nxt : G;
#pragma unroll
                for (int g = 0; g < G; ++g) ge[g] = (uint32_t)__builtin_amdgcn_readlane((int)x, g);
            };
            auto load_rows = [&](const uint32_t (&ge)[G], int gs, float (&R)[G][EPL]) {
#pragma unroll
                for (int g = 0; g < G; ++g)
                    if (g < gs) load_row(ge[g], R[g]);
            };
            auto process = [&](int gs, const float (&R)[G][EPL]) {
                float p[G];
#pragma unroll
                for (int g = 0; g < G; ++g) p[g] = 0.0f;
#pragma unroll
                for (int c = 0; c < EPL; ++c)
#pragma unroll
                    for (int g = 0; g < G; ++g)
                        if (g < gs) p[g] = fmaf(v[c], R[g][c], p[g]);
                float tv[G];
                bool ok[G];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const float f = g < gs ? wave_sum_butterfly(p[g]) : 0.0f;
                    ok[g] = g < gs && sigmoid_in_window(f);
                    tv[g] = exp_table[ok[g] ? sigmoid_index(f, exp_scale) : 0];
                }
                float wk[EPL];
#pragma unroll
                for (int c = 0; c < EPL; ++c) wk[c] = 0.0f;
#pragma unroll
                for (int g = 0; g < G; ++g)
                    if (ok[g]) {
                        const float gg = ((g == 0 ? 1.0f : 0.0f) - tv[g]) * a;
#pragma unroll
                        for (int c = 0; c < EPL; ++c) wk[c] = fmaf(gg, R[g][c], wk[c]);
                    }
#pragma unroll
                for (int c = 0; c < EPL; ++c) v[c] = v[c] + wk[c];
            };
            uint32_t ea[G], eb[G];
            int ga = 0, gb = 0;
            float Ra[G][EPL], Rb[G][EPL];
            int j = 0;
            read_group(0, ea, ga);
            load_rows(ea, ga, Ra);
            for (;;) {
                int jn = j + ga;
                bool more = jn < m;
                if (more) {
                    read_group(jn, eb, gb);
                    load_rows(eb, gb, Rb);
                }
                process(ga, Ra);
                if (!more) break;
                j = jn;
                jn = j + gb;
                more = jn < m;
                if (more) {
                    read_group(jn, ea, ga);
                    load_rows(ea, ga, Ra);
                }
                process(gb, Rb);
                if (!more) break;
                j = jn;
            }
        }
        alpha -= alpha_delta;
    }
#pragma unroll
    for (int c = 0; c < EPL; ++c)
        if (lane + 64 * c < dim) out[doc * dim + lane + 64 * c] = v[c];
}

// ---------------------------------------------------------------------------------------------
// Training (genmodel.py:159-162: Doc2Vec(vector_size=300, window=50, min_count=1, workers=1, dm=0), build_vocab, train(epochs=100)).
// One document's pass = the inference step above PLUS the hidden-layer update syn1neg[target] += g * doc_vector
// (doc2vec_inner.pyx::fast_document_dbow_neg with learn_hidden = 1), the document vector updated in place in the table.
// A job's alpha (word2vec.py::_get_next_alpha): alpha0 - (alpha0 - min_alpha) * (epoch + first_doc_of_job / ndocs) / epochs.
//   SEQUENTIAL (mode 0)  one wavefront walks every document of every epoch in corpus order -- the reference's workers=1
//                        semantics; bit-identical to oracle/csrc/oracle.c::orc_d2v_train.  For small corpora and parity.
//   PARALLEL (mode 1)    a wavefront per document, the corpus in chunks of HIPTS_D2V_CHUNK (default 2048) documents per launch:
//                        documents of a chunk train concurrently against the hidden layer as the chunks before left it, their
//                        own updates of it are float atomic adds (gensim's worker threads race with plain stores, which works
//                        while collisions are rare; with thousands of concurrent documents on a 10 k-word vocabulary plain
//                        stores lose nearly every update -- measured: neighbour purity at chance).  Not reproducible run to
//                        run; its quality is judged downstream (tests/test_gpu_d2v_train.py).
// ---------------------------------------------------------------------------------------------
template <int EPL, Hidden H>
__device__ __forceinline__ void train_document(const Model& m, const int32_t* __restrict__ words, int64_t wb, int64_t we, float* __restrict__ vrow,
                                               uint64_t next_random, float a, const float* exp_table, uint32_t cum_last, int lane) {
    float v[EPL], work[EPL];
    load_vec<EPL>(v, vrow, m.dim, lane);
    for (int64_t i = wb; i < we; ++i) {
        const int32_t w = __builtin_amdgcn_readfirstlane(words[i]);
        if (w < 0 || w >= m.V) continue;
        if (m.sample_int && !subsample_keeps(m.sample_int[w], next_random)) continue;
        ns_word_step<EPL, H>(v, w, next_random, m, cum_last, a, exp_table, lane, work);
#pragma unroll
        for (int c = 0; c < EPL; ++c) v[c] = v[c] + work[c];
    }
    store_vec<EPL>(vrow, v, m.dim, lane);
}

__device__ __forceinline__ float job_alpha(int epoch, int64_t job_first, int64_t ndocs, const Schedule& s) {
    const double progress = ((double)epoch + (double)job_first / (double)ndocs) / (double)s.epochs;
    double al = (double)s.alpha0 - ((double)s.alpha0 - (double)s.min_alpha) * progress;
    if (al < (double)s.min_alpha) al = (double)s.min_alpha;
    return (float)al;
}

// mode 1: grid over documents [doc0, doc1) of ONE epoch.  mode 0: one wavefront (grid 1, 64 threads), epochs [epoch0, epoch1).
template <int EPL, bool SEQUENTIAL>
__global__ __launch_bounds__(256) void d2v_train_kernel(Model m, Schedule sched, const int64_t* __restrict__ doc_ptr, const int32_t* __restrict__ words,
                                                        const int64_t* __restrict__ job_first, int64_t ndocs, float* __restrict__ doc_vectors,
                                                        uint64_t seed, int epoch0, int epoch1, int64_t doc0, int64_t doc1) {
    __shared__ float exp_table[EXP_TABLE_SIZE];
    load_exp_table(exp_table, m.exp_table, blockDim.x);      // 64 threads sequential, 256 parallel
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t cum_last = m.cum_table[m.V - 1];
    if (SEQUENTIAL) {
        if (blockIdx.x != 0 || threadIdx.x >= 64) return;
        for (int e = epoch0; e < epoch1; ++e)
            for (int64_t doc = 0; doc < ndocs; ++doc)
                train_document<EPL, Hidden::store>(m, words, doc_ptr[doc], doc_ptr[doc + 1], doc_vectors + doc * m.dim,
                                                   epoch_lcg(seed, (uint64_t)e * (uint64_t)ndocs + (uint64_t)doc),
                                                   job_alpha(e, job_first[doc], ndocs, sched), exp_table, cum_last, lane);
    } else {
        const int64_t doc = doc0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
        if (doc >= doc1) return;
        train_document<EPL, Hidden::atomic>(m, words, doc_ptr[doc], doc_ptr[doc + 1], doc_vectors + doc * m.dim,
                                            epoch_lcg(seed, (uint64_t)epoch0 * (uint64_t)ndocs + (uint64_t)doc),
                                            job_alpha(epoch0, job_first[doc], ndocs, sched), exp_table, cum_last, lane);
    }
}

// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------
// word2vec_inner.pyx: EXP_TABLE[i] = exp((i / 1000 * 2 - 1) * 6); EXP_TABLE[i] /= (EXP_TABLE[i] + 1)   (REAL_t)
void exp_table_host(float (&table)[EXP_TABLE_SIZE]) {
    for (int i = 0; i < EXP_TABLE_SIZE; ++i) {
        const float e = (float)exp((i / (float)EXP_TABLE_SIZE * 2 - 1) * MAX_EXP);
        table[i] = (float)(e / (e + 1));
    }
}

// The kernels are instantiated for 1 .. 8 elements per lane (dim <= 512): f(std::integral_constant<int, EPL>).
template <typename F>
void dispatch_epl(int epl, F f) {
    switch (epl) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        default: return f(std::integral_constant<int, 8>{});
    }
}

Model model_of(const hipts_d2v* h, const DevBuf& syn) {
    return Model{syn.as<float>(), h->cum_table.as<uint32_t>(), h->has_sample ? h->sample_int.as<uint32_t>() : nullptr,
                 h->exp_table.as<float>(), h->V, h->dim, h->negative, h->exp_scale};
}

// Inference input into the handle's staging buffers (enqueued on s); the result goes to `out` itself when that is device memory.
int stage_documents(hipts_d2v* h, const int64_t* doc_ptr, const int32_t* words, int64_t ndocs, const float* v0, const uint64_t* seeds,
                    float* out, int out_memspace, hipStream_t s, Docs* docs) {
    const int64_t nw = doc_ptr[ndocs];
    HIPTS_TRY(h->ws_ptr.reserve((size_t)(ndocs + 1) * 8));
    HIPTS_TRY(h->ws_words.reserve((size_t)(nw ? nw : 1) * 4));
    HIPTS_TRY(h->ws_v0.reserve((size_t)ndocs * h->dim * 4));
    HIPTS_TRY(h->ws_seeds.reserve((size_t)ndocs * 8));
    HIPTS_HIP(hipMemcpyAsync(h->ws_ptr.p, doc_ptr, (size_t)(ndocs + 1) * 8, hipMemcpyHostToDevice, s));
    if (nw) HIPTS_HIP(hipMemcpyAsync(h->ws_words.p, words, (size_t)nw * 4, hipMemcpyHostToDevice, s));
    HIPTS_HIP(hipMemcpyAsync(h->ws_v0.p, v0, (size_t)ndocs * h->dim * 4, hipMemcpyHostToDevice, s));
    HIPTS_HIP(hipMemcpyAsync(h->ws_seeds.p, seeds, (size_t)ndocs * 8, hipMemcpyHostToDevice, s));
    float* out_dev = out;
    if (out_memspace != HIPTS_DEVICE) {
        HIPTS_TRY(h->ws_out.reserve((size_t)ndocs * h->dim * 4));
        out_dev = h->ws_out.as<float>();
    }
    *docs = Docs{h->ws_ptr.as<int64_t>(), h->ws_words.as<int32_t>(), ndocs, h->ws_v0.as<float>(), h->ws_seeds.as<uint64_t>(), out_dev};
    return HIPTS_OK;
}

int finish_documents(hipts_d2v* h, const Docs& docs, float* out, int out_memspace, hipStream_t s) {
    HIPTS_LAUNCH_CHECK();
    if (out_memspace != HIPTS_DEVICE) HIPTS_HIP(hipMemcpyAsync(out, docs.out, (size_t)docs.ndocs * h->dim * 4, hipMemcpyDeviceToHost, s));
    HIPTS_HIP(hipStreamSynchronize(s));   // staging buffers are reused by the next call
    return HIPTS_OK;
}

}  // namespace

extern "C" {

int hipts_d2v_create(const float* syn1neg, const uint32_t* cum_table, const uint32_t* sample_int, int64_t vocab, int dim,
                     int negative, double exp_scale, int device, hipts_d2v_t** out) {
    HIPTS_REQUIRE(syn1neg && cum_table && out && vocab >= 1 && vocab < (1ll << 31), "hipts_d2v_create: bad arguments");
    HIPTS_REQUIRE(dim >= 1 && dim <= 512, "hipts_d2v_create: dim must be in [1, 512]");
    HIPTS_REQUIRE(negative >= 0 && negative <= 64, "hipts_d2v_create: negative out of range");
    HIPTS_REQUIRE(cum_table[vocab - 1] > 0, "hipts_d2v_create: cum_table[-1] must be positive");
    HIPTS_TRY(use_device(device));
    auto* h = new hipts_d2v();
    h->device = device;
    h->V = vocab;
    h->dim = dim;
    h->negative = negative;
    h->exp_scale = exp_scale;
    h->has_sample = sample_int != nullptr;
    float table[EXP_TABLE_SIZE];
    exp_table_host(table);
    int st;
    if ((st = h->syn1neg.alloc((size_t)vocab * dim * 4)) || (st = h->cum_table.alloc((size_t)vocab * 4)) ||
        (st = h->exp_table.alloc(sizeof(table))) || (st = upload(h->syn1neg.p, syn1neg, (size_t)vocab * dim * 4)) ||
        (st = upload(h->cum_table.p, cum_table, (size_t)vocab * 4)) || (st = upload(h->exp_table.p, table, sizeof(table))) ||
        (sample_int && ((st = h->sample_int.alloc((size_t)vocab * 4)) || (st = upload(h->sample_int.p, sample_int, (size_t)vocab * 4))))) {
        delete h;
        return st;
    }
    {
        const int epl = (dim + 63) / 64;
        if ((st = h->syn_lane.alloc((size_t)vocab * lane_row_floats(epl) * 4))) {
            delete h;
            return st;
        }
        d2v_lane_major_kernel<<<ceil_div(vocab, 4), 256>>>(h->syn1neg.as<float>(), h->syn_lane.as<float>(), vocab, dim, epl);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
            delete h;
            return set_error(HIPTS_ERR_HIP, "hipts_d2v_create: building the lane-major copy failed");
        }
    }
    *out = h;
    return HIPTS_OK;
}

int hipts_d2v_destroy(hipts_d2v_t* h) {
    if (h) {
        (void)hipSetDevice(h->device);
        delete h;
    }
    return HIPTS_OK;
}

int hipts_d2v_infer(hipts_d2v_t* h, const int64_t* doc_ptr, const int32_t* words, int64_t ndocs, const float* v0,
                    const uint64_t* seeds, int epochs, float alpha, float min_alpha, float* out, int out_memspace,
                    void* stream) {
    HIPTS_REQUIRE(h && doc_ptr && v0 && seeds && out && ndocs >= 1 && epochs >= 1, "hipts_d2v_infer: bad arguments");
    HIPTS_TRY(use_device(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int64_t nw = doc_ptr[ndocs];
    HIPTS_REQUIRE(doc_ptr[0] == 0 && nw >= 0 && (words || nw == 0), "hipts_d2v_infer: bad CSR");
    Docs docs;
    HIPTS_TRY(stage_documents(h, doc_ptr, words, ndocs, v0, seeds, out, out_memspace, s, &docs));
    const int grid = ceil_div(ndocs, 4);
    static const bool planned_ok = !(getenv("HIPTS_D2V_PLAN") && strcmp(getenv("HIPTS_D2V_PLAN"), "0") == 0);      // A/B switch
    const bool planned = planned_ok && h->negative <= PLAN_MAX_NEG;
    const Model m = model_of(h, planned ? h->syn_lane : h->syn1neg);
    dispatch_epl((h->dim + 63) / 64, [&](auto epl) {
        if (planned)
            d2v_infer_plan_kernel<decltype(epl)::value><<<grid, 256, 0, s>>>(m.syn, m.cum_table, m.sample_int, m.V, m.dim, docs.doc_ptr, docs.words, docs.ndocs,
                                                                              docs.v0, docs.seeds, epochs, alpha, min_alpha, m.negative, m.exp_scale,
                                                                              m.exp_table, docs.out);
        else d2v_infer_kernel<decltype(epl)::value><<<grid, 256, 0, s>>>(m, docs, Schedule{epochs, alpha, min_alpha});
    });
    return finish_documents(h, docs, out, out_memspace, s);
}

int hipts_d2v_set_word_vectors(hipts_d2v_t* h, const float* word_vectors) {
    HIPTS_REQUIRE(h && word_vectors, "hipts_d2v_set_word_vectors: null argument");
    HIPTS_TRY(use_device(h->device));
    HIPTS_TRY(h->word_vectors.alloc((size_t)h->V * h->dim * 4));
    return upload(h->word_vectors.p, word_vectors, (size_t)h->V * h->dim * 4);
}

int hipts_d2v_infer_dm(hipts_d2v_t* h, const int64_t* doc_ptr, const int32_t* words, int64_t ndocs, const float* v0,
                       const uint64_t* seeds, int epochs, float alpha, float min_alpha, int window, int dm_mean, float* out,
                       int out_memspace, void* stream) {
    HIPTS_REQUIRE(h && doc_ptr && v0 && seeds && out && ndocs >= 1 && epochs >= 1, "hipts_d2v_infer_dm: bad arguments");
    HIPTS_REQUIRE(window >= 1, "hipts_d2v_infer_dm: window must be >= 1");
    if (!h->word_vectors.p)
        return set_error(HIPTS_ERR_STATE, "hipts_d2v_infer_dm: the model has no word vectors (hipts_d2v_set_word_vectors)");
    HIPTS_TRY(use_device(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int64_t nw = doc_ptr[ndocs];
    HIPTS_REQUIRE(doc_ptr[0] == 0 && nw >= 0 && (words || nw == 0), "hipts_d2v_infer_dm: bad CSR");
    for (int64_t d = 0; d < ndocs; ++d)
        HIPTS_REQUIRE(doc_ptr[d + 1] >= doc_ptr[d] && doc_ptr[d + 1] - doc_ptr[d] <= DM_CAP,
                      "hipts_d2v_infer_dm: document %lld has %lld words, at most %d are supported", (long long)d,
                      (long long)(doc_ptr[d + 1] - doc_ptr[d]), DM_CAP);
    Docs docs;
    HIPTS_TRY(stage_documents(h, doc_ptr, words, ndocs, v0, seeds, out, out_memspace, s, &docs));
    const Schedule sched{epochs, alpha, min_alpha};
    dispatch_epl((h->dim + 63) / 64, [&](auto epl) {
        d2v_infer_dm_kernel<decltype(epl)::value><<<ceil_div(ndocs, 4), 256, 0, s>>>(model_of(h, h->syn1neg), h->word_vectors.as<float>(), docs, sched,
                                                                                      window, dm_mean ? 1 : 0);
    });
    return finish_documents(h, docs, out, out_memspace, s);
}

int hipts_d2v_train(const uint32_t* cum_table, const uint32_t* sample_int, int64_t vocab, int dim, int negative, double exp_scale,
                    const int64_t* doc_ptr, const int32_t* words, int64_t ndocs, float* doc_vectors, float* syn1neg, int epochs,
                    float alpha, float min_alpha, uint64_t seed, int batch_words, int mode, int device, void* stream) {
    HIPTS_REQUIRE(cum_table && doc_ptr && doc_vectors && syn1neg && vocab >= 1 && vocab < (1ll << 31) && ndocs >= 1 && epochs >= 1,
                  "hipts_d2v_train: bad arguments");
    HIPTS_REQUIRE(dim >= 1 && dim <= 512 && negative >= 0 && negative <= 64 && batch_words >= 1 && (mode == 0 || mode == 1),
                  "hipts_d2v_train: dim in [1, 512], negative in [0, 64], batch_words >= 1, mode 0 (sequential) or 1 (parallel)");
    HIPTS_REQUIRE(cum_table[vocab - 1] > 0, "hipts_d2v_train: cum_table[-1] must be positive");
    const int64_t nw = doc_ptr[ndocs];
    HIPTS_REQUIRE(doc_ptr[0] == 0 && nw >= 0 && (words || nw == 0), "hipts_d2v_train: bad CSR");
    HIPTS_TRY(use_device(device));
    hipStream_t s = (hipStream_t)stream;
    // jobs (word2vec.py::_job_producer): consecutive documents while their raw word counts fit batch_words
    std::vector<int64_t> job_first((size_t)ndocs);
    {
        int64_t first = 0, jw = 0;
        for (int64_t d = 0; d < ndocs; ++d) {
            const int64_t n = doc_ptr[d + 1] - doc_ptr[d];
            if (d == 0 || jw + n > batch_words) {
                first = d;
                jw = 0;
            }
            jw += n;
            job_first[(size_t)d] = first;
        }
    }
    float table[EXP_TABLE_SIZE];
    exp_table_host(table);
    DevBuf d_syn, d_dv, d_cum, d_si, d_ptr, d_words, d_job, d_exp;
    HIPTS_TRY(d_syn.alloc((size_t)vocab * dim * 4));
    HIPTS_TRY(d_dv.alloc((size_t)ndocs * dim * 4));
    HIPTS_TRY(d_cum.alloc((size_t)vocab * 4));
    HIPTS_TRY(d_ptr.alloc((size_t)(ndocs + 1) * 8));
    HIPTS_TRY(d_words.alloc((size_t)(nw > 0 ? nw : 1) * 4));
    HIPTS_TRY(d_job.alloc((size_t)ndocs * 8));
    HIPTS_TRY(d_exp.alloc(sizeof(table)));
    HIPTS_TRY(upload(d_syn.p, syn1neg, (size_t)vocab * dim * 4, s));
    HIPTS_TRY(upload(d_dv.p, doc_vectors, (size_t)ndocs * dim * 4, s));
    HIPTS_TRY(upload(d_cum.p, cum_table, (size_t)vocab * 4, s));
    HIPTS_TRY(upload(d_ptr.p, doc_ptr, (size_t)(ndocs + 1) * 8, s));
    if (nw) HIPTS_TRY(upload(d_words.p, words, (size_t)nw * 4, s));
    HIPTS_TRY(upload(d_job.p, job_first.data(), (size_t)ndocs * 8, s));
    HIPTS_TRY(upload(d_exp.p, table, sizeof(table), s));
    if (sample_int) {
        HIPTS_TRY(d_si.alloc((size_t)vocab * 4));
        HIPTS_TRY(upload(d_si.p, sample_int, (size_t)vocab * 4, s));
    }
    const Model model{d_syn.as<float>(), d_cum.as<uint32_t>(), sample_int ? d_si.as<uint32_t>() : nullptr, d_exp.as<float>(), vocab, dim, negative, exp_scale};
    const Schedule sched{epochs, alpha, min_alpha};
    // sequential: one wavefront, documents [0, ndocs); parallel: a wavefront per document of [d0, d1).  A launch covers one epoch.
    auto launch = [&](auto sequential, int grid, int threads, int e, int64_t d0, int64_t d1) {
        dispatch_epl((dim + 63) / 64, [&](auto epl) {
            d2v_train_kernel<decltype(epl)::value, decltype(sequential)::value><<<grid, threads, 0, s>>>(
                model, sched, d_ptr.as<int64_t>(), d_words.as<int32_t>(), d_job.as<int64_t>(), ndocs, d_dv.as<float>(), seed, e, e + 1, d0, d1);
        });
    };
    if (mode == 0) {
        // one wavefront; a launch per epoch keeps each kernel bounded (a watchdog-safe few seconds even for mid-sized corpora)
        for (int e = 0; e < epochs; ++e) {
            launch(std::true_type{}, 1, 64, e, 0, ndocs);
            HIPTS_LAUNCH_CHECK();
        }
    } else {
        static const int64_t chunk = getenv("HIPTS_D2V_CHUNK") && atoll(getenv("HIPTS_D2V_CHUNK")) > 0 ? atoll(getenv("HIPTS_D2V_CHUNK")) : 2048;
        for (int e = 0; e < epochs; ++e)
            for (int64_t d0 = 0; d0 < ndocs; d0 += chunk) {
                const int64_t d1 = d0 + chunk < ndocs ? d0 + chunk : ndocs;
                launch(std::false_type{}, ceil_div(d1 - d0, 4), 256, e, d0, d1);
                HIPTS_LAUNCH_CHECK();
            }
    }
    HIPTS_HIP(hipMemcpyAsync(syn1neg, d_syn.p, (size_t)vocab * dim * 4, hipMemcpyDeviceToHost, s));
    HIPTS_HIP(hipMemcpyAsync(doc_vectors, d_dv.p, (size_t)ndocs * dim * 4, hipMemcpyDeviceToHost, s));
    HIPTS_HIP(hipStreamSynchronize(s));
    return HIPTS_OK;
}

}  // extern "C"
