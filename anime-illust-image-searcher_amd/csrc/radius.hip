// radius.hip -- fixed-radius neighbour lists over the feature index and DBSCAN on top of them (hipts_radius_*).
//
// Goes past the reference: its CCIP code comes from a library that offers clustering over the pairwise differences
// (gen_cfeatures.py:257-274 is the pairwise call); here the relation is the one crerank.hip cuts by,
//     j in N(i)  <=>  1.0f - s(i, j) < T     (float32; s = hipts_index_query's product of row i against row j),
// for ALL pairs of index rows, without ever storing a score.
//
//   product    radius_pairs_kernel: a block of 256 index rows (8 tiles of 32) plays the queries, staged k-chunk by k-chunk in LDS out of
//              the tile-major copy; every wave of the workgroup multiplies its own 32-row document tile against the 8 query tiles with
//              v_mfma_f32_32x32x2_f32 -- operands and k order of sim_mfma_wide_kernel, so s(i, j) has hipts_index_query's bits.  The
//              chain is symmetric bit for bit (fmaf(a, b, c) == fmaf(b, a, c), same k order), so only block pairs (I, J >= I) are
//              walked: an off-diagonal block credits both rows of a pair, the diagonal block is computed as the full square and
//              credits the query side only.  The comparison happens on the accumulators.
//   pass 1     counts degrees (integer atomics: their sum does not depend on the order)
//   scan       degrees -> int64 CSR offsets (one workgroup)
//   pass 2     the same product again; a row's slots are handed out by an atomic cursor, so the ids arrive in any order ...
//   sort       ... and every row is then sorted ascending: the lists are the same bytes run to run
//   dbscan     core flags from the degrees; components of the core rows by min-label propagation with pointer jumping (one launch per
//              sweep, the host reads a "changed" flag back; labels only ever decrease and the fixed point is the smallest core index
//              of the component, whatever the interleaving); roots -> ranks by flag + scan; border rows take the smallest label among
//              their core neighbours.  No workgroup waits for another one anywhere.
// Compiled with -ffp-contract=off: diff = 1 - s stays one float32 subtraction.
//
// A second relation builds the same handle (hipts_radius_create_hamming): the Hamming distance of 128-bit image hashes (imghash.hip),
//     j in N(i)  <=>  popcount(h_i[0] ^ h_j[0]) + popcount(h_i[1] ^ h_j[1]) <= T,
// by hamming_pairs_kernel through the same pass 1 / scan / pass 2 / sort (radius_build); everything from the lists on is shared.
// Its algorithmic work: rows^2 / 2 pairs per pass at nine vector instructions each (four XORs, four accumulating population counts,
// one compare); bytes: 16 per row per block pair it takes part in, read as uniform loads, plus the lists.
#include <algorithm>
#include <vector>

#include "../../include/hip_tagsearch_debug.h"
#include "common.h"
#include "rank_util.h"

using namespace hipts;

struct hipts_radius {
    int device = 0;
    int64_t rows = 0, pairs = 0;
    float pass_ms[3] = {0.f, 0.f, 0.f};                // pass 1, pass 2, row sort of the create call (hiptsdbg_radius_passes)
    DevBuf d_deg, d_ptr, d_ids;                        // int32 [rows], int64 [rows + 1], int32 [pairs]
    DevBuf ws_label, ws_flag, ws_rank, ws_out, ws_changed;      // dbscan: int32 [rows] x2, int64 [rows + 1], int32 [rows], int32
};

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int RAD_QS = 288;              // floats per k-row of the LDS chunk: 256 queries + 32 (the two half-waves use different banks)
constexpr int RAD_BLOCK = 256;           // index rows per block = 8 tiles: the queries of a workgroup, and its 8 waves' document tiles
constexpr int RAD_SORT_THREADS = 256;
constexpr int RAD_SORT_LDS = 2048;       // rows up to this long are sorted in LDS, longer ones in place in global memory
constexpr int32_t RAD_NONCORE = 0x7fffffff;

// work item p of the upper triangle (row-block I, document block g >= I), row-major: row I holds nb - I items
__device__ __forceinline__ void radius_decode(int64_t p, int64_t nb, int64_t& I, int64_t& g) {
    auto off = [&](int64_t x) { return x * nb - x * (x - 1) / 2; };
    const double d = 2.0 * (double)nb + 1.0;
    int64_t i = (int64_t)((d - sqrt(d * d - 8.0 * (double)p)) * 0.5);
    i = i < 0 ? 0 : (i > nb - 1 ? nb - 1 : i);
    while (i > 0 && off(i) > p) --i;
    while (i + 1 < nb && off(i + 1) <= p) ++i;
    I = i;
    g = i + (p - off(i));
}

// FILL false: pass 1, deg[row] += the row's neighbours found here.  FILL true: pass 2, the ids go to ids[ptr[row] + slot], the slots
// handed out by cursor[row]; deg is read-only then and bounds every slot.
template <bool FILL>
__global__ __launch_bounds__(512) void radius_pairs_kernel(const float4* __restrict__ tiled, int64_t N, int K, float T, int64_t nblk, int64_t nwork,
                                                           int32_t* __restrict__ deg, const int64_t* __restrict__ ptr,
                                                           int32_t* __restrict__ cursor, int32_t* __restrict__ ids) {
    __shared__ float qs[2][8][RAD_QS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t ntiles = (N + 31) / 32;
    const int KQ = K >> 2;                       // float4 per row
    const int nchunks = (KQ + 1) >> 1;           // 8 k per chunk; the last one holds 4 when K % 8 == 4
    const int nfull = KQ >> 1;
    const int sj = tid & 255, sh = tid >> 8;     // staging role: query sj of the block, k-half sh of the chunk (a wave reads 2 x 512 contiguous bytes)
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t p = blockIdx.x; p < nwork; p += gridDim.x) {
        int64_t I, g;
        radius_decode(p, nblk, I, g);
        const int64_t qtile = I * 8 + (sj >> 5);
        const bool qv = qtile < ntiles;          // rows past N inside the last tile are zero in the tile-major copy
        const float4* __restrict__ qsrc = tiled + (qv ? qtile : ntiles - 1) * KQ * 32 + (sj & 31);
        auto load_q = [&](int c) {
            const int kq = 2 * c + sh;
            return (qv && kq < KQ) ? qsrc[(int64_t)kq * 32] : zero4;
        };
        auto store_q = [&](int buf, float4 v) {
            qs[buf][4 * sh + 0][sj] = v.x;
            qs[buf][4 * sh + 1][sj] = v.y;
            qs[buf][4 * sh + 2][sj] = v.z;
            qs[buf][4 * sh + 3][sj] = v.w;
        };
        const int64_t tile = g * 8 + wave;
        const bool tv = tile < ntiles;
        const float4* __restrict__ trow = tiled + (tv ? tile : ntiles - 1) * KQ * 32 + r;
        f32x16 acc[8];
#pragma unroll
        for (int b = 0; b < 8; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[b][i] = 0.0f;
        float4 d0 = trow[0], d1 = 1 < KQ ? trow[32] : zero4;
        store_q(0, load_q(0));                   // buffer 0 was last read before the final barrier of the previous work item
        __syncthreads();
        for (int c = 0; c < nfull; ++c) {
            const bool more = c + 1 < nchunks;
            float4 qn = zero4, e0 = zero4, e1 = zero4;
            if (more) {                          // the next chunk's loads are in flight under this chunk's MFMAs
                qn = load_q(c + 1);
                e0 = trow[(2 * c + 2) * 32];
                e1 = 2 * c + 3 < KQ ? trow[(2 * c + 3) * 32] : zero4;
            }
            const float b0 = h ? d0.y : d0.x, b1 = h ? d0.w : d0.z, b2 = h ? d1.y : d1.x, b3 = h ? d1.w : d1.z;
            const float* qrow = &qs[c & 1][h][r];
            // k-pair by k-pair across the query tiles: consecutive MFMAs are independent, per tile the k order is ascending
#pragma unroll
            for (int b = 0; b < 8; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow[b * 32], b0, acc[b], 0, 0, 0);
#pragma unroll
            for (int b = 0; b < 8; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow[b * 32 + 2 * RAD_QS], b1, acc[b], 0, 0, 0);
#pragma unroll
            for (int b = 0; b < 8; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow[b * 32 + 4 * RAD_QS], b2, acc[b], 0, 0, 0);
#pragma unroll
            for (int b = 0; b < 8; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow[b * 32 + 6 * RAD_QS], b3, acc[b], 0, 0, 0);
            if (more) {
                store_q((c + 1) & 1, qn);
                d0 = e0;
                d1 = e1;
            }
            __syncthreads();
        }
        if (KQ & 1) {                            // the chunk of 4 (staged by the last iteration above, or by the prologue when K == 4)
            const float b0 = h ? d0.y : d0.x, b1 = h ? d0.w : d0.z;
            const float* qrow = &qs[nfull & 1][h][r];
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow[b * 32], b0, acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow[b * 32 + 2 * RAD_QS], b1, acc[b], 0, 0, 0);
            }
            __syncthreads();                     // the next work item's prologue writes buffer 0 again
        }
        // D layout: column = lane & 31 = document, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) = query of the tile.  No barrier below.
        const int64_t doc = tile * 32 + r;
        const bool dv = tv && doc < N;
        const bool diag = g == I;                // the full square: every ordered pair is here itself, credit the query side only
        int dcount = 0;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int64_t q0 = (I * 8 + b) * 32;                 // first row of query tile b
            uint32_t m = 0;                                      // bit reg: (query of reg, doc) are neighbours
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int64_t qr = q0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                const float diff = 1.0f - acc[b][reg];
                if (dv && qr < N && diff < T) m |= 1u << reg;    // float32 comparison
            }
            if (__ballot(m != 0) == 0) continue;                 // uniform: nothing under the threshold in this 32 x 32 tile
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {                 // query side: the 32 lanes of a half-wave share the query
                const bool on = (m >> reg) & 1;
                const uint64_t bal = __ballot(on);
                if (bal == 0) continue;                          // uniform
                const uint32_t mine = h ? (uint32_t)(bal >> 32) : (uint32_t)bal;
                const int cnt = __popc(mine);
                const int64_t qr = q0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;      // < N when cnt > 0
                if (!FILL) {
                    if (r == 0 && cnt) atomicAdd(&deg[qr], cnt);
                } else {
                    int base = 0;
                    if (r == 0 && cnt) base = atomicAdd(&cursor[qr], cnt);
                    base = __shfl(base, lane & 32);
                    if (on) {
                        const int k = base + __popc(mine & ((1u << r) - 1u));
                        if (k < deg[qr]) ids[ptr[qr] + k] = (int32_t)doc;
                    }
                }
            }
            if (!diag && m) {                                    // document side: by symmetry s(doc, query) has the same bits
                const int c = __popc(m);
                if (!FILL) {
                    dcount += c;
                } else {
                    int k = atomicAdd(&cursor[doc], c);
                    const int lim = deg[doc];
                    const int64_t o = ptr[doc];
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg)
                        if ((m >> reg) & 1) {
                            if (k < lim) ids[o + k] = (int32_t)(q0 + (reg & 3) + 8 * (reg >> 2) + 4 * h);
                            ++k;
                        }
                }
            }
        }
        if (!FILL && dcount) atomicAdd(&deg[doc], dcount);
    }
}

// out[i] = in[0] + ... + in[i - 1] for i = 0 .. n (one workgroup)
__global__ __launch_bounds__(1024) void radius_scan_kernel(const int32_t* __restrict__ in, int64_t n, long long* __restrict__ out) {
    __shared__ long long scratch[17];
    long long carry = 0;
    for (int64_t b0 = 0; b0 < n; b0 += 1024) {
        const int64_t i = b0 + threadIdx.x;
        const long long c = i < n ? (long long)in[i] : 0;
        long long total;
        const long long ex = block_excl_scan(c, scratch, &total);
        if (i < n) out[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) out[n] = carry;
}

// One workgroup per row: its ids ascending.  The bitonic network in the form whose comparators all point the same way (each merge
// starts with the mirror step i <-> i ^ (k - 1)): the smaller value always goes to the lower index, so the slots past n, thought of as
// holding +inf, never take part and n need not be a power of two.
__device__ __forceinline__ void radius_sort_ascending(int32_t* a, uint32_t n) {
    const uint32_t tid = threadIdx.x;
    uint32_t P = 2;
    while (P < n) P <<= 1;
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const bool mirror = j == (k >> 1);
            for (uint32_t i = tid; i < n; i += RAD_SORT_THREADS) {
                const uint32_t x = mirror ? i ^ (k - 1) : i ^ j;
                if (x > i && x < n) {
                    const int32_t u = a[i], v = a[x];
                    if (u > v) {
                        a[i] = v;
                        a[x] = u;
                    }
                }
            }
            __syncthreads();                     // n is uniform: every thread passes the same barriers; orders the global form too
        }
    }
}
__global__ __launch_bounds__(RAD_SORT_THREADS) void radius_sort_rows_kernel(const long long* __restrict__ ptr, int32_t* ids) {
    __shared__ int32_t sk[RAD_SORT_LDS];
    const long long b = ptr[blockIdx.x], e = ptr[blockIdx.x + 1];
    const uint32_t n = (uint32_t)(e - b);        // < 2^31
    if (n < 2) return;                           // uniform
    int32_t* row = ids + b;
    if (n <= RAD_SORT_LDS) {
        for (uint32_t i = threadIdx.x; i < n; i += RAD_SORT_THREADS) sk[i] = row[i];
        __syncthreads();
        radius_sort_ascending(sk, n);
        for (uint32_t i = threadIdx.x; i < n; i += RAD_SORT_THREADS) row[i] = sk[i];
    } else {
        radius_sort_ascending(row, n);
    }
}

// ---------------------------------------------------------------------------------------------
// DBSCAN over the lists
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void radius_core_kernel(const int32_t* __restrict__ deg, int64_t n, int min_samples, int32_t* __restrict__ label) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) label[i] = deg[i] >= min_samples ? (int32_t)i : RAD_NONCORE;
}

// One sweep.  label[i] of a core row is always the index of a core row of i's component, <= i.  A row takes the minimum over its core
// neighbours' labels, follows the labels down from there (pointer jumping), and lowers its own label and its old root's to what it
// found.  Values read while other threads lower them are merely older: labels only decrease, so the fixed point -- every row of a
// component at the component's smallest core index -- is the same whatever the interleaving.
__global__ __launch_bounds__(256) void radius_sweep_kernel(const long long* __restrict__ ptr, const int32_t* __restrict__ ids, int32_t* label, int64_t n,
                                                           int32_t* changed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t old = __atomic_load_n(&label[i], __ATOMIC_RELAXED);
    if (old == RAD_NONCORE) return;
    int32_t m = old;
    for (long long e = ptr[i]; e < ptr[i + 1]; ++e) {
        const int32_t lj = __atomic_load_n(&label[ids[e]], __ATOMIC_RELAXED);      // RAD_NONCORE is above every index
        m = lj < m ? lj : m;
    }
    for (;;) {                                   // strictly decreasing: ends at a row that is its own label
        const int32_t up = __atomic_load_n(&label[m], __ATOMIC_RELAXED);
        if (up >= m) break;
        m = up;
    }
    if (m < old) {
        atomicMin(&label[i], m);
        atomicMin(&label[old], m);
        *changed = 1;
    }
}

__global__ __launch_bounds__(256) void radius_roots_kernel(const int32_t* __restrict__ label, int64_t n, int32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) flag[i] = label[i] == (int32_t)i ? 1 : 0;
}

// core: the rank of its root; border: the smallest such rank among its core neighbours; noise: -1
__global__ __launch_bounds__(256) void radius_assign_kernel(const long long* __restrict__ ptr, const int32_t* __restrict__ ids,
                                                            const int32_t* __restrict__ label, const long long* __restrict__ rank, int64_t n,
                                                            int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t li = label[i];
    if (li != RAD_NONCORE) {
        out[i] = (int32_t)rank[li];
        return;
    }
    long long best = -1;
    for (long long e = ptr[i]; e < ptr[i + 1]; ++e) {
        const int32_t lj = label[ids[e]];
        if (lj == RAD_NONCORE) continue;
        const long long c = rank[lj];
        if (best < 0 || c < best) best = c;
    }
    out[i] = (int32_t)best;
}

// ---------------------------------------------------------------------------------------------
// The Hamming relation over 128-bit hashes (hipts_radius_create_hamming)
// ---------------------------------------------------------------------------------------------
constexpr int HAM_BLOCK = 256;           // rows per block = threads per workgroup: a lane per row of block I
constexpr int HAM_UNROLL = 8;            // rows of block J per step: their 32 dwords are requested together
constexpr int HAM_GRID_PER_CU = 32;      // workgroups per CU in the grid (8 fit at a time); the block pairs are walked grid-stride

// j in N(i)  <=>  popcount(h_i ^ h_j) <= T over the four dwords.  Block pairs (I, J >= I), radius_pairs_kernel's convention: an
// off-diagonal block credits both rows of a hit, the diagonal block is walked as the full square and credits the row side only.  A lane
// keeps its own row of block I in registers and walks the rows of block J, whose dwords are the same for every lane: I and J are made
// wave-uniform explicitly, so the loads are uniform ones that land in scalar registers -- four XORs against them, four population
// counts that accumulate and one compare per pair.  Hits are rare: the ballots of HAM_UNROLL rows are ORed, and everything after that
// runs only where the OR is non-zero.  FILL as in radius_pairs_kernel.  Rows at or beyond N take no part on either side.
template <bool FILL>
__global__ __launch_bounds__(HAM_BLOCK) void hamming_pairs_kernel(const uint32_t* __restrict__ words, int64_t N, int T, int64_t nblk, int64_t nwork,
                                                                  int32_t* __restrict__ deg, const int64_t* __restrict__ ptr,
                                                                  int32_t* __restrict__ cursor, int32_t* __restrict__ ids) {
    const int tid = threadIdx.x, lane = tid & 63;
    for (int64_t p = blockIdx.x; p < nwork; p += gridDim.x) {
        int64_t Id, Jd;
        radius_decode(p, nblk, Id, Jd);
        const int64_t I = __builtin_amdgcn_readfirstlane((int)Id), J = __builtin_amdgcn_readfirstlane((int)Jd);      // nblk < 2^23
        const int64_t i = I * HAM_BLOCK + tid;
        const bool iv = i < N;
        const uint2* __restrict__ own = reinterpret_cast<const uint2*>(words) + 2 * (iv ? i : 0);      // a uint64 pointer: 8-byte aligned
        const uint2 w0 = own[0], w1 = own[1];
        const uint4 mine = make_uint4(w0.x, w0.y, w1.x, w1.y);
        const int64_t j0 = J * HAM_BLOCK;
        const int jn = (int)(N - j0 < HAM_BLOCK ? N - j0 : HAM_BLOCK);      // >= 1
        const bool diag = I == J;
        const uint32_t* __restrict__ other = words + 4 * j0;
        const int tl = iv ? T : -1;                              // a lane without a row is nobody's neighbour, without a branch
        auto hit_mask = [&](uint32_t o0, uint32_t o1, uint32_t o2, uint32_t o3) -> uint64_t {       // the lanes whose row is a neighbour of row o
            int d = __popc(mine.x ^ o0);
            d += __popc(mine.y ^ o1);
            d += __popc(mine.z ^ o2);
            d += __popc(mine.w ^ o3);
            return __ballot(d <= tl);
        };
        int count = 0;                                           // pass 1: this lane's own row
        auto credit = [&](int j, uint64_t m) {                   // m != 0, uniform
            const bool on = (m >> lane) & 1;
            const int64_t jr = j0 + j;
            if (!FILL) {
                count += on ? 1 : 0;
                if (!diag && lane == 0) atomicAdd(&deg[jr], __popcll(m));
            } else {
                if (on) {
                    const int k = atomicAdd(&cursor[i], 1);
                    if (k < deg[i]) ids[ptr[i] + k] = (int32_t)jr;
                }
                if (!diag) {
                    int base = 0;
                    if (lane == 0) base = atomicAdd(&cursor[jr], __popcll(m));
                    base = __builtin_amdgcn_readfirstlane(base);
                    if (on) {
                        const int k = base + __popcll(m & (((uint64_t)1 << lane) - 1));
                        if (k < deg[jr]) ids[ptr[jr] + k] = (int32_t)i;
                    }
                }
            }
        };
        int j = 0;
        for (; j + HAM_UNROLL <= jn; j += HAM_UNROLL) {
            uint32_t o[4 * HAM_UNROLL];
#pragma unroll
            for (int k = 0; k < 4 * HAM_UNROLL; ++k) o[k] = other[4 * j + k];
            uint64_t m[HAM_UNROLL], any = 0;
#pragma unroll
            for (int u = 0; u < HAM_UNROLL; ++u) {
                m[u] = hit_mask(o[4 * u], o[4 * u + 1], o[4 * u + 2], o[4 * u + 3]);
                any |= m[u];
            }
            if (any == 0) continue;                              // uniform
#pragma unroll
            for (int u = 0; u < HAM_UNROLL; ++u)
                if (m[u]) credit(j + u, m[u]);
        }
        for (; j < jn; ++j) {                                    // the ragged last block
            const uint32_t* __restrict__ o = other + 4 * j;
            const uint64_t m = hit_mask(o[0], o[1], o[2], o[3]);
            if (m) credit(j, m);
        }
        if (!FILL && count) atomicAdd(&deg[i], count);
    }
}

// The pass 1 / scan / pass 2 / sort protocol both relations share.  launch(fill, deg, ptr, cursor, ids) enqueues the relation's pair
// kernel on `s`; `who` and `where` word the refusal ("<who>: <count> neighbour pairs <where>, max_pairs allows <max_pairs>").
template <typename Launch>
int radius_build(const char* who, const char* where, int device, int64_t N, int64_t max_pairs, hipStream_t s, hipts_radius_t** out, Launch launch) {
    if (max_pairs == 0) {                        // the library's default: the ids may take half of what is free now
        size_t free_b = 0, total_b = 0;
        HIPTS_HIP(hipMemGetInfo(&free_b, &total_b));
        max_pairs = (int64_t)(free_b / 2 / 4);
    }
    hipts_radius* h = new hipts_radius();
    h->device = device;
    h->rows = N;
    DevBuf cursor;
    hipEvent_t ev[5] = {};                       // around pass 1, around pass 2, after the sort
    auto run = [&]() -> int {
        for (auto& e : ev) HIPTS_HIP(hipEventCreate(&e));
        HIPTS_TRY(h->d_deg.alloc((size_t)N * 4));
        HIPTS_TRY(h->d_ptr.alloc((size_t)(N + 1) * 8));
        HIPTS_HIP(hipMemsetAsync(h->d_deg.p, 0, (size_t)N * 4, s));
        HIPTS_HIP(hipEventRecord(ev[0], s));
        launch(false, h->d_deg.as<int32_t>(), nullptr, nullptr, nullptr);
        HIPTS_LAUNCH_CHECK();
        HIPTS_HIP(hipEventRecord(ev[1], s));
        radius_scan_kernel<<<1, 1024, 0, s>>>(h->d_deg.as<int32_t>(), N, h->d_ptr.as<long long>());
        HIPTS_LAUNCH_CHECK();
        long long total = 0;
        HIPTS_HIP(hipMemcpyAsync(&total, h->d_ptr.as<long long>() + N, 8, hipMemcpyDeviceToHost, s));
        HIPTS_HIP(hipStreamSynchronize(s));
        HIPTS_REQUIRE(total <= max_pairs, "%s: %lld neighbour pairs %s, max_pairs allows %lld", who, total, where, (long long)max_pairs);
        h->pairs = total;
        HIPTS_TRY(h->d_ids.alloc((size_t)total * 4));
        HIPTS_TRY(cursor.alloc((size_t)N * 4));
        HIPTS_HIP(hipMemsetAsync(cursor.p, 0, (size_t)N * 4, s));
        HIPTS_HIP(hipEventRecord(ev[2], s));
        launch(true, h->d_deg.as<int32_t>(), h->d_ptr.as<int64_t>(), cursor.as<int32_t>(), h->d_ids.as<int32_t>());
        HIPTS_LAUNCH_CHECK();
        HIPTS_HIP(hipEventRecord(ev[3], s));
        radius_sort_rows_kernel<<<(int)N, RAD_SORT_THREADS, 0, s>>>(h->d_ptr.as<long long>(), h->d_ids.as<int32_t>());
        HIPTS_LAUNCH_CHECK();
        HIPTS_HIP(hipEventRecord(ev[4], s));
        HIPTS_HIP(hipStreamSynchronize(s));
        HIPTS_HIP(hipEventElapsedTime(&h->pass_ms[0], ev[0], ev[1]));
        HIPTS_HIP(hipEventElapsedTime(&h->pass_ms[1], ev[2], ev[3]));
        HIPTS_HIP(hipEventElapsedTime(&h->pass_ms[2], ev[3], ev[4]));
        return HIPTS_OK;
    };
    const int st = run();
    for (auto& e : ev)
        if (e) (void)hipEventDestroy(e);
    if (st != HIPTS_OK) {
        delete h;
        return st;
    }
    *out = h;
    return HIPTS_OK;
}

}  // namespace

extern "C" {

int hipts_radius_create(hipts_index_t* features, float threshold, int64_t max_pairs, void* stream, hipts_radius_t** out) {
    HIPTS_REQUIRE(out, "hipts_radius_create: null output");
    *out = nullptr;
    HIPTS_REQUIRE(features && max_pairs >= 0, "hipts_radius_create: bad arguments");
    const float4* tiled = nullptr;
    int64_t N = 0;
    int dim = 0, device = 0;
    HIPTS_TRY(index_tiled_view(features, &tiled, &N, &dim, &device));
    HIPTS_REQUIRE(dim >= 4 && dim % 4 == 0, "hipts_radius_create: the index dimension must be a multiple of 4, got %d", dim);
    HIPTS_REQUIRE(N > 0 && tiled, "hipts_radius_create: empty index");
    HIPTS_REQUIRE(N < ((int64_t)1 << 31), "hipts_radius_create: %lld rows, the limit is 2^31 - 1", (long long)N);
    HIPTS_TRY(use_device(device));
    hipStream_t s = (hipStream_t)stream;
    const int64_t nblk = (N + RAD_BLOCK - 1) / RAD_BLOCK, nwork = nblk * (nblk + 1) / 2;
    const int grid = (int)std::min<int64_t>(nwork, (int64_t)1 << 22);
    return radius_build("hipts_radius_create", "under the threshold", device, N, max_pairs, s, out,
                        [&](bool fill, int32_t* deg, const int64_t* ptr, int32_t* cursor, int32_t* ids) {
                            if (fill) radius_pairs_kernel<true><<<grid, 512, 0, s>>>(tiled, N, dim, threshold, nblk, nwork, deg, ptr, cursor, ids);
                            else radius_pairs_kernel<false><<<grid, 512, 0, s>>>(tiled, N, dim, threshold, nblk, nwork, deg, ptr, cursor, ids);
                        });
}

int hipts_radius_create_hamming(const uint64_t* hashes, int hashes_memspace, int64_t rows, int max_distance, int64_t max_pairs, int device,
                                void* stream, hipts_radius_t** out) {
    HIPTS_REQUIRE(out, "hipts_radius_create_hamming: null output");
    *out = nullptr;
    HIPTS_REQUIRE(max_distance >= 0 && max_distance <= 128, "hipts_radius_create_hamming: max_distance must be in [0, 128], got %d", max_distance);
    HIPTS_REQUIRE(rows > 0, "hipts_radius_create_hamming: empty input");
    HIPTS_REQUIRE(hashes && max_pairs >= 0, "hipts_radius_create_hamming: bad arguments");
    HIPTS_REQUIRE(rows < ((int64_t)1 << 31), "hipts_radius_create_hamming: %lld rows, the limit is 2^31 - 1", (long long)rows);
    HIPTS_TRY(use_device(device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf copy;                                 // host hashes: a device copy that lives as long as this call (which ends synchronised)
    const uint32_t* words = reinterpret_cast<const uint32_t*>(hashes);
    if (hashes_memspace != HIPTS_DEVICE) {
        HIPTS_TRY(copy.alloc((size_t)rows * 16));
        HIPTS_HIP(hipMemcpyAsync(copy.p, hashes, (size_t)rows * 16, hipMemcpyHostToDevice, s));
        words = copy.as<uint32_t>();
    }
    const int64_t nblk = (rows + HAM_BLOCK - 1) / HAM_BLOCK, nwork = nblk * (nblk + 1) / 2;
    const int grid = (int)std::min<int64_t>(nwork, (int64_t)HAM_GRID_PER_CU * current_device_cus());
    return radius_build("hipts_radius_create_hamming", "within the distance", device, rows, max_pairs, s, out,
                        [&](bool fill, int32_t* deg, const int64_t* ptr, int32_t* cursor, int32_t* ids) {
                            if (fill) hamming_pairs_kernel<true><<<grid, HAM_BLOCK, 0, s>>>(words, rows, max_distance, nblk, nwork, deg, ptr, cursor, ids);
                            else hamming_pairs_kernel<false><<<grid, HAM_BLOCK, 0, s>>>(words, rows, max_distance, nblk, nwork, deg, ptr, cursor, ids);
                        });
}

int hipts_radius_destroy(hipts_radius_t* h) {
    if (h) {
        (void)use_device(h->device);
        delete h;
    }
    return HIPTS_OK;
}

int hipts_radius_info(const hipts_radius_t* h, int64_t* rows, int64_t* pairs) {
    HIPTS_REQUIRE(h, "hipts_radius_info: null handle");
    if (rows) *rows = h->rows;
    if (pairs) *pairs = h->pairs;
    return HIPTS_OK;
}

int hiptsdbg_radius_passes(const hipts_radius_t* h, double* pass1_ms, double* pass2_ms, double* sort_ms) {
    HIPTS_REQUIRE(h, "null handle");
    if (pass1_ms) *pass1_ms = h->pass_ms[0];
    if (pass2_ms) *pass2_ms = h->pass_ms[1];
    if (sort_ms) *sort_ms = h->pass_ms[2];
    return HIPTS_OK;
}

int hipts_radius_read(hipts_radius_t* h, int64_t* ptr_out, int32_t* ids_out) {
    HIPTS_REQUIRE(h && ptr_out && (ids_out || h->pairs == 0), "hipts_radius_read: null argument");
    HIPTS_TRY(use_device(h->device));
    HIPTS_HIP(hipMemcpy(ptr_out, h->d_ptr.p, (size_t)(h->rows + 1) * 8, hipMemcpyDeviceToHost));
    if (h->pairs > 0) HIPTS_HIP(hipMemcpy(ids_out, h->d_ids.p, (size_t)h->pairs * 4, hipMemcpyDeviceToHost));
    return HIPTS_OK;
}

int hipts_radius_dbscan(hipts_radius_t* h, int min_samples, int32_t* labels_out, int64_t* num_clusters, int32_t* sweeps_out) {
    HIPTS_REQUIRE(h && labels_out, "hipts_radius_dbscan: null argument");
    HIPTS_REQUIRE(min_samples >= 1, "hipts_radius_dbscan: min_samples must be at least 1, got %d", min_samples);
    HIPTS_TRY(use_device(h->device));
    const int64_t N = h->rows;
    const int nb = ceil_div(N, 256);
    HIPTS_TRY(h->ws_label.reserve((size_t)N * 4));
    HIPTS_TRY(h->ws_flag.reserve((size_t)N * 4));
    HIPTS_TRY(h->ws_rank.reserve((size_t)(N + 1) * 8));
    HIPTS_TRY(h->ws_out.reserve((size_t)N * 4));
    HIPTS_TRY(h->ws_changed.reserve(4));
    const long long* ptr = h->d_ptr.as<long long>();
    const int32_t* ids = h->d_ids.as<int32_t>();
    int32_t* label = h->ws_label.as<int32_t>();
    radius_core_kernel<<<nb, 256>>>(h->d_deg.as<int32_t>(), N, min_samples, label);
    HIPTS_LAUNCH_CHECK();
    int64_t sweeps = 0;
    bool settled = false;
    while (sweeps < N && !settled) {             // hard cap: a path of N rows settles in N - 1 sweeps, the N-th finds nothing to do
        int32_t changed = 0;
        HIPTS_HIP(hipMemsetAsync(h->ws_changed.p, 0, 4, nullptr));
        radius_sweep_kernel<<<nb, 256>>>(ptr, ids, label, N, h->ws_changed.as<int32_t>());
        HIPTS_LAUNCH_CHECK();
        HIPTS_HIP(hipMemcpy(&changed, h->ws_changed.p, 4, hipMemcpyDeviceToHost));
        ++sweeps;
        settled = changed == 0;
    }
    if (sweeps_out) *sweeps_out = (int32_t)sweeps;
    if (!settled) return set_error(HIPTS_ERR_INVALID, "hipts_radius_dbscan: the labels had not settled after %lld sweeps (the cap)", (long long)sweeps);
    radius_roots_kernel<<<nb, 256>>>(label, N, h->ws_flag.as<int32_t>());
    HIPTS_LAUNCH_CHECK();
    radius_scan_kernel<<<1, 1024>>>(h->ws_flag.as<int32_t>(), N, h->ws_rank.as<long long>());
    HIPTS_LAUNCH_CHECK();
    radius_assign_kernel<<<nb, 256>>>(ptr, ids, label, h->ws_rank.as<long long>(), N, h->ws_out.as<int32_t>());
    HIPTS_LAUNCH_CHECK();
    long long clusters = 0;
    HIPTS_HIP(hipMemcpy(&clusters, h->ws_rank.as<long long>() + N, 8, hipMemcpyDeviceToHost));
    HIPTS_HIP(hipMemcpy(labels_out, h->ws_out.p, (size_t)N * 4, hipMemcpyDeviceToHost));
    if (num_clusters) *num_clusters = clusters;
    return HIPTS_OK;
}

}  // extern "C"
