// gemm_loop.h -- the named pieces of the GEMM main loops outside their epilogues, each stated once: the tile walk of the persistent loops
// (gemm_pp_kernel, gemm_q4_kernel, and the host through hiptsdbg_gemm_tile_walk), a persistent workgroup's work item, the
// folded-LayerNorm row table of the pp, dw and 4-wave loops, the test "this launch takes the LDS-staged epilogue" of the pp and dw
// loops and of launch_gemm's precondition, and of the ping-pong loop's K-tile the multiply of a phase (with the HIPTS_MFMA_ORDER index
// helper).  Included INSIDE `namespace hipts { namespace {` of gemm.hip and gemm4.hip, directly after
// gemm_epi.h: every function is a forceinline function of that translation unit.
// What is here compiles, in every kernel that calls it, to the registers, LDS, scratch and per-opcode counts of MFMA, LDS, memory,
// barrier and wait instructions it had with the text in place (tools/kernel_diff.py; LABNOTES, "GEMM main loops").  A function is
// simplified on its own before it is inlined, so that is not a given: the ping-pong loop's staging slots, the K-tile as a whole, its
// fragment reads and staging schedules, the split-K tail, the cycle stamps, the epilogue choice and the stat_part finish were tried here too, moved one of
// those figures (the fragment reads: integer address instructions in 8 of 9 kernels probed) each, and stay text in the kernels.

// ---- tile walk ---------------------------------------------------------------------------------------------------------------
// Origin (first row, first column) of tile number `id` of a tiles_m x tiles_n grid of TILE_ROWS x BN tiles.  The id is first put
// through the XCD remap (xcd_work_id: ids equal mod 8 share an L2 and are handed one contiguous run of the order below), then
// placed by the launcher's raster (GemmArgs::raster_gn / raster_gm; neither: row-major).  Persistent workgroup w walks ids w,
// w + grid, w + 2 grid, ...; the grid is a multiple of 8 (or the whole problem), so every tile of a workgroup keeps its XCD and
// the workgroups that share an L2 walk neighbouring tiles.
template <int TILE_ROWS>
__host__ __device__ __forceinline__ void tile_origin(const GemmArgs& a, int id, int tiles_m, int tiles_n, int& m0, int& n0) {
    const int bid = xcd_work_id(id, tiles_m * tiles_n);
    if (a.raster_gn > 0) {
        // Column groups outermost: all row panels x raster_gn column tiles, row-major inside the group, then the next group.
        // An XCD's contiguous chunk of the order then lies inside one group (or two): its slice of W (raster_gn panels) is all the
        // W it ever reads and stays in its L2, a round is 32 / raster_gn row panels x raster_gn column tiles, and a row panel of A
        // is fetched once per column group.
        const int per = tiles_m * a.raster_gn, grp = bid / per, rem = bid - grp * per;
        const int left = tiles_n - grp * a.raster_gn, gn = left < a.raster_gn ? left : a.raster_gn;
        m0 = (rem / gn) * TILE_ROWS;
        n0 = (grp * a.raster_gn + rem % gn) * BN;
        return;
    }
    if (a.raster_gm > 0) {
        // Wide outputs (fc1: 12 column tiles): row-major order hands the 32 workgroups of an XCD 2.7 row panels x ALL column
        // tiles per round -- the whole W (4.7 MB) plus 1 MB of A against a 4 MB L2, so W is pulled through the fabric again every
        // round.  Groups of raster_gm row panels, walked column-major inside the group: a round is raster_gm row panels x
        // 32 / raster_gm column tiles, and the next rounds keep the same row panels.
        const int per = a.raster_gm * tiles_n, grp = bid / per, rem = bid - grp * per;
        const int left = tiles_m - grp * a.raster_gm, gm = left < a.raster_gm ? left : a.raster_gm;
        m0 = (grp * a.raster_gm + rem % gm) * TILE_ROWS;
        n0 = (rem / gm) * BN;
        return;
    }
    m0 = (bid / tiles_n) * TILE_ROWS;
    n0 = (bid % tiles_n) * BN;
}

// ---- work item -----------------------------------------------------------------------------------------------------------------
// What a persistent workgroup of gemm_pp_kernel takes per turn: a tile, or with split-K a (tile, K slice) pair (its `decode`).
struct WorkItem {
    int tile;       // tile number (tile_origin's id)
    int slice;      // K slice, -1: whole K
    int kt0, nt;    // first K-tile and K-tile count
};

// ---- folded-LayerNorm row table ------------------------------------------------------------------------------------------------
// (rstd, rstd * mean) of a tile's rows, one row per thread, into an LDS table the epilogue reads (its st_lds).  A loop with work to
// put in between asks for its row's partial pairs early (row_stat_request of gemm_epi.h: at most four) and calls fold_publish when
// it needs the table; the others call fold_rows.  Every thread of the workgroup calls either: both end in the fence / barrier /
// fence that makes the table visible.
__device__ __forceinline__ void lds_table_visible() {      // what the threads of a workgroup wrote to LDS, to all of them
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// Thread t < rows finishes row m0 + t into table[t].  many: the launch has more than four partial pairs per row (EVA02's fc2: 22, one
// per 256-column tile of the SwiGLU launch) and nothing was requested: row_stat sums them now, in index order (deterministic), 8
// loads in flight.  (t < rows stands in both arms: as one flag passed in, the 224- and 192-row GELU kernels' s_waitcnt counts moved.)
__device__ __forceinline__ void fold_publish(const GemmArgs& a, int m0, int t, int rows, bool many, const float2 (&pv)[4], float2* table) {
    if (many) {
        if (t < rows) table[t] = row_stat(a, m0 + t);
    } else if (t < rows) table[t] = row_stat_finish(a, pv);
    lds_table_visible();
}
// Request and finish back to back: every thread of the workgroup takes row m.  MANY: built with the arm for more than four partial
// pairs; the dw loop's launches never have that many (gemm_plan.h).  (One branch around both steps, not fold_publish behind a
// request under a branch of its own: that form spilled 30 to 110 registers more in the 4-wave kernels.)
template <bool MANY>
__device__ __forceinline__ void fold_rows(const GemmArgs& a, int m, float2* table, int t) {
    if (MANY && a.stat_in_blocks > 4) {
        table[t] = row_stat(a, m);
    } else {
        float2 pv[4];
        row_stat_request(a, m, pv);
        table[t] = row_stat_finish(a, pv);
    }
    lds_table_visible();
}

// ---- staged epilogue -------------------------------------------------------------------------------------------------------------
// The epilogues with an LDS-staged form (gemm_epilogue_staged) ...
__host__ __device__ constexpr bool staged_epilogue_built(int epi) {
    return epi == EPI_VT || epi == EPI_GELU || epi == EPI_STAR || epi == EPI_QK || epi == EPI_QK_ROPE || epi == EPI_SWIGLU;
}
// ... and whether this launch's outputs are aligned for it: whole eight-token groups (V^T), whole heads (q | k | v), 16-byte row
// pieces (the rest; SWIGLU: N % 16 == 0 makes N and its output width N / 2 agree).  The pp and dw loops and launch_gemm's
// precondition for a folded LayerNorm all ask here, so host and device cannot drift apart.
__host__ __device__ __forceinline__ bool staged_epilogue_ok(int epi, const GemmArgs& a) {
    return epi == EPI_VT                            ? (a.tokens % 8 == 0 && a.tokens_pad % 8 == 0)
           : (epi == EPI_QK || epi == EPI_QK_ROPE) ? (a.dim % 64 == 0)
                                                    : ((a.ld_out ? a.ld_out : a.N) % 8 == 0);
}

// ---- one K-tile of the ping-pong loop: the multiply of a phase ---------------------------------------------------------------------
// HIPTS_MFMA_ORDER (measurement): (row block i, column block j) of the ij-th of a phase's 16 MFMAs.  0 = rows outer (the A fragment stays
// for four MFMAs), 1 = snake (every MFMA shares one operand with its predecessor), 2 = columns outer (the W fragment stays)
__device__ __forceinline__ void mfma_order(int ij, int& i, int& j) {
#if HIPTS_MFMA_ORDER == 2
    j = ij >> 2, i = ij & 3;
#elif HIPTS_MFMA_ORDER == 1
    i = ij >> 2, j = (i & 1) ? 3 - (ij & 3) : (ij & 3);
#else
    i = ij >> 2, j = ij & 3;
#endif
}

// The products of phase p: 16 MFMAs 16x16x32 (e4m3: 4 x 2 of 16x16x128) onto the accumulators of its m-half.  FIRST: the phases that touch
// an accumulator block first multiply onto a literal zero.
template <int EPI, int MR, bool F16, bool OP8, bool FIRST>
__device__ __forceinline__ void pp_multiply(int p, f32x4 (&acc)[MR][4], const bf16x8 (&wf)[2][4], const bf16x8 (&af)[4], const i32x8 (&wf8)[4],
                                            const i32x8 (&af8)[4], int scale_w, int scale_1) {
    const int mh = p >> 1, kk = p & 1;
    if constexpr (OP8) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const int j = 2 * kk + jj;
                const f32x4 c = FIRST ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[mh * 4 + i][j];
                if constexpr (EPI == EPI_VT)
                    acc[mh * 4 + i][j] = mfma_16x16x128_e4m3(af8[i], wf8[j], c, scale_1, scale_w);
                else
                    acc[mh * 4 + i][j] = mfma_16x16x128_e4m3(wf8[j], af8[i], c, scale_w, scale_1);
            }
    } else {
#pragma unroll
        for (int ij = 0; ij < 16; ++ij) {
            int i, j;
            mfma_order(ij, i, j);
            if (mh * 4 + i >= MR) continue;
            const f32x4 c = (FIRST && kk == 0) ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[mh * 4 + i][j];
            if constexpr (EPI == EPI_VT)
                acc[mh * 4 + i][j] = mfma_16x16x32<F16>(af[i], wf[kk][j], c);
            else
                acc[mh * 4 + i][j] = mfma_16x16x32<F16>(wf[kk][j], af[i], c);
        }
    }
}
