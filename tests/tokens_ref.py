"""Host restatements of the small kernels at the head and tail of the five forwards -- token assembly (eva.hip), patch merging, hi | lo rows
and token mean (swinv2.hip), the 3 x 3 s2 patch matrix (ccip.hip), the 16-bit copy (convnext.hip), the two pools with partial sums (vit.hip:
pool_partial_kernel + pool_finalize_kernel; eva.hip: eva_colsum_kernel) -- for tests/test_tokens_host.py (CPU) and tests/test_gpu_tokens.py
(one launch per case through the hiptsdbg_* entries beside the kernels).  Each function is written from the operation's definition: reshapes
and transposes, a zero-padded array and strided slices, a concatenation, a matrix of which token belongs to which partial sum.  The 16-bit
conversions, the hi | lo split, the blocked layout, the exact-answer constructions and the float64 / float32 LayerNorm forms are those of
tests/rows_ref.py.

A `*_expected` function returns the WHOLE buffer an entry hands back when it was given GUARD bytes more than the launch's extent and
fill = 0xff: the launch's words, then the guard still holding the fill.

The pools come in a float64 form and a float32 form of the same formula (rows_ref.pool_ln64 / pool_ln32 are the pattern).  Which token a
partial sum contains is a 0 / 1 matrix (assign); the mutants of tests/test_tokens_host.py are edits of that matrix.
"""
import numpy as np

import rows_ref as R

F32 = np.float32
GUARD = 256                                   # guard bytes behind every output buffer
FILL16, FILL32 = 0xFFFF, 0xFFFFFFFF           # what fill = 0xff leaves in 16-bit / 32-bit words: NaNs no case produces
EVA_SPLITS = 16                               # eva.hip POOL_SPLITS


# ---- buffers ---------------------------------------------------------------------------------------------------------------------------
def words(x):
    """float32 values as their bit patterns"""
    return np.ascontiguousarray(x, F32).view(np.uint32).ravel()


def guard16(body):
    return np.concatenate([np.ascontiguousarray(body, np.uint16).ravel(), np.full(GUARD // 2, FILL16, np.uint16)])


def guard32(body):
    return np.concatenate([np.ascontiguousarray(body, np.uint32).ravel(), np.full(GUARD // 4, FILL32, np.uint32)])


def hilo_rows(v, f16):
    """[..., D] float32 -> 16-bit patterns [..., hi(D) | lo(D)]"""
    return np.concatenate(R.split_hilo(v, f16), -1)


def distinct_f32(n, seed):
    """n float32 values, pairwise distinct, of both signs, magnitudes in [1, 2), the last mantissa bit set: none is a value of either
    16-bit type, so every lo half is non-zero"""
    v = (1.0 + (np.random.default_rng(seed).permutation(n) + 0.37) / n).astype(F32)
    v = (v.view(np.uint32) | np.uint32(1)).view(F32) * np.where(np.arange(n) % 2, F32(-1), F32(1))
    assert np.unique(v).size == n
    for f16 in (0, 1):
        assert np.all(R.from_op(R.split_hilo(v, f16)[1], f16) != 0)
    return v


def distinct_u16(n, seed):
    """n 16-bit patterns, pairwise distinct, none zero"""
    assert n < 65535
    return (np.random.default_rng(seed).permutation(65535)[:n] + 1).astype(np.uint16)


# ---- copies, gathers, casts ------------------------------------------------------------------------------------------------------------
def merge_rows(x, swap=False):
    """SwinV2 patch merging's gather, x [B][H][H][C] -> [B (H/2)^2][4 C]: timm's reshape(B, H/2, 2, W/2, 2, C).permute(0, 1, 3, 4, 2, 5),
    columns in (dx, dy, c) order.  swap: (dy, dx, c), the mutant."""
    B, H, _, C = x.shape
    Ho = H // 2
    perm = (0, 1, 3, 2, 4, 5) if swap else (0, 1, 3, 4, 2, 5)
    return np.ascontiguousarray(x.reshape(B, Ho, 2, Ho, 2, C).transpose(perm)).reshape(B * Ho * Ho, 4 * C)


def merge_expected(x, f16, swap=False):
    return guard16(hilo_rows(merge_rows(np.ascontiguousarray(x, F32), swap), f16))


def split_x_expected(x, f16):
    return guard16(hilo_rows(np.ascontiguousarray(x, F32), f16))


def im2col_rows(xn, pad_bottom_right=True):
    """3 x 3 stride-2 pad-1 patches, xn [B][H][H][C] -> [B (H/2)^2][9 C], tap (ky, kx) at columns (3 ky + kx) C ..: a zero-padded array and
    nine strided slices.  For an even H the last window ends at row 2 (H/2 - 1) - 1 + 2 = H - 1: the padding below and to the right is
    never read, so an array padded at the top and left only (pad_bottom_right=False) gives the same matrix."""
    B, H, _, C = xn.shape
    Ho = H // 2
    side = H + 2 if pad_bottom_right else H + 1
    p = np.zeros((B, side, side, C), xn.dtype)
    p[:, 1:H + 1, 1:H + 1] = xn
    taps = [p[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Ho:2] for ky in range(3) for kx in range(3)]
    return np.stack(taps, 3).reshape(B * Ho * Ho, 9 * C)


def im2col_expected(xn):
    return guard16(im2col_rows(xn))


def cast_expected(x, f16):
    return guard16(R.to_op(x, f16))


def cast_values(n4):
    """4 n4 float32 values: the edge cases of both 16-bit types first (as far as there is room), ordinary numbers behind them.  Per type:
    ties between two neighbours with an odd and an even one below, and the float32 values next to those ties; the smallest subnormal, ties
    between subnormals, half of the smallest subnormal (a tie that goes to zero) and the float32 value just above it, a quarter of it;
    the smallest normal and values just below it that round up to it; the largest finite value, the largest float32 value that still rounds
    to it, and the halfway point above it, which rounds to infinity.  Then +-0, the float32 extremes, float32 subnormals.  All with both signs."""
    def near(v, up):
        return np.nextafter(F32(v), F32(np.inf if up else 0))

    edge = []
    for mant, emin, emax in ((10, -14, 15), (7, -126, 127)):
        ulp1, sub = 2.0 ** -mant, 2.0 ** (emin - mant)
        for tie in (1 + 0.5 * ulp1, 1 + 1.5 * ulp1, 1.5 * sub, 2.5 * sub, 0.5 * sub, 2.0 ** emin * (1 - 2.0 ** -(mant + 1))):
            edge += [F32(tie), near(tie, True), near(tie, False)]
        edge += [F32(sub), F32(0.25 * sub), F32(37.5 * sub), F32(2.0 ** emin), near(2.0 ** emin, False)]
        top, half = (2 - ulp1) * 2.0 ** emax, (2 - 0.5 * ulp1) * 2.0 ** emax
        edge += [F32(top), near(top, True), near(half, False), F32(half)]
    edge += [F32(0), np.finfo(F32).max, np.finfo(F32).tiny, F32(2.0 ** -149), F32(2.0 ** -140)]
    edge = np.array(edge, F32)
    assert np.all(np.isfinite(edge))
    edge = np.concatenate([edge, -edge])
    rng = np.random.default_rng(n4)
    body = (rng.standard_normal(4 * n4) * 10.0 ** rng.integers(-6, 5, 4 * n4)).astype(F32)
    k = min(edge.size, 4 * n4)
    body[:k] = edge[:k]
    return body


def assemble_rows(tmp, cls, pos0, TS):
    """EVA token assembly, tmp [B][np][D] -> [B][TS][D]: [cls + pos[0] | the patch rows | zero rows up to TS]"""
    tmp = np.ascontiguousarray(tmp, F32)
    B, n, D = tmp.shape
    head = np.broadcast_to((np.asarray(cls, F32) + np.asarray(pos0, F32))[None, None, :], (B, 1, D))          # one float32 addition
    return np.concatenate([head, tmp, np.zeros((B, TS - 1 - n, D), F32)], 1)


def assemble_expected(tmp, cls, pos0, TS, blocked):
    """(the row-major buffer, the blocked buffer): the blocked copy has whole 16-row blocks; rows of the last block past batch * TS belong
    to nobody and keep the fill.  blocked == 0: the second buffer is GUARD bytes of fill."""
    x = assemble_rows(tmp, cls, pos0, TS)
    M, D = x.shape[0] * TS, x.shape[2]
    if not blocked:
        return guard32(words(x)), np.full(GUARD // 4, FILL32, np.uint32)
    blk = np.full((M + 15) // 16 * 16 * D + GUARD // 4, FILL32, np.uint32)
    blk[R.blocked_offsets(M, D).ravel()] = words(x)
    return guard32(words(x)), blk


# ---- pools: which row belongs to which partial sum ------------------------------------------------------------------------------------------
def assign(batch, rows, first, count, splits):
    """A [batch * splits][batch * rows] of 0 / 1: row first + r (r < count) of image b is summed into split r // per of image b, per =
    ceil(count / splits).  A split past the last token owns nothing: its partial sum is zero."""
    per = -(-count // splits)
    A = np.zeros((batch * splits, batch * rows))
    for b in range(batch):
        for r in range(count):
            A[b * splits + r // per, b * rows + first + r] = 1
    return A


def partial64(y, A, splits):
    """y [batch][rows][D] -> [batch][splits][D], partial = A y in float64"""
    batch, rows, D = y.shape
    return (A @ np.asarray(y, np.float64).reshape(batch * rows, D)).reshape(batch, splits, D)


def partial32(y, first, count, splits):
    """the same sums in float32, each split's rows added in numpy's order"""
    y = np.asarray(y, F32)
    per = -(-count // splits)
    return np.stack([y[:, first + s * per:first + min(count, (s + 1) * per)].sum(1, dtype=F32) for s in range(splits)], 1)


def empty_splits(count, splits):
    per = -(-count // splits)
    return [s for s in range(splits) if s * per >= count]


def forward_splits(tokens):
    """hipts_vit_create's pool_splits (vit.hip; test_tokens_host.py finds the expression there)"""
    return min(32, max(8, tokens // 28)) if tokens >= 64 else 1


# ViT: final norm + mean pool
def vit_contrib64(x, eps, pool_then_norm):
    """what a token adds to its partial sum: itself (pool-then-norm) or (x - mean) * rstd (norm-then-pool: the affine follows the mean)"""
    x = np.asarray(x, np.float64)
    return x if pool_then_norm else R.layernorm64(x, 1.0, None, eps)


def vit_contrib32(x, eps, pool_then_norm):
    x = np.asarray(x, F32)
    return x if pool_then_norm else R.layernorm32(x, F32(1), None, eps, add_zero=False)


def vit_finalize64(part, g, b, eps, tokens, pool_then_norm):
    a = np.asarray(part, np.float64).sum(1) / tokens
    return R.layernorm64(a, g, b, eps) if pool_then_norm else a * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def vit_finalize32(part, g, b, eps, tokens, pool_then_norm):
    a = np.asarray(part, F32).sum(1, dtype=F32) / F32(tokens)
    return R.layernorm32(a, g, b, eps) if pool_then_norm else a * np.asarray(g, F32) + np.asarray(b, F32)


def vit_pool64(x, g, b, eps, pool_then_norm, splits, A=None):
    """x [batch][tokens][D] -> (partials [batch][splits][D], feature [batch][D])"""
    batch, T, _ = x.shape
    part = partial64(vit_contrib64(x, eps, pool_then_norm), assign(batch, T, 0, T, splits) if A is None else A, splits)
    return part, vit_finalize64(part, g, b, eps, T, pool_then_norm)


def vit_pool32(x, g, b, eps, pool_then_norm, splits):
    T = x.shape[1]
    part = partial32(vit_contrib32(x, eps, pool_then_norm), 0, T, splits)
    return part, vit_finalize32(part, g, b, eps, T, pool_then_norm)


def vit_pool_expected(part, feat, f16):
    return guard32(words(part)), guard16(hilo_rows(np.ascontiguousarray(feat, F32), f16))


# EVA: column sums over the patch rows, then rows_ref.pool_ln64 / pool_ln32 over the 16 partial rows with count = np
def eva_colsum64(x, n, A=None):
    batch, TS, _ = x.shape
    return partial64(x, assign(batch, TS, 1, n, EVA_SPLITS) if A is None else A, EVA_SPLITS)


def eva_colsum32(x, n):
    return partial32(x, 1, n, EVA_SPLITS)


# SwinV2: mean over tokens
def sw_mean64(y, A=None):
    batch, T, _ = y.shape
    return partial64(y, assign(batch, T, 0, T, 1) if A is None else A, 1)[:, 0] / T


def sw_mean32(y):
    y = np.asarray(y, F32)
    return y.sum(1, dtype=F32) / F32(y.shape[1])


# ---- the mutants: edits of an assignment matrix (tests/test_tokens_host.py) ---------------------------------------------------------------------
def mutant_drop_last(A):
    """the last token of the first non-empty split is not summed"""
    A = A.copy()
    row = next(i for i in range(A.shape[0]) if A[i].any())
    A[row, np.flatnonzero(A[row])[-1]] = 0
    return A


def mutant_double(A, which=0):
    A = A.copy()
    rows, cols = np.nonzero(A)
    k = which % rows.size
    A[rows[k], cols[k]] = 2
    return A


def mutant_move_first_of_image1(A, batch):
    """the first token of image 1 is summed into image 0's last non-empty split instead (its neighbour in memory)"""
    A = A.copy()
    per_image = A.shape[0] // batch
    col = np.flatnonzero(A[per_image:2 * per_image].any(0))[0]
    A[per_image:2 * per_image, col] = 0
    last = max(i for i in range(per_image) if A[i].any())
    A[last, col] = 1
    return A


def mutant_include(A, batch, splits, rows, row, split):
    """row `row` of every image is summed into its split `split` as well"""
    A = A.copy()
    for b in range(batch):
        A[b * splits + split, b * rows + row] = 1
    return A


# ---- inputs with exact answers ---------------------------------------------------------------------------------------------------------------
def vit_exact_tokens(batch, T, D, pool_then_norm, seed):
    """norm-then-pool: token t of image b is the row m_bt + s_bt r_bt u_b[c] (u_b a balanced sign pattern of the image, r_bt = +-1, m an
    integer, s a power of two): with eps = 0 its normalised row is exactly r_bt u_b, so a partial sum is u_b times an integer that every
    token changes by one, and the images' totals sum_t r_bt differ (as far as T + 1 values allow).
    pool-then-norm: rows_ref.exact_pool -- integer rows whose sum over all tokens is T (m_b +- s_b), so the pooled row normalises to exactly
    +-1; every partial sum is an exact integer, the rows of an image pairwise distinct."""
    if pool_then_norm:
        return R.exact_pool(batch, T, D, seed)[0]
    rng = np.random.default_rng(seed)
    u = R.balanced_signs(batch, D, seed + 1)
    r = -np.ones((batch, T), np.int64)
    for b in range(batch):
        r[b, rng.permutation(T)[:min(T, T // 2 + 1 + b)]] = 1                 # sum_t r_bt = 1 + 2 b or 2 + 2 b: another total per image
    m, s = rng.integers(-20, 21, (batch, T)), 2 ** rng.integers(0, 6, (batch, T))
    return (m[..., None] + (s * r)[..., None] * u[:, None, :]).astype(F32)


def eva_exact_rows(batch, n, TS, D, seed):
    """[batch][TS][D]: small integers in the patch rows 1 .. n, 1e30 in row 0 and in the pad rows"""
    x = np.full((batch, TS, D), 1e30, F32)
    x[:, 1:1 + n] = np.random.default_rng(seed).integers(-50, 51, (batch, n, D))
    return x


SW_MEAN_SCALE = 513.0 / 512.0


def sw_exact_tokens(batch, T, C, seed):
    """rows_ref.exact_pool times 513 / 512: every partial sum is an integer below 2^15 times 2^-9 (exact in float32), sum / T is exactly
    (m_b +- s_b) 513 / 512, which has more bits than either 16-bit type holds: the lo half is not zero everywhere"""
    x = R.exact_pool(batch, T, C, seed)[0].astype(np.float64) * SW_MEAN_SCALE
    assert np.array_equal(x.astype(F32).astype(np.float64), x) and np.abs(x).sum(1).max() * 512 < 2 ** 24
    return x.astype(F32)


# ---- the cases of tests/test_gpu_tokens.py; tests/test_tokens_host.py runs the mutants over the pooling ones -------------------------------------
MERGE_SHAPES = [(1, 2, 4), (2, 6, 96), (3, 4, 260)]                       # (batch, H, C)
SPLIT_ROWS, SPLIT_D = (1, 7, 65), (4, 96, 260)
IM2COL_SHAPES = [(1, 2, 8), (2, 4, 64), (2, 6, 72)]                       # (batch, H, C)
CAST_N4 = (1, 255, 257)
ASSEMBLE_SHAPES = [(1, 4, 5, 16), (2, 9, 13, 64), (3, 9, 16, 80)]         # (batch, np, TS, D): batch * TS = 5, 26, 48; TS == np + 1 in the first
ASSEMBLE_ROWMAJOR_ONLY = [(2, 4, 6, 4)]                                   # D = 4: no blocked copy
COLSUM_NP, COLSUM_PAD, COLSUM_D = (1, 10, 16, 37, 64), (1, 7), (4, 260, 1024)       # TS = np + pad
SW_MEAN_T, SW_MEAN_C = (1, 49, 64), (4, 260, 1024)
VIT_POOL_TS = [(1, 1), (63, 1), (64, 8), (70, 8), (70, 32), (196, 8), (196, 28)]          # (tokens, splits)
VIT_POOL_D = (4, 192, 260, 1024)
POOL_BATCH = 3
# statistics against float64: (tokens, splits, D) for the ViT pool, (np, TS, D) for the EVA chain, (T, C) for the SwinV2 mean
STAT_INPUT_KINDS = ("gauss", "offset")
VIT_STAT = [(196, 28, 768), (70, 8, 260)]
EVA_STAT = [(37, 40, 260)]
SW_STAT = [(49, 1024)]


OFFSET_RATIO = 64.0


def stat_tokens(kind, batch, T, D, seed):
    """'gauss': rows_ref.stat_rows.  'offset': its offset kind -- Gaussian rows of a spread s_t drawn from [0.5, 2] around a mean +-OFFSET_RATIO
    s_t -- with |mean| / spread = 2^6 instead of 2^10.  A pool divides the spread of what it sums by sqrt(T) and keeps the offsets, so behind
    a pool-then-norm the ratio is another 8 to 14 times larger; at 2^10 the float32 restatement's own error after that LayerNorm (E32 =
    3.4e-3 at 196 tokens) is wider than the spacing of IEEE half, and a kernel that never wrote the lo half would pass.  At 2^6 every mutant
    of tests/test_tokens_host.py is at least 6 bounds away; at 2^8 the nearest is 1.7."""
    if kind == "gauss":
        return R.stat_rows(kind, batch * T, D, seed).reshape(batch, T, D)
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((batch * T, D))
    std = rng.uniform(0.5, 2.0, (batch * T, 1))
    return (std * z + OFFSET_RATIO * std * rng.choice([-1.0, 1.0], (batch * T, 1))).astype(F32).reshape(batch, T, D)


def eva_stat_rows(kind, batch, n, TS, D, seed):
    x = np.full((batch, TS, D), 1e30, F32)
    x[:, 1:1 + n] = stat_tokens(kind, batch, n, D, seed)
    return x


# the inputs of a case, the same for the GPU test and for the mutants of the host test: (x, g, b, eps)
def vit_exact_case(T, splits, D, pool_then_norm):
    return (vit_exact_tokens(POOL_BATCH, T, D, pool_then_norm, 1000 * T + 10 * splits + D),) + R.gamma_beta(D) + (0.0,)


def vit_stat_case(kind, T, D):
    return (stat_tokens(kind, POOL_BATCH, T, D, 51),) + R.stat_affine(D, 52) + (R.STAT_KINDS[kind],)


def eva_exact_case(n, pad, D):
    return eva_exact_rows(2, n, n + pad, D, 100 * n + 10 * pad + D)


def eva_stat_case(kind, n, TS, D):
    return (eva_stat_rows(kind, 2, n, TS, D, 53),) + R.stat_affine(D, 54) + (R.STAT_KINDS[kind],)


def sw_exact_case(T, C):
    return sw_exact_tokens(POOL_BATCH, T, C, 100 * T + C)


def sw_stat_case(kind, T, C):
    return stat_tokens(kind, POOL_BATCH, T, C, 55)


# ---- which test launches which kernel on its own (tests/test_kernel_inventory_host.py) -------------------------------------------------------
TOKEN_KERNELS = ("pool_partial_kernel", "pool_finalize_kernel", "eva_assemble_kernel", "eva_colsum_kernel", "sw_merge_kernel", "sw_split_x_kernel",
                 "sw_mean_kernel", "ds_im2col_kernel", "cnx_cast_kernel")
