"""The folded LayerNorm as a chain: inputs, float64 reference and a float32 emulation (pure numpy, no GPU).

A residual GEMM (EPI_RESID_XG / XGI; EVA02's inner norm: EPI_SWIGLU) writes x, the 16-bit operand 16bit(gamma x) and per 256-column tile a
float32 pair (sum x, sum x^2); the consumer GEMM computes rstd (W (gamma x)) - rstd mean u + c with u = W gamma, c = W beta + b
(fold_ln_kernel) and (rstd, rstd mean) from the pairs (ln_stat_pair, or rowstat_kernel).  tests/test_ln_fold_host.py holds this module's
reference and bound (gemm_epi_ref.fold_bound) to a float32 emulation of the chain; tests/test_gpu_ln_fold.py runs the chain on the device:
call 1 the producer, call 2 the consumer on exactly what call 1 wrote.

Rows: every launch holds every regime, dealt cyclically (row r: regime r % len), so every 16-row block holds each.  Two kinds of input:
  grid     x = scale (m + k q), k integer, q = 2^-3 (IEEE half) / 2^-2 (bf16), gamma in {1/2, 1, 2}: the 16-bit copy IS gamma x and every
           float32 partial sum is exact in any order (sum x^2 / (scale q)^2 < 2^24), so the bound has no operand-rounding term and no
           summation term -- grid_preconditions() asserts both;
  generic  random rows, gamma ~ U(0.5, 1.5), a real product in the producer; additionally |mean| / sigma = 64."""
import numpy as np

import gemm_epi_ref as R

M = 272                 # one 256-row tile plus a ragged 16
EPS = 1e-6
U = R.U
F32 = np.float32

# (name, |mean| / sigma, log2 scale, outlier in sigmas, outlier's column tile, constant value or None)
GRID_REGIMES = [("ms0", 0, 0, 0, None, None), ("ms1", 1, 0, 0, None, None), ("ms4", 4, 0, 0, None, None), ("ms8", 8, 0, 0, None, None),
                ("ms16", 16, 0, 0, None, None), ("out30-first", 0, 0, 30, "first", None), ("out300-first", 0, 0, 300, "first", None),
                ("out30-last", 0, 0, 30, "last", None), ("out300-last", 0, 0, 300, "last", None), ("ms4-scale-8", 4, -8, 0, None, None),
                ("ms4-scale+10", 4, 10, 0, None, None), ("const0", 0, 0, 0, None, 0.0), ("const2", 0, 0, 0, None, 2.0)]
GENERIC_REGIMES = GRID_REGIMES + [("ms64", 64, 0, 0, None, None)]
assert len(GENERIC_REGIMES) <= 16


def regimes(kind):
    return GRID_REGIMES if kind == "grid" else GENERIC_REGIMES


def regime_of_row(kind, m=M):
    return np.arange(m) % len(regimes(kind))


# ---- the 16-bit operand types ------------------------------------------------------------------------------------------------------
def to16(x32, f16):
    """(bit patterns, widened float64) of float32 values rounded to nearest even in the operand type"""
    x32 = np.ascontiguousarray(x32, F32)
    if f16:
        with np.errstate(over="ignore"):
            h = x32.astype(np.float16)
        return h.view(np.uint16), h.astype(np.float64)
    u = x32.view(np.uint32)
    bits = ((u + np.uint32(0x7FFF) + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return bits, from16(bits, 0)


def from16(bits, f16):
    bits = np.ascontiguousarray(bits, np.uint16)
    if f16:
        return bits.view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << 16).view(F32).astype(np.float64)


def e16(f16):
    return 2.0 ** -11 if f16 else 2.0 ** -8


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
def grid_q(f16):
    return 2.0 ** -3 if f16 else 2.0 ** -2


def outlier_column(D, tile):
    return 5 if tile == "first" else D - 3


def rows(kind, D, f16, seed, m_max=16.0, m=M):
    """(x float32 [m][D], scale [m]: the power of two a row is scaled by)  --  the rows as the LayerNorm is to see them.
    grid: k uniform in [-r, r] with r the largest integer whose sigma q sqrt(r (r + 1) / 3) stays below min(1, 0.75 m_max / ms), centre
    the largest multiple of q below ms sigma: |k| <= 3 / q and centre <= m_max hold (m_max: 16, or 8 for the 2730-wide rows)."""
    rng = np.random.default_rng(seed)
    x = np.zeros((m, D))
    scale = np.ones(m)
    q = grid_q(f16)
    for r, ri in enumerate(regime_of_row(kind, m)):
        name, ms, lg, out, tile, const = regimes(kind)[ri]
        scale[r] = 2.0 ** lg
        if const is not None:
            x[r] = const
            continue
        if kind == "grid":
            target = min(1.0, 0.75 * m_max / ms) if ms else 1.0
            rr = max(k for k in range(1, int(3 / q) + 1) if q * np.sqrt(k * (k + 1) / 3.0) <= target)
            sigma = q * np.sqrt(rr * (rr + 1) / 3.0)
            centre = np.floor(ms * sigma / q) * q
            assert centre <= m_max
            x[r] = centre + q * rng.integers(-rr, rr + 1, D)
            if out:
                x[r, outlier_column(D, tile)] = float(out)
        else:
            x[r] = ms + rng.standard_normal(D)
            if out:
                x[r, outlier_column(D, tile)] = float(out)
        x[r] *= scale[r]
    return x.astype(F32), scale


def vectors(kind, D, N, seed, with_beta=True):
    """gamma [D], beta [D] or None, b [N] or None (the CAFormer's norms have no beta and its Linears no bias), float32"""
    rng = np.random.default_rng(seed)
    gamma = rng.choice([0.5, 1.0, 2.0], D) if kind == "grid" else rng.uniform(0.5, 1.5, D)
    beta = rng.standard_normal(D) * 0.1
    b = rng.standard_normal(N) * 0.1
    if not with_beta:
        return gamma.astype(F32), None, None
    return gamma.astype(F32), beta.astype(F32), b.astype(F32)


def weight(N, K, f16, seed, std=0.02):
    """(float32 W before rounding, bit patterns, widened float64) of a Linear's weight [N][K]"""
    w32 = (np.random.default_rng(seed).standard_normal((N, K)) * std).astype(F32)
    bits, w64 = to16(w32, f16)
    return w32, bits, w64


def grid_preconditions(x32, scale, gamma, f16, tile=256):
    """both must hold for the grid kind: (copy exact, every float32 partial sum exact)"""
    gx = x32 * gamma[None, :]                                            # float32 product of exact operands
    copy_exact = np.array_equal(gx.astype(np.float64), x32.astype(np.float64) * gamma.astype(np.float64)[None, :]) and \
        np.array_equal(to16(gx, f16)[1], gx.astype(np.float64))
    unit = (scale * grid_q(f16))[:, None]
    k = x32.astype(np.float64) / unit
    sums_exact = np.array_equal(k, np.round(k)) and float(((k * k).sum(1)).max()) < 2.0 ** 24 and float(np.abs(k).sum(1).max()) < 2.0 ** 24
    return copy_exact, sums_exact


# ---- the fold's two vectors (fold_ln_kernel) -----------------------------------------------------------------------------------------
def fold_vectors64(w64, gamma, beta, bias):
    """u = W gamma, c = W beta + b in float64 from the 16-bit values of W, and the magnitudes sum |W gamma|, sum |W beta| + |b|"""
    g = gamma.astype(np.float64)
    u, mu = w64 @ g, np.abs(w64) @ np.abs(g)
    c, mc = np.zeros(len(u)), np.zeros(len(u))
    if beta is not None:
        c, mc = w64 @ beta.astype(np.float64), np.abs(w64) @ np.abs(beta.astype(np.float64))
    if bias is not None:
        c, mc = c + bias.astype(np.float64), mc + np.abs(bias.astype(np.float64))
    return u, c, mu, mc


def fold_vector_bound(val, mag, K):
    """|got - val| <= 2^-24 |val| + K 2^-53 mag: the kernel sums in double and rounds once to float32"""
    return 2.0 ** -24 * np.abs(val) + K * 2.0 ** -53 * mag


# ---- float64 reference -----------------------------------------------------------------------------------------------------------------
def moments64(x, eps=EPS, ln_dim=None):
    """row moments of x [m][D] (float64, two passes) in the record gemm_epi_ref.fold_bound reads"""
    x = x.astype(np.float64)
    D = ln_dim or x.shape[1]
    mean = x.sum(1, keepdims=True) / D
    ex2 = (x * x).sum(1, keepdims=True) / D
    var = ((x - mean) ** 2).sum(1, keepdims=True) / D - (mean ** 2) * (x.shape[1] - D) / D      # columns past D are zero pads
    return dict(rstd=1.0 / np.sqrt(var + eps), mean=mean, ex2=ex2, var_eps=var + eps, absmean=np.abs(x).sum(1, keepdims=True) / D, given=False)


def reference_z(x, copy64, w64, gamma, beta, bias, kind, blocks, f16, eps=EPS, ln_dim=None):
    """Linear(LayerNorm(x)) in float64 from the producer's rows x and the 16-bit values of W -- never through the folded formula -- as a Q
    whose bound is gemm_epi_ref.fold_bound for the operand copy64 the consumer was handed.  Columns of x past ln_dim are zero pads."""
    x = x.astype(np.float64)
    st = moments64(x, eps, ln_dim)
    st["n_s"] = 0 if kind == "grid" else 256 + blocks + 4
    D = ln_dim or x.shape[1]
    live = (np.arange(x.shape[1]) < D)[None, :]
    g = gamma.astype(np.float64)[None, :]
    ln = np.where(live, (x - st["mean"]) * st["rstd"] * g + (beta.astype(np.float64)[None, :] if beta is not None else 0.0), 0.0)
    u, c, _, _ = fold_vectors64(w64, gamma, beta, bias)
    z = ln @ w64.T + (bias.astype(np.float64)[None, :] if bias is not None else 0.0)
    acc, S = copy64 @ w64.T, np.abs(copy64) @ np.abs(w64).T
    K = x.shape[1]
    b = R.fold_bound(z, c[None, :], acc, S, u[None, :], st, K, 0.0 if kind == "grid" else e16(f16))
    return R.Q(z, np.abs(z), 2, b - 2.0 * U * np.abs(z)), st


def perturbation_bound(dx, x, z, c, w64, gamma, st, ln_dim):
    """How far Linear(LayerNorm(.)) moves when its rows move by at most dx (first order): with Wg = W gamma and D = ln_dim,
    d z_n / d x_j = rstd (Wg_nj - u_n / D) - (z_n - c_n) rstd^2 (x_j - mean) / D.  For the chain behind EPI_SWIGLU, whose float32 rows the
    launch does not return: the reference takes the rows read back from the 16-bit copy (rows_of_copy) and this is its own error.
    Columns past ln_dim are zero pads (dx = 0).  tests/test_ln_fold_host.py holds it to float64 rows moved by dx."""
    wg = np.abs(w64 * gamma.astype(np.float64)[None, :])
    u = np.abs(w64 @ gamma.astype(np.float64))[None, :]
    return st["rstd"] * (dx @ wg.T + u * dx.sum(1, keepdims=True) / ln_dim) + \
        np.abs(z - c) * st["rstd"] ** 2 * (np.abs(x - st["mean"]) * dx).sum(1, keepdims=True) / ln_dim


def rows_of_copy(copy_bits, gamma, f16, ln_dim):
    """(x^, dx) float64: the rows a producer normalised, read back from the 16-bit copy it wrote, where the launch does not return them
    in float32 (EPI_SWIGLU).  copy = 16bit(float32(gamma x)), so x^ = copy / gamma holds x to dx = (e16 + 2 U) |x^|, for IEEE half plus
    half the subnormal quantum 2^-24 over |gamma|.  Columns past ln_dim (gamma = 0, the copy 0) are zero pads with dx = 0."""
    c = from16(copy_bits, f16)
    g = gamma.astype(np.float64)[None, :]
    live = (np.arange(c.shape[1]) < ln_dim)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.where(live, c / g, 0.0)
        dx = np.where(live, (e16(f16) + 2.0 * U) * np.abs(x) + (2.0 ** -25 / np.abs(g) if f16 else 0.0), 0.0)
    return x, dx


def pair_bound(x, dx, tile):
    """(sums [tiles][m][2], bound) of the float32 pairs (sum x, sum x^2) per `tile` columns a producer wrote of float32 rows within dx
    of x: the rows' own distance, sum dx and sum (2 |x| + dx) dx, and tile + 4 float32 roundings of the magnitude (a square rounds once
    more than a sum's term)."""
    m, D = x.shape
    tiles = (D + tile - 1) // tile
    pad = lambda a: np.pad(a, ((0, 0), (0, tiles * tile - D))).reshape(m, tiles, tile)
    xt, dt = pad(x), pad(dx)
    n = tile + 4
    val = np.stack([xt.sum(2), (xt * xt).sum(2)], -1)
    b = np.stack([dt.sum(2) + n * U * (np.abs(xt) + dt).sum(2), ((2.0 * np.abs(xt) + dt) * dt).sum(2) + (n + 1) * U * ((np.abs(xt) + dt) ** 2).sum(2)], -1)
    return val.transpose(1, 0, 2), b.transpose(1, 0, 2)


def ratio(got, want, bound):
    """|got - want| / bound per element; where the bound is 0 (a zero row with no beta: the answer is exactly 0) 0 if met, else inf"""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))


# ---- float32 emulation of the chain ----------------------------------------------------------------------------------------------------
def tile_sums32(x32, tile=256):
    """[tiles][m][2] float32: (sum x, sum x^2) per row and `tile` columns, float32 additions (numpy's pairwise order)"""
    m, D = x32.shape
    tiles = (D + tile - 1) // tile
    xp = np.zeros((m, tiles * tile), F32)
    xp[:, :D] = x32
    xp = xp.reshape(m, tiles, tile)
    part = np.stack([xp.sum(2, dtype=F32), (xp * xp).sum(2, dtype=F32)], -1)
    return np.ascontiguousarray(part.transpose(1, 0, 2))


def finish32(part, ln_dim, eps=EPS, divide=False):
    """(rstd, rstd mean) float32 [m] from [blocks][m][2]: blocks added in index order, then ln_stat_pair (divide: rowstat_kernel's s / D)"""
    s1, s2 = np.zeros(part.shape[1], F32), np.zeros(part.shape[1], F32)
    for b in range(part.shape[0]):
        s1, s2 = s1 + part[b, :, 0], s2 + part[b, :, 1]
    if divide:
        mean, m2 = s1 / F32(ln_dim), s2 / F32(ln_dim)
    else:
        inv = F32(1.0) / F32(ln_dim)
        mean, m2 = s1 * inv, s2 * inv
    var = np.maximum(m2 - mean * mean, F32(0.0))
    rstd = F32(1.0) / np.sqrt(var + F32(eps))
    return rstd, rstd * mean


def emulate(x32, gamma, w64, u32, c32, f16, ln_dim=None, part=None, tile=256):
    """the chain in float32: the producer's copy and sums of x32, the finish, the consumer's  acc rstd + (c - u rstd mean)"""
    copy_bits, copy64 = to16(x32 * gamma[None, :], f16)
    part = tile_sums32(x32, tile) if part is None else part
    rstd, rm = finish32(part, ln_dim or x32.shape[1])
    acc = copy64.astype(F32) @ w64.astype(F32).T
    z = acc * rstd[:, None] + (c32[None, :] - u32[None, :] * rm[:, None])
    return z, copy64, part


# ---- the wirings of the three forwards ---------------------------------------------------------------------------------------------------
# geometry: D columns of the consumer's operand (its K), ln_dim of them live, one pair per `tile` of them, grid centres up to m_max
GEOMETRY = {
    "vit": dict(model="vit_b16_448", D=768, ln_dim=768, tile=256, m_max=16.0, beta=True),
    "eva": dict(model="eva02_l14_448", D=1024, ln_dim=1024, tile=256, m_max=16.0, beta=True),
    "eva_fc2": dict(model="eva02_l14_448", D=2752, ln_dim=2730, tile=128, m_max=8.0, beta=True),      # 22 pairs over 2730 of 43 x 64 columns
    "ccip": dict(model="ccip_b36_384", D=512, ln_dim=512, tile=256, m_max=16.0, beta=False),
}
_RX = R.STAT_PART | R.COPY16
# (id, geometry, producer (epilogue, features, x_blocked), consumer (epilogue, features, x_blocked, N), how the pairs reach the consumer)
WIRINGS = [
    ("vit-xg-qkv", "vit", (R.RESID_XG, _RX | R.SK_WS, 1), (R.QK, R.STAT_IN, 0, 384), "stat_in"),
    ("vit-xg-gelu", "vit", (R.RESID_XG, _RX | R.SK_WS, 1), (R.GELU, R.STAT_IN, 0, 384), "stat_in"),
    ("eva-xg-qkrope", "eva", (R.RESID_XG, _RX | R.SK_WS, 1), (R.QK_ROPE, R.STAT_IN, 0, 384), "stat_in"),
    ("eva-xgi-qkrope", "eva", (R.RESID_XGI, _RX | R.SK_WS | R.STAT_IN, 1), (R.QK_ROPE, R.STAT_IN, 0, 384), "stat_in"),
    ("eva-xg-swiglu", "eva", (R.RESID_XG, _RX | R.SK_WS, 1), (R.SWIGLU, R.STAT_PART | R.STAT_IN | R.LDOUT, 0, 512), "stat_in"),
    ("eva-swiglu-rowstat", "eva_fc2", (R.SWIGLU, R.STAT_PART | R.STAT_IN | R.LDOUT, 0), (R.RESID_ROWSTAT, R.STAT_IN | R.SK_WS | R.ROWMAJOR, 1, 384), "stat_in"),
    ("eva-swiglu-rowstat-kernel", "eva_fc2", (R.SWIGLU, R.STAT_PART | R.STAT_IN | R.LDOUT, 0), (R.RESID_ROWSTAT, R.STAT_IN | R.SK_WS | R.ROWMAJOR, 1, 384), "rowstat"),
    ("eva-swiglu-xgi", "eva_fc2", (R.SWIGLU, R.STAT_PART | R.STAT_IN | R.LDOUT, 0), (R.RESID_XGI, _RX | R.SK_WS | R.STAT_IN, 1, 384), "stat_in"),
    ("eva-swiglu-xgi-kernel", "eva_fc2", (R.SWIGLU, R.STAT_PART | R.STAT_IN | R.LDOUT, 0), (R.RESID_XGI, _RX | R.SK_WS | R.STAT_IN, 1, 384), "rowstat"),
    ("ccip-xg-star", "ccip", (R.RESID_XG, _RX | R.RES_SCALE, 0), (R.STAR, R.STAT_IN, 0, 384), "stat_in"),
    ("ccip-xg-qk", "ccip", (R.RESID_XG, _RX | R.RES_SCALE, 0), (R.QK, R.STAT_IN, 0, 256), "stat_in"),
    ("ccip-xg-vt", "ccip", (R.RESID_XG, _RX | R.RES_SCALE, 0), (R.VT, R.STAT_IN, 0, 256), "stat_in"),
]


def blocks_of(geom):
    g = GEOMETRY[geom]
    return (g["D"] + g["tile"] - 1) // g["tile"]


def launches_hold(wiring):
    """gemm_epi_ref.LAUNCHES is the authority: the wiring's producer and consumer are launches of its model, with these features (the
    consumer's width aside: the tests take one or two column tiles of it)"""
    _, geom, (pe, pf, pxb), (ce, cf, cxb, _), _ = wiring
    launches = R.MODELS[GEOMETRY[geom]["model"]][3]
    has = lambda e, f, xb: any(r[2] == e and r[6] == f and r[7] == xb for r in launches)
    return has(pe, pf, pxb) and has(ce, cf, cxb)
