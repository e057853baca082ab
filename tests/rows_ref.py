"""Host restatements of the row kernels (csrc/row_ln.h, csrc/patch_rows.h and the two LDS-tiled uint8 stems), for tests/test_rows_host.py
(CPU) and tests/test_gpu_rows.py (one launch per case through csrc/rows_dbg.hip):
  * float64 references: layernorm64, pool_ln64;
  * float32 restatements of the kernels' own formula (two passes, three roundings), and a one-pass variant as a negative control;
  * the 16-bit conversions (round to nearest even) and the hi | lo split, as numpy float32 / integer arithmetic;
  * the index maps: blocked stream, 2 x 2 s2 patch matrix, the three windows' patch rows;
  * the input constructions whose answers are exact: rows of m +- s (exact_rows), pooled images (exact_pool);
  * the (source, affine, sink) / (pixel, window) tuples the forwards launch, as the GPU tests run them and test_rows_host.py finds them
    in the sources.
e4m3 packing is absent on purpose: no forward reaches launch_layernorm8 (test_rows_host.py asserts that), so ToE4m3 is not built into the
debug entry and has nothing to be compared with.
"""
import itertools

import numpy as np

F32 = np.float32

# ---- enumerators of include/hip_tagsearch_debug.h ---------------------------------------------------------------------------------------
SRC_F32, SRC_F32_BLOCKED, SRC_F32_INPLACE, SRC_16_BIAS = range(4)
AFF_GAMMA_BETA, AFF_GAMMA_OPT_BETA, AFF_GAMMA_ADD_ZERO, AFF_GAMMA_PLAIN = range(4)
SINK_16, SINK_E4M3, SINK_F32, SINK_F32_AND_16, SINK_PATCH2X2, SINK_ADD_HILO, SINK_BACK = range(7)
PIX_U8_AFFINE, PIX_U8_TABLE, PIX_F32_FLIP, PIX_F32, PIX_U8_RAW = range(5)
WIN_PATCH, WIN_4X4, WIN_7X7 = range(3)

# source text of a policy -> enumerator; what test_rows_host.py reads out of csrc/*.hip
SRC_NAMES = {"FromF32": SRC_F32, "FromF32Blocked": SRC_F32_BLOCKED, "F32InPlace": SRC_F32_INPLACE, "From16Bias": SRC_16_BIAS}
AFF_NAMES = {"LnGammaBeta": AFF_GAMMA_BETA, "LnGammaOptBeta": AFF_GAMMA_OPT_BETA, "LnGamma<true>": AFF_GAMMA_ADD_ZERO, "LnGamma<false>": AFF_GAMMA_PLAIN}
SINK_NAMES = {"To16": SINK_16, "ToE4m3": SINK_E4M3, "ToF32": SINK_F32, "ToF32And16": SINK_F32_AND_16, "ToPatch2x2": SINK_PATCH2X2,
              "AddToStreamHiLo": SINK_ADD_HILO, "BackToSource": SINK_BACK}
PIX_NAMES = {"PixelU8Affine": PIX_U8_AFFINE, "PixelU8Table": PIX_U8_TABLE, "PixelF32Planes<true>": PIX_F32_FLIP, "PixelF32Planes<false>": PIX_F32}
WIN_NAMES = {"WindowPatch": WIN_PATCH, "Window4x4": WIN_4X4, "Window7x7": WIN_7X7}

# The row_ln_kernel variants the GPU tests run: (id, source, affine, sink, has an operand type, blk, beta present)
ROW_LN_VARIANTS = [
    ("opt16_beta", SRC_F32, AFF_GAMMA_OPT_BETA, SINK_16, True, 0, True),
    ("opt16_nobeta", SRC_F32, AFF_GAMMA_OPT_BETA, SINK_16, True, 0, False),
    ("blocked16_add0", SRC_F32_BLOCKED, AFF_GAMMA_ADD_ZERO, SINK_16, True, 0, False),
    ("inplace_rowmajor", SRC_F32_INPLACE, AFF_GAMMA_PLAIN, SINK_BACK, False, 0, False),
    ("inplace_blocked", SRC_F32_INPLACE, AFF_GAMMA_PLAIN, SINK_BACK, False, 1, False),
    ("f32and16", SRC_F32, AFF_GAMMA_BETA, SINK_F32_AND_16, True, 0, True),
    ("patch2x2", SRC_F32, AFF_GAMMA_BETA, SINK_PATCH2X2, True, 0, True),
    ("from16bias", SRC_16_BIAS, AFF_GAMMA_BETA, SINK_16, True, 0, True),
    ("addhilo", SRC_F32, AFF_GAMMA_BETA, SINK_ADD_HILO, True, 0, True),
    ("tof32", SRC_F32, AFF_GAMMA_BETA, SINK_F32, False, 0, True),
]
ROW_LN_TUPLES = sorted({v[1:4] for v in ROW_LN_VARIANTS})
# pool_ln_kernel: (sink, has an operand type); patch_gather_kernel: (pixel, window)
POOL_SINKS = [("PooledF32", False), ("PooledHiLo", True)]
GATHER_TUPLES = [(PIX_U8_AFFINE, WIN_PATCH), (PIX_U8_TABLE, WIN_4X4), (PIX_F32_FLIP, WIN_PATCH), (PIX_F32_FLIP, WIN_4X4), (PIX_F32, WIN_7X7)]

# Every launch of the three kernels in csrc/*.hip, in source order, as the policy names written (or declared) there.
# "unreached": vit.hip's launch_layernorm8 has no caller in any forward, so its tuple is not run (test_rows_host.py asserts it has none).
ROW_LN_CALL_SITES = {
    "vit.hip": [("FromF32", "LnGammaOptBeta", "To16"), ("FromF32", "LnGammaOptBeta", "To16"), ("FromF32", "LnGammaOptBeta", "ToE4m3", "unreached")],
    "ccip.hip": [("FromF32Blocked", "LnGamma<true>", "To16"), ("F32InPlace", "LnGamma<false>", "BackToSource")],
    "convnext.hip": [("FromF32", "LnGammaBeta", "ToF32And16"), ("FromF32", "LnGammaBeta", "ToPatch2x2"), ("From16Bias", "LnGammaBeta", "To16")],
    "swinv2.hip": [("FromF32", "LnGammaBeta", "ToF32And16"), ("FromF32", "LnGammaBeta", "ToF32And16"), ("FromF32", "LnGammaBeta", "AddToStreamHiLo"),
                   ("FromF32", "LnGammaBeta", "AddToStreamHiLo"), ("FromF32", "LnGammaBeta", "ToF32")],
    "rows_dbg.hip": [("FromF32", "LnGammaOptBeta", "To16"), ("FromF32Blocked", "LnGamma<true>", "To16"), ("F32InPlace", "LnGamma<false>", "BackToSource"),
                     ("FromF32", "LnGammaBeta", "ToF32And16"), ("FromF32", "LnGammaBeta", "ToPatch2x2"), ("From16Bias", "LnGammaBeta", "To16"),
                     ("FromF32", "LnGammaBeta", "AddToStreamHiLo"), ("FromF32", "LnGammaBeta", "ToF32")],
}
POOL_LN_CALL_SITES = {"eva.hip": ["PooledHiLo"], "ccip.hip": ["PooledF32"], "convnext.hip": ["PooledHiLo"], "rows_dbg.hip": ["PooledHiLo", "PooledF32"]}
GATHER_CALL_SITES = {
    "eva.hip": [("PixelU8Affine", "WindowPatch"), ("PixelF32Planes<true>", "WindowPatch")],
    "ccip.hip": [("PixelF32Planes<false>", "Window7x7")],
    "vit.hip": [("PixelF32Planes<true>", "WindowPatch")],
    "convnext.hip": [("PixelU8Table", "Window4x4"), ("PixelF32Planes<true>", "Window4x4")],
    "swinv2.hip": [("PixelU8Table", "Window4x4"), ("PixelF32Planes<true>", "Window4x4")],
    "rows_dbg.hip": [("PixelU8Affine", "WindowPatch"), ("PixelU8Table", "Window4x4"), ("PixelF32Planes<true>", "WindowPatch"),
                     ("PixelF32Planes<true>", "Window4x4"), ("PixelF32Planes<false>", "Window7x7")],
}


# The shapes of the exact-answer cases: the smallest at which the indexing can go wrong (a lane tail with D / 4 no multiple of 64, D = 4,
# D = 1024; rows % 4 != 0; more than one workgroup)
LN_SHAPES = [(rows, D) for rows in (1, 5, 7, 64) for D in (4, 96, 256, 260, 768, 1024)]
LN_BLOCKED_SHAPES = [(rows, D) for rows in (16, 48) for D in (16, 128, 256)]
LN_PATCH_SHAPES = [(2, H, 96) for H in (2, 6)]              # (batch, H, D)
POOL_T, POOL_C = (1, 3, 4, 49, 197), (16, 96, 256, 260, 1024)
POOL_BLK_T, POOL_BLK_C = (16, 48), (16, 96, 256, 1024)


# ---- 16-bit operand types ----------------------------------------------------------------------------------------------------------------
def to_op(x, f16):
    """float32 -> 16-bit patterns of the operand type (IEEE half or bf16), round to nearest even"""
    x = np.ascontiguousarray(x, F32)
    if f16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def from_op(bits, f16):
    """16-bit patterns -> float32 (exact)"""
    bits = np.ascontiguousarray(bits, np.uint16)
    if f16:
        return bits.view(np.float16).astype(F32)
    return (bits.astype(np.uint32) << 16).view(F32)


def split_hilo(v, f16, lo_scale=None):
    """row_ln.h split_hilo: hi = 16bit(v), lo = 16bit((v - hi) [* lo_scale]), every step one float32 operation"""
    v = np.ascontiguousarray(v, F32)
    hi = to_op(v, f16)
    r = v - from_op(hi, f16)
    if lo_scale is not None:
        r = r * F32(lo_scale)
    return hi, to_op(r, f16)


def spacing(want, kind):
    """distance between neighbouring values of the output type at |want|: kind 'f32' (0: the bound's spacing term is zero there), 'f16', 'bf16'"""
    want = np.abs(np.asarray(want, np.float64))
    if kind == "f32":
        return np.zeros_like(want)
    e = np.floor(np.log2(np.maximum(want, 2.0 ** -126)))
    if kind == "f16":
        return 2.0 ** (np.maximum(e, -14) - 10)
    return 2.0 ** (e - 7)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------------
def layernorm64(x, g, b, eps):
    x = np.asarray(x, np.float64)
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    y = (x - mean) / np.sqrt(var + np.float64(F32(eps))) * np.asarray(g, np.float64)
    return y if b is None else y + np.asarray(b, np.float64)


def layernorm32(x, g, b, eps, add_zero=True):
    """row_ln.h in numpy float32: two passes, eps inside the square root, (x - mean) * rstd * g + b as three roundings.  b None: + 0 when
    add_zero (LnGammaOptBeta without beta, LnGamma<true>), no addition otherwise (LnGamma<false>).  The sums run in numpy's order."""
    x = np.asarray(x, F32)
    D = F32(x.shape[-1])
    mean = x.sum(-1, keepdims=True, dtype=F32) / D
    d = x - mean
    var = (d * d).sum(-1, keepdims=True, dtype=F32) / D
    rstd = F32(1) / np.sqrt(var + F32(eps))
    y = d * rstd * np.asarray(g, F32)
    if b is not None:
        return y + np.asarray(b, F32)
    return y + F32(0) if add_zero else y


def layernorm32_one_pass(x, g, b, eps):
    """the negative control: variance as E[x^2] - mean^2 in float32"""
    x = np.asarray(x, F32)
    D = F32(x.shape[-1])
    mean = x.sum(-1, keepdims=True, dtype=F32) / D
    var = (x * x).sum(-1, keepdims=True, dtype=F32) / D - mean * mean
    rstd = F32(1) / np.sqrt(np.maximum(var, F32(0)) + F32(eps))
    y = (x - mean) * rstd * np.asarray(g, F32)
    return y if b is None else y + np.asarray(b, F32)


def pool_ln64(x, g, b, eps, count):
    """x [batch][T][C] -> LN(sum over T / count) [batch][C]"""
    return layernorm64(np.asarray(x, np.float64).sum(1) / count, g, b, eps)


def pool_ln32(x, g, b, eps, count):
    x = np.asarray(x, F32)
    return layernorm32(x.sum(1, dtype=F32) / F32(count), g, b, eps)


STAT_KINDS = {"gauss": 1e-6, "offset": 1e-6, "tiny": 1e-5}          # kind -> eps


def stat_rows(kind, rows, D, seed):
    """ordinary numbers for the statistics: Gaussian rows; rows with |mean| / std = 2^10 (a one-pass variance loses them); rows whose
    variance (1e-8) is far below eps (1e-5), where an eps outside the square root would change the answer by orders of magnitude"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((rows, D))
    if kind == "gauss":
        x = 1.7 * z + 0.4
    elif kind == "offset":
        std = rng.uniform(0.5, 2.0, (rows, 1))
        x = std * z + 1024.0 * std * rng.choice([-1.0, 1.0], (rows, 1))
    else:
        x = 1.0 + 1e-4 * z
    return x.astype(F32)


def stat_affine(D, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 1.5, D).astype(F32) * rng.choice([-1, 1], D).astype(F32), (0.3 * rng.standard_normal(D)).astype(F32)


def e32_of(restated32, want64):
    """E32 of the issue: four times the largest error of the float32 restatement against float64 on the same case (the margin covers
    another, equally valid summation order)"""
    return 4.0 * float(np.max(np.abs(np.asarray(restated32, np.float64) - want64)))


def hilo_bounds(want, e32, f16):
    """(bound on |hi - want|, bound on |hi + lo - want|) per element for a hi | lo pair split from a float32 v with |v - want| <= e32:
    hi is v rounded to the operand type; lo = 16bit(v - hi) with |v - hi| <= spacing(v) / 2 <= |v| 2^-(m + 1) (m mantissa bits), rounded
    with relative error 2^-(m + 1), or half a subnormal step of IEEE half (2^-25)"""
    m = 10 if f16 else 7
    want = np.abs(np.asarray(want, np.float64))
    return spacing(want, "f16" if f16 else "bf16") + e32, want * 2.0 ** -(2 * m + 2) + 2.0 ** -25 + e32 * (1 + 2.0 ** -m)


# ---- index maps --------------------------------------------------------------------------------------------------------------------------
def blocked_offsets(M, D):
    """element offset of (m, n) in the blocked stream [m / 16][n / 16][m % 16][n % 16] (row_ln.h x_blk_row + x_blk_vec)"""
    m, n = np.arange(M)[:, None], np.arange(D)[None, :]
    return (((m >> 4) * (D >> 4) + (n >> 4)) << 8) + (m & 15) * 16 + (n & 15)


def to_blocked(x):
    M, D = x.shape
    out = np.empty(M * D, x.dtype)
    out[blocked_offsets(M, D).ravel()] = x.ravel()
    return out


def patch2x2_offsets(batch, H, D):
    """element offset in the 2 x 2 s2 patch matrix of (row (b, iy, ix) of an H x H map, column c) (row_ln.h ToPatch2x2)"""
    row = np.arange(batch * H * H)
    ix, iy, b = row % H, (row // H) % H, row // (H * H)
    Ho = H >> 1
    base = (((b * Ho + (iy >> 1)) * Ho + (ix >> 1)) * 4 + ((iy & 1) * 2 + (ix & 1))) * D
    return base[:, None] + np.arange(D)[None, :]


WINDOWS = {WIN_4X4: dict(ks=4, stride=4, pad=0, half=64, zero_pad=True), WIN_7X7: dict(ks=7, stride=4, pad=2, half=160, zero_pad=False)}


def window(win, P=0, KH=0):
    if win == WIN_PATCH:
        return dict(ks=P, stride=P, pad=0, half=KH, zero_pad=False)
    return WINDOWS[win]


def gather_taps(pix, ks, stride, pad, G):
    """pix [B][S][S][3] (memory channel order) -> [B * G * G][ks * ks * 3]: tap (ky, kx) of channel c at column (ky * ks + kx) * 3 + c of
    token (b, oy, ox), zero outside the image -- the index arithmetic of patch_gather_kernel, one (token, ky, kx, c) at a time"""
    B, S = pix.shape[0], pix.shape[1]
    b, oy, ox, ky, kx, c = np.meshgrid(np.arange(B), np.arange(G), np.arange(G), np.arange(ks), np.arange(ks), np.arange(3), indexing="ij")
    iy, ix = stride * oy - pad + ky, stride * ox - pad + kx
    inside = (iy >= 0) & (iy < S) & (ix >= 0) & (ix < S)
    v = pix[b, np.clip(iy, 0, S - 1), np.clip(ix, 0, S - 1), c]
    return np.where(inside, v, pix.dtype.type(0)).reshape(B * G * G, ks * ks * 3)


def pixels(pixel, images, lut=None):
    """the normalised float32 pixel [B][S][S][3] in memory channel order, as the pixel policy computes it"""
    if pixel == PIX_U8_AFFINE:
        return (images.astype(F32) / F32(255.0) - F32(0.5)) / F32(0.5)
    if pixel == PIX_U8_TABLE:
        return np.stack([lut[c][images[..., c]] for c in range(3)], -1).astype(F32)
    if pixel == PIX_F32_FLIP:                   # planes [B][3][S][S]; plane 2 - c holds memory channel c
        return np.ascontiguousarray(images[:, ::-1].transpose(0, 2, 3, 1))
    if pixel == PIX_F32:
        return np.ascontiguousarray(images.transpose(0, 2, 3, 1))
    raise ValueError(pixel)


def gather_expected(pixel, win, f16, images, lut, P, KH, rows_alloc, fill16=0xFFFF):
    """the whole a0 buffer [rows_alloc][2 half] a launch leaves behind in memory holding fill16: hi | lo of every tap, zeros in the pad
    columns of a ZERO_PAD window, fill16 everywhere else"""
    w = window(win, P, KH)
    S = images.shape[1] if pixel in (PIX_U8_AFFINE, PIX_U8_TABLE) else images.shape[2]
    G = S // w["stride"]
    taps = gather_taps(pixels(pixel, images, lut), w["ks"], w["stride"], w["pad"], G)
    hi, lo = split_hilo(taps, f16)
    n, half = taps.shape[1], w["half"]
    out = np.full((rows_alloc, 2 * half), fill16, np.uint16)
    if w["zero_pad"]:
        out[:taps.shape[0]] = 0
    out[:taps.shape[0], :n] = hi
    out[:taps.shape[0], half:half + n] = lo
    return out


def patchify_raw_expected(images, P, f16, rows_alloc, fill16=0xFFFF):
    """patchify_u8_kernel: A0[m][(ky * P + kx) * 3 + c] = 16bit(raw byte)"""
    B, S = images.shape[0], images.shape[1]
    taps = gather_taps(images, P, P, 0, S // P)
    out = np.full((rows_alloc, 3 * P * P), fill16, np.uint16)
    out[:taps.shape[0]] = to_op(taps.astype(F32), f16)
    return out


# ---- inputs with exact answers -----------------------------------------------------------------------------------------------------------
def balanced_signs(rows, D, seed):
    """[rows][D] of +1 / -1, half of each per row; pairwise distinct rows where D allows (D = 4 has 6 balanced patterns: rows cycle through
    them, so any two rows fewer than 6 apart differ)"""
    out = -np.ones((rows, D), np.int64)
    if D == 4:
        combos = list(itertools.combinations(range(D), D // 2))
        for r in range(rows):
            out[r, list(combos[r % len(combos)])] = 1
        return out
    rng = np.random.default_rng(seed)
    seen = set()
    for r in range(rows):
        while True:
            pos = rng.permutation(D)[:D // 2]
            key = tuple(sorted(pos))
            if key not in seen:
                seen.add(key)
                break
        out[r, pos] = 1
    return out


def gamma_beta(D):
    """g[c] = 1 + c / 1024 and b[c] = c identify every column; +-g + b is exact in float32"""
    c = np.arange(D, dtype=F32)
    return F32(1) + c / F32(1024), c.copy()


def exact_rows(rows, D, seed):
    """(x float32 [rows][D], signs): row r holds m_r + s_r on a balanced half of its columns and m_r - s_r on the rest, m_r an integer in
    [-20, 20], s_r in {1, 2, .., 32}.  Every partial sum of a row is an integer below 2^24 in absolute value, the mean is m_r, the variance
    s_r^2 (a power of four), rstd = 1 / s_r: all exact in float32 under any summation order, and the normalised value is exactly +-1."""
    rng = np.random.default_rng(seed)
    m = rng.integers(-20, 21, rows)
    s = 2 ** rng.integers(0, 6, rows)
    sg = balanced_signs(rows, D, seed + 1)
    return (m[:, None] + s[:, None] * sg).astype(F32), sg


def exact_answer(signs, g, b):
    """fl(fl(+-g) + b) (b None: + 0 or nothing, which differ only in the sign of zero -- there is no zero here)"""
    y = signs.astype(F32) * np.asarray(g, F32)
    return y + np.asarray(b, F32) if b is not None else y


def exact_pool(batch, T, C, seed, scale=1):
    """(x float32 [batch][T][C], signs [batch][C]): x[b][r][c] = scale * ((m_b +- s_b) + z[r][c]) with integers z that cancel over r in + k / - k
    pairs (one zero row when T is odd): every partial sum over rows is an exact integer in any grouping, the column sum is scale * T * (m_b +- s_b)"""
    rng = np.random.default_rng(seed)
    m = rng.integers(-20, 21, batch)
    s = 2 ** rng.integers(0, 6, batch)
    sg = balanced_signs(batch, C, seed + 1)
    base = m[:, None] + s[:, None] * sg
    k = rng.integers(1, 50, (T // 2, C))
    z = np.concatenate([k, -k] + ([np.zeros((1, C), np.int64)] if T % 2 else []), 0)
    z = z[rng.permutation(T)]
    return (scale * (base[:, None, :] + z[None, :, :])).astype(F32), sg
