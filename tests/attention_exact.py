"""Attention inputs whose answer is known in closed form, and the comparisons that go with them (numpy only, no GPU).

tests/test_gpu_attention_exact.py and the SwinV2 window tests run these through the kernels; tests/test_attention_exact_host.py checks the
constructions against the plain float64 softmax and shows that every comparison rejects a wrong answer.  Every value is exactly
representable in bf16 and in IEEE half (but V of the permutation / window cases: normal, rounded to the operand type), so no bound here
has a term for input rounding: each follows from the 16-bit output type alone.

Shapes are [BH, tokens, hd], BH = batch * heads, q in the log2 domain as the kernels take it.

  counting     every real score is the same (`level`: 0 or -16), V an indicator of the key's position inside its tile ("pos") or of its tile
               ("tile") times s = 2^(bh % 4): o[i][d] = s * count_d / tokens for every row.  A padded key scores 0: at level -16 it would
               outweigh a real key by 2^16.
  permutation  key j carries its index as 3 one-hot digits, q[i] the digits of sigma(i): the target scores 72, any other key at most 48,
               o[i] = v[sigma(i)].
  pad noise    finite values for the rows tokens .. tokens_pad - 1 of K and V: masked keys must not reach a real row.
  window       the same two ideas for the SwinV2 window kernel, groups = (window, roll region)."""
import math

import numpy as np


# ---------------------------------------------------------------------------------------------------------------- 16-bit types
def to_op(x, f16):
    """float32 values rounded (to nearest even) to the 16-bit operand type: bf16, or IEEE half with f16."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if f16:
        return x.astype(np.float16).astype(np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def bits(x, f16):
    """The 16-bit patterns of float32 values that are representable in the type."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if f16:
        return x.astype(np.float16).view(np.uint16)
    return (x.view(np.uint32) >> 16).astype(np.uint16)


def from_bits(b, f16):
    b = np.ascontiguousarray(b, dtype=np.uint16)
    if f16:
        return b.view(np.float16).astype(np.float32)
    return (b.astype(np.uint32) << 16).view(np.float32)


def ulp16(x, f16):
    """Spacing of the 16-bit type at |x| (float64): the largest error of one rounding to nearest is half of it, of a truncation all of it."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    _, e = np.frexp(a)                                   # a = m 2^e, m in [0.5, 1)
    emin = -14 if f16 else -126
    e = np.where(a == 0, emin, np.maximum(e - 1, emin))
    return np.ldexp(1.0, e - (10 if f16 else 7))


def split_lo_scale(f16):
    """csrc/vit_internal.h split_lo_scale: what the low half of a hi | lo output pair is multiplied by."""
    return 64.0 if f16 else 1.0


# ---------------------------------------------------------------------------------------------------------------- counting
def tile_keys(hd):
    """G: 64 for the head_dim-64 kernels, 32 for attn.hip at head_dim 32."""
    return 64 if hd == 64 else 32


def counting_v(BH, tokens, hd, form):
    G = tile_keys(hd)
    j = np.arange(tokens)
    col = j % G if form == "pos" else (j // G) % hd
    assert form in ("pos", "tile") and G <= hd
    v = np.zeros((BH, tokens, hd), np.float32)
    for bh in range(BH):
        v[bh, j, col] = 2.0 ** (bh % 4)
    return v


def counting(BH, tokens, hd, level, form):
    """(q, k, v, want): want float64, the same for every query row of an (image, head)."""
    assert level in (0, -16)
    q = np.full((BH, tokens, hd), 0.0 if level == 0 else 0.5, np.float32)
    k = np.full((BH, tokens, hd), -16.0 / (0.5 * hd), np.float32)        # -0.5 at hd 64, -1 at hd 32: with q = 0.5 every score is -16
    v = counting_v(BH, tokens, hd, form)
    want = np.repeat(v.astype(np.float64).sum(axis=1, keepdims=True) / tokens, tokens, axis=1)
    return q, k, v, want


def counting_bad(got, want, f16, exp2_tokens=0):
    """Boolean array, True where `got` misses |got - want| <= ulp16(want) + 2^-20 |want| -- P is one power of two for every key and V is 0
    or a power of two, so the float32 sums are exact and the reciprocal and the product cost 2^-22 at most -- or is not a zero where a
    zero is expected (or is not finite).  exp2_tokens: the float32 term as tokens * 2^-24 |want| instead (an inexact hardware exp2)."""
    got = np.asarray(got, dtype=np.float64)
    rel = exp2_tokens * 2.0 ** -24 if exp2_tokens else 2.0 ** -20
    ok = np.abs(got - want) <= ulp16(want, f16) + rel * np.abs(want)
    return ~np.where(want == 0, got == 0, ok)


# ---------------------------------------------------------------------------------------------------------------- permutation
def sigma(tokens):
    a = tokens // 2 + 1
    while math.gcd(a, tokens) != 1:
        a += 1
    return (a * np.arange(tokens) + tokens // 3) % tokens


def digit_codes(n, width, base, value):
    """[n, width] float32: row j holds `value` at the columns d * base + digit_d(j), d = 0 .. 2."""
    assert n <= base ** 3 and 3 * base <= width
    j = np.arange(n)
    c = np.zeros((n, width), np.float32)
    for d in range(3):
        c[j, d * base + (j // base ** d) % base] = value
    return c


def permutation(BH, tokens, hd, f16, seed=0):
    """(q, k, v, want, sigma): scores 24 x (matching digits); want = v[sigma] (float64)."""
    base = 16 if hd == 64 else 10
    sg = sigma(tokens)
    k1 = digit_codes(tokens, hd, base, 4.0)
    q1 = digit_codes(tokens, hd, base, 6.0)[sg]
    v = to_op(np.random.default_rng(1000 * tokens + hd + seed).standard_normal((BH, tokens, hd)), f16)
    q = np.repeat(q1[None], BH, axis=0)
    k = np.repeat(k1[None], BH, axis=0)
    return q, k, v, v[:, sg].astype(np.float64), sg


LEAK = 2.0 ** -16      # x max |v|: at most 45 keys share two digits with the target (3 x 15), each at 2^-24 of its weight; 45 * 2^-24 < 2^-18


def permutation_bad(got, want, f16, vmax):
    got = np.asarray(got, dtype=np.float64)
    return ~(np.abs(got - want) <= ulp16(want, f16) + LEAK * vmax)


def half_overflow_rows(q, k):
    """Rows of one (image, head) that cannot stay on the half-operand fast path: P = 2^(S - m_ref) with m_ref = the row's maximum over
    its first keys + 10 bits; the target's P reaches 2^16 (inf in half) when its score lies 26 above that maximum.  The first 64 keys
    are taken here (the kernels take 32 or 64 of them): a superset, so a larger maximum and fewer rows."""
    s = q.astype(np.float64) @ k.astype(np.float64).T
    return np.nonzero(s.max(axis=1) - s[:, :64].max(axis=1) >= 26.0)[0]


# ---------------------------------------------------------------------------------------------------------------- pad noise
def pad_noise(BH, rows, hd, f16, seed):
    """Finite values, |x| <= 2, for the padded rows of K or V."""
    return to_op(np.random.default_rng(seed).uniform(-2.0, 2.0, (BH, rows, hd)), f16)


# ---------------------------------------------------------------------------------------------------------------- hi | lo output
SPLIT_REL = {0: 2.0 ** -14, 1: 2.0 ** -18}     # bf16: the low half (<= 2^-9 |x|) rounded at 2^-9 -> 2^-18 |x|; half: (<= 2^-11) at 2^-11 -> 2^-22


def split_bad(hi, lo, want, f16, lo_scale, leak=0.0):
    """True where |hi + lo / lo_scale - want| <= SPLIT_REL |want| (+ leak, the permutation's absolute term) fails."""
    got = np.asarray(hi, dtype=np.float64) + np.asarray(lo, dtype=np.float64) / lo_scale
    return ~(np.abs(got - want) <= SPLIT_REL[f16] * np.abs(want) + leak)


# ---------------------------------------------------------------------------------------------------------------- SwinV2 windows
def window_groups(side, window, shift, regions):
    """Per raster token (numpy int arrays [side^2]): its window after the roll by -shift, its index inside the window, and its
    (window, region) group id.  regions: the roll region of every raster token (swinv2_ref.raster_regions)."""
    y, x = np.divmod(np.arange(side * side), side)
    yr, xr = (y - shift) % side, (x - shift) % side                       # where the roll by -shift puts the token
    win = (yr // window) * (side // window) + xr // window
    local = (yr % window) * window + xr % window
    return win, local, win * 9 + np.asarray(regions).astype(np.int64)


def window_counting(batch, heads, side, window, shift, regions, f16, seed=0):
    """q = k = one vector per head for every token (every cosine 1), cpb 0, logit scale ln 10: a token's output is the mean of v over its
    group.  Returns (q, k, v, logit_scale, cpb, want) in hiptsdbg_swinv2_window_attention's layouts, want float64."""
    rng = np.random.default_rng(7000 + 100 * window + shift + seed)
    N, C = side * side, 32 * heads
    u = to_op(rng.integers(1, 4, C) * rng.choice([-0.5, 0.5], C), f16)
    q = np.broadcast_to(u, (batch, N, C)).astype(np.float32)
    v = to_op(rng.standard_normal((batch, N, C)), f16)
    _, _, grp = window_groups(side, window, shift, regions)
    want = np.empty((batch, N, C), np.float64)
    for g in np.unique(grp):
        m = grp == g
        want[:, m] = v[:, m].astype(np.float64).mean(axis=1, keepdims=True)
    ls = np.full(heads, math.log(10.0), np.float32)
    return q, q.copy(), v, ls, np.zeros((heads, (2 * window - 1) ** 2), np.float32), want


def window_placement(batch, heads, side, window, shift, regions, f16, seed=0):
    """k[j] = the window-local index of j as two one-hot base-16 digits, q[i] = the code of the next token of i's group in cyclic order
    (by local index); logit scale ln 100: scores 100, 50 or 0, want = v[next(i)]."""
    rng = np.random.default_rng(9000 + 100 * window + shift + seed)
    N, C = side * side, 32 * heads
    _, local, grp = window_groups(side, window, shift, regions)
    nxt = np.empty(N, np.int64)
    for g in np.unique(grp):
        idx = np.nonzero(grp == g)[0]
        idx = idx[np.argsort(local[idx])]
        nxt[idx] = np.roll(idx, -1)
    code = np.zeros((N, 32), np.float32)
    code[np.arange(N), local % 16] = 1.0
    code[np.arange(N), 16 + local // 16] = 1.0
    k = np.broadcast_to(np.tile(code, (1, heads)), (batch, N, C)).astype(np.float32)
    q = np.ascontiguousarray(k[:, nxt])
    v = to_op(rng.standard_normal((batch, N, C)), f16)
    ls = np.full(heads, math.log(100.0), np.float32)
    return q, k, v, ls, np.zeros((heads, (2 * window - 1) ** 2), np.float32), v[:, nxt].astype(np.float64)


def window_counting_bad(got, want, f16, vmax):
    """ulp16(want) + 2^-16 max |v|: every numerator is the same, at most 256 float32 terms are summed (256 * 2^-24 = 2^-16)."""
    return ~(np.abs(np.asarray(got, dtype=np.float64) - want) <= ulp16(want, f16) + 2.0 ** -16 * vmax)


def window_placement_bad(got, want, f16):
    return ~(np.abs(np.asarray(got, dtype=np.float64) - want) <= ulp16(want, f16))
