"""CPU: the host restatements of tests/rows_ref.py against independent definitions (plain reshapes, sliding windows, float64, integer
arithmetic), the properties that make the exact-answer inputs of tests/test_gpu_rows.py exact, the negative control of its float64 bound,
and the table of every row_ln_kernel / pool_ln_kernel / patch_gather_kernel launch in csrc/*.hip."""
import glob
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rows_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "anime-illust-image-searcher_amd", "csrc")
F32 = np.float32


# ---- 16-bit conversions -----------------------------------------------------------------------------------------------------------------
def _nearest_even_16(x, f16):
    """round to nearest even by exact rational comparison in float64: the two neighbouring patterns of the 16-bit type, the nearer one,
    the even pattern on a tie"""
    mant = 10 if f16 else 7
    emin = -14 if f16 else -126
    out = np.zeros(x.shape, np.uint16)
    for i, v in enumerate(x.astype(np.float64)):
        sign = 0x8000 if np.signbit(v) else 0
        a = abs(v)
        e = max(int(np.floor(np.log2(a))) if a > 0 else emin, emin)
        q = a / 2.0 ** (e - mant)                     # in units of the spacing: exact (a power-of-two scaling of a float32)
        lo = np.floor(q)
        n = int(lo) + (1 if (q - lo > 0.5 or (q - lo == 0.5 and int(lo) % 2 == 1)) else 0)
        bits = n if e == emin and n < (1 << mant) else ((e - emin + 1) << mant) + (n - (1 << mant))      # a carry into the exponent falls out
        out[i] = sign | bits
    return out


@pytest.mark.parametrize("f16", [0, 1])
def test_to_op_rounds_to_nearest_even(f16):
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 4, 4000), [0.0, -0.0, 1.0, -1.0, 255.0, 448.0, 1e-7, -3e-6]]).astype(F32)
    # exact ties: halfway between two neighbours, odd and even below
    mant = 10 if f16 else 7
    ties = (np.arange(1 << mant, (1 << mant) + 64) + 0.5) * 2.0 ** -mant
    x = np.concatenate([x, ties.astype(F32), -ties.astype(F32)])
    assert np.array_equal(ties.astype(F32).astype(np.float64), ties)
    got = R.to_op(x, f16)
    assert np.array_equal(got, _nearest_even_16(x, f16))
    assert np.array_equal(R.to_op(R.from_op(got, f16), f16), got)                    # from_op is exact
    assert R.to_op(np.array([-0.0], F32), f16)[0] == 0x8000 and R.to_op(np.array([0.0], F32), f16)[0] == 0


@pytest.mark.parametrize("f16", [0, 1])
def test_split_hilo_is_a_function_of_the_float32_value(f16):
    rng = np.random.default_rng(4)
    v = (rng.standard_normal(5000) * 3).astype(F32)
    hi, lo = R.split_hilo(v, f16)
    h = R.from_op(hi, f16)
    assert np.array_equal(hi, R.to_op(v, f16))
    assert np.array_equal(lo, R.to_op(v - h, f16))                                   # v - hi is exact in float32 (neighbours within a factor 2)
    assert np.array_equal((v - h).astype(np.float64), v.astype(np.float64) - h.astype(np.float64))
    bits = 22 if f16 else 16                                                         # significant bits the pair keeps (row_ln.h)
    err = np.abs(h.astype(np.float64) + R.from_op(lo, f16).astype(np.float64) - v)
    assert np.all(err <= np.abs(v) * 2.0 ** -(bits - 1) + 2.0 ** -24)
    hi2, lo2 = R.split_hilo(v, f16, 64.0)
    assert np.array_equal(hi2, hi) and np.array_equal(lo2, R.to_op((v - h) * F32(64), f16))
    far = np.abs(v - h) > 2.0 ** -14
    assert np.array_equal(R.from_op(lo2, f16)[far], R.from_op(lo, f16)[far] * F32(64))  # scaling by a power of two changes no bit above the subnormals


# ---- index maps against plain reshapes --------------------------------------------------------------------------------------------------
def test_layout_indices_equal_reshapes():
    for M, D in [(16, 16), (48, 128), (32, 256)]:
        x = np.arange(M * D, dtype=np.int64).reshape(M, D)
        want = x.reshape(M // 16, 16, D // 16, 16).transpose(0, 2, 1, 3).ravel()
        assert np.array_equal(R.to_blocked(x), want)
        assert np.array_equal(np.sort(R.blocked_offsets(M, D).ravel()), np.arange(M * D))
    for B, H, D in [(2, 2, 8), (2, 6, 96), (3, 4, 4)]:
        y = np.arange(B * H * H * D, dtype=np.int64).reshape(B, H, H, D)
        Ho = H // 2
        want = y.reshape(B, Ho, 2, Ho, 2, D).transpose(0, 1, 3, 2, 4, 5).reshape(B * Ho * Ho, 4 * D)       # [(b, oy, ox)][(dy, dx, c)]
        got = np.empty(B * H * H * D, np.int64)
        got[R.patch2x2_offsets(B, H, D).ravel()] = y.ravel()
        assert np.array_equal(got.reshape(B * Ho * Ho, 4 * D), want)


@pytest.mark.parametrize("win,P,S", [(R.WIN_7X7, 0, 8), (R.WIN_7X7, 0, 12), (R.WIN_7X7, 0, 20), (R.WIN_4X4, 0, 4), (R.WIN_4X4, 0, 20),
                                     (R.WIN_PATCH, 8, 24), (R.WIN_PATCH, 14, 42), (R.WIN_PATCH, 16, 16)])
def test_window_rows_equal_unfold(win, P, S):
    w = R.window(win, P, 3 * P * P)
    rng = np.random.default_rng(S)
    pix = rng.standard_normal((3, S, S, 3)).astype(F32)
    G = S // w["stride"]
    padded = np.pad(pix, ((0, 0), (w["pad"], w["pad"] + w["ks"]), (w["pad"], w["pad"] + w["ks"]), (0, 0)))
    v = np.lib.stride_tricks.sliding_window_view(padded, (w["ks"], w["ks"]), axis=(1, 2))        # [B][y][x][c][ky][kx]
    v = v[:, ::w["stride"], ::w["stride"]][:, :G, :G].transpose(0, 1, 2, 4, 5, 3)                 # [B][oy][ox][ky][kx][c]
    assert np.array_equal(R.gather_taps(pix, w["ks"], w["stride"], w["pad"], G), v.reshape(3 * G * G, -1))


def test_gather_expected_places_halves_pads_and_fill():
    rng = np.random.default_rng(0)
    u8 = rng.integers(0, 256, (2, 8, 8, 3), dtype=np.uint8)
    lut = rng.standard_normal((3, 256)).astype(F32)
    e = R.gather_expected(R.PIX_U8_TABLE, R.WIN_4X4, 0, u8, lut, 0, 0, 2 * 4 + 1)
    assert e.shape == (9, 128) and np.all(e[8] == 0xFFFF) and np.all(e[:8, 48:64] == 0) and np.all(e[:8, 112:] == 0)
    assert R.from_op(e[3, 3 * (1 * 4 + 2) + 1], 0) == R.from_op(R.to_op(lut[1, u8[0, 4 * 1 + 1, 4 * 1 + 2, 1]], 0), 0)      # token (0, 1, 1), tap (1, 2), channel 1
    planes = rng.standard_normal((2, 3, 8, 8)).astype(F32)
    e = R.gather_expected(R.PIX_F32, R.WIN_7X7, 1, planes, None, 0, 0, 2 * 4)
    assert np.all(e[:, 147:160] == 0xFFFF) and np.all(e[:, 307:] == 0xFFFF)
    assert np.all(e[0, :2 * 21] == 0)                                                              # token (0, 0, 0): rows iy = -2, -1 are border zeros
    assert e[0, (2 * 7 + 2) * 3 + 2] == R.to_op(planes[0, 2, 0, 0], 1)
    e = R.gather_expected(R.PIX_F32_FLIP, R.WIN_PATCH, 0, planes, None, 8, 256, 2)
    assert e[1, 5] == R.to_op(planes[1, 2 - 2, 0, 1], 0) and np.all(e[:, 192:256] == 0xFFFF)         # column 5 = tap (0, 1), memory channel 2 = plane 0
    raw = R.patchify_raw_expected(u8, 4, 1, 9)
    assert raw.shape == (9, 48) and np.all(raw[8] == 0xFFFF) and R.from_op(raw[3, (2 * 4 + 1) * 3], 1) == float(u8[0, 4 + 2, 4 + 1, 0])
    aff = R.pixels(R.PIX_U8_AFFINE, np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, -1))
    assert aff.dtype == F32 and aff.min() == -1.0 and aff.max() == 1.0 and np.max(np.abs(aff.ravel()[::3] - (np.arange(256) / 127.5 - 1))) < 2e-7


# ---- references -------------------------------------------------------------------------------------------------------------------------
def test_float64_references_equal_their_definitions():
    rng = np.random.default_rng(5)
    x, g, b = rng.standard_normal((7, 96)) * 2 + 1, rng.standard_normal(96), rng.standard_normal(96)
    want = (x - x.mean(1, keepdims=True)) / np.sqrt(x.var(1, keepdims=True) + 2.0 ** -10) * g + b
    assert np.allclose(R.layernorm64(x, g, b, 2.0 ** -10), want, rtol=1e-12, atol=1e-12)
    assert np.max(np.abs(R.layernorm32(x.astype(F32), g, b, 2.0 ** -10) - R.layernorm64(x.astype(F32), g.astype(F32), b.astype(F32), 2.0 ** -10))) < 1e-5
    t = rng.standard_normal((3, 49, 96))
    assert np.allclose(R.pool_ln64(t, g, b, 2.0 ** -10, 49), R.layernorm64(t.mean(1), g, b, 2.0 ** -10), rtol=1e-12, atol=1e-12)
    assert np.allclose(R.pool_ln64(4 * t, g, b, 2.0 ** -10, 4 * 49), R.pool_ln64(t, g, b, 2.0 ** -10, 49), rtol=1e-12, atol=1e-12)


# ---- what makes the exact-answer inputs exact -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,D", R.LN_SHAPES + R.LN_BLOCKED_SHAPES + [(2 * H * H, D) for _, H, D in R.LN_PATCH_SHAPES])
def test_exact_rows_are_exact(rows, D):
    x, sg = R.exact_rows(rows, D, 1000 * rows + D)
    x64 = x.astype(np.float64)
    assert np.array_equal(x64, np.round(x64)) and np.all(np.abs(x64).sum(1) < 2 ** 24)        # every partial sum: an integer below 2^24
    assert np.all(np.abs(x64) <= 128)                                                         # exact in bf16 even after an integer bias of a few units
    assert np.all(sg.sum(1) == 0)
    mean, var = x64.mean(1), x64.var(1)
    assert np.array_equal(mean, np.round(mean))
    l4 = np.log2(var) / 2
    assert np.array_equal(l4, np.round(l4)) and np.all(D * var < 2 ** 24)                      # a power of four; the sum of squares D s^2 is exact too
    if D == 4:
        assert all(not np.array_equal(sg[i], sg[j]) for i in range(rows) for j in range(i + 1, min(rows, i + 6)))
        assert len({tuple(r) for r in sg}) == min(rows, 6)
    else:
        assert len({tuple(r) for r in sg}) == rows                                            # the sign pattern identifies the row
    g, b = R.gamma_beta(D)
    assert len(set(zip(g.tolist(), b.tolist()))) == D                                         # (g, b) identifies the column
    want = R.exact_answer(sg, g, b)
    assert np.array_equal(want.astype(np.float64), sg * g.astype(np.float64) + b.astype(np.float64))      # +-g + b needs no rounding at all
    assert np.array_equal(R.layernorm32(x, g, b, 0.0).view(np.uint32), want.view(np.uint32))  # the float32 restatement gives it bit for bit
    assert np.array_equal(R.layernorm32(x[:, ::-1], g[::-1], b[::-1], 0.0)[:, ::-1].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("T,C", [(T, C) for T in R.POOL_T + R.POOL_BLK_T for C in R.POOL_C])
def test_exact_pool_is_exact(T, C):
    for scale in (1, 4):
        x, sg = R.exact_pool(3, T, C, 100 * T + C, scale)
        x64 = x.astype(np.float64)
        assert np.array_equal(x64, np.round(x64)) and np.all(np.abs(x64).sum(1) < 2 ** 24)
        col = x64.sum(1) / (scale * T)
        for rg in range(4):                                       # the four row groups' partial sums are integers whatever their order
            part = x64[:, rg::4].sum(1)
            assert np.array_equal(part, np.round(part))
        assert np.array_equal(col, np.round(col)) and np.all(sg.sum(1) == 0)
        var = col.var(1)
        assert np.array_equal(np.log2(var) / 2, np.round(np.log2(var) / 2)) and np.array_equal(col.mean(1), np.round(col.mean(1)))
        assert np.array_equal((col - col.mean(1, keepdims=True)) / np.sqrt(var)[:, None], sg)
        g, b = R.gamma_beta(C)
        assert np.array_equal(R.pool_ln32(x, g, b, 0.0, scale * T).view(np.uint32), R.exact_answer(sg, g, b).view(np.uint32))


# ---- the float64 bound: a wrong formula must miss it ---------------------------------------------------------------------------------------
def test_one_pass_variance_misses_the_bound():
    """the offset rows (|mean| / std = 2^10) with the bound of test_gpu_rows.py's group C for a float32 sink, E32 alone: the float32 ONE-pass
    restatement misses it by far, so the case can tell a two-pass kernel from a one-pass one"""
    rows, D = 64, 260
    x = R.stat_rows("offset", rows, D, 11)
    ratio = np.abs(x.astype(np.float64).mean(1)) / x.astype(np.float64).std(1)
    assert np.all((ratio > 900) & (ratio < 1200))
    g, b = R.stat_affine(D, 12)
    eps = R.STAT_KINDS["offset"]
    want = R.layernorm64(x, g, b, eps)
    e32 = R.e32_of(R.layernorm32(x, g, b, eps), want)
    one = np.max(np.abs(R.layernorm32_one_pass(x, g, b, eps).astype(np.float64) - want))
    print("offset rows: E32 = %.3g, one-pass error %.3g" % (e32, one))
    assert one > 10 * e32


def test_eps_outside_the_root_misses_the_bound():
    rows, D = 64, 260
    x = R.stat_rows("tiny", rows, D, 13)
    assert np.all(x.astype(np.float64).var(1) < 1e-2 * R.STAT_KINDS["tiny"])
    g, b = R.stat_affine(D, 14)
    eps = R.STAT_KINDS["tiny"]
    want = R.layernorm64(x, g, b, eps)
    e32 = R.e32_of(R.layernorm32(x, g, b, eps), want)
    x64 = x.astype(np.float64)
    wrong = (x64 - x64.mean(1, keepdims=True)) / (x64.std(1, keepdims=True) + eps) * g + b
    assert np.max(np.abs(wrong - want)) > 10 * e32


# ---- every launch in the sources ----------------------------------------------------------------------------------------------------------
def _split_args(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch in "({":
            depth += 1
        elif ch in ")}":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return out + [cur.strip()]


def _policy(text, pos, arg):
    """the policy type of a launch argument: written in place (Type{...}) or declared before the launch (const Type name{...})"""
    m = re.match(r"(\w+(?:<\w+>)?)\{", arg)
    if m:
        return m.group(1)
    decl = re.findall(r"const (\w+(?:<\w+>)?) %s\{" % re.escape(arg), text[:pos])
    assert decl, "no declaration of %r" % arg
    return decl[-1]


def _launches(path, kernel):
    """[(macro or None, [arguments]), ...] of every launch of `kernel` in a source file, in order"""
    text = re.sub(r"//[^\n]*", "", open(path).read())
    pat = r"(HIPTS_LAUNCH(?:_U8)?_F16)\(((?:[^;](?!HIPTS_LAUNCH))*?\b%s\b[^;]*)\);|\b%s<(?:true|false)><<<[^;]*?>>>\(([^;]*)\);" % (kernel, kernel)
    out = []
    for m in re.finditer(pat, text, flags=re.S):
        if m.group(1):
            args = _split_args(m.group(2))
            k = 2 if m.group(1) == "HIPTS_LAUNCH_U8_F16" else 1
            assert args[k] == kernel
            out.append((m.group(1), args[k + 5:], text, m.start()))
        else:
            out.append((None, _split_args(m.group(3)), text, m.start()))
    return out


def _sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def test_row_ln_table_names_every_call_site():
    """every row_ln_kernel launch in csrc/*.hip is in ROW_LN_CALL_SITES with its (source, affine, sink), and every tuple there that a forward
    reaches is one test_gpu_rows.py runs (ROW_LN_VARIANTS); a new launch, or a new tuple, fails here"""
    seen = {}
    for path in _sources():
        found = [tuple(_policy(text, pos, a) for a in args[:3]) for _, args, text, pos in _launches(path, "row_ln_kernel")]
        if found:
            seen[os.path.basename(path)] = found
    assert seen == {f: [s[:3] for s in sites] for f, sites in R.ROW_LN_CALL_SITES.items()}
    run = {v[1:4] for v in R.ROW_LN_VARIANTS}
    reached = set()
    for f, sites in R.ROW_LN_CALL_SITES.items():
        for s in sites:
            t = (R.SRC_NAMES[s[0]], R.AFF_NAMES[s[1]], R.SINK_NAMES[s[2]])
            if len(s) == 4:
                assert s[3] == "unreached" and t not in run
                continue
            assert t in run, "%s launches %s, which test_gpu_rows.py does not run" % (f, s)
            if f != "rows_dbg.hip":
                reached.add(t)
    assert reached == run == set(R.ROW_LN_TUPLES), "the debug entry builds exactly the tuples the forwards launch"
    ids = {v[0]: v for v in R.ROW_LN_VARIANTS}
    assert ids["inplace_blocked"][5] == 1 and ids["inplace_rowmajor"][5] == 0 and ids["opt16_beta"][6] and not ids["opt16_nobeta"][6]


def test_the_e4m3_layernorm_has_no_caller():
    """launch_layernorm8 (ToE4m3) is declared and defined and never called: were a forward to call it again, its tuple would have to join the
    debug entry and the GPU tests, with an e4m3 packing in rows_ref.py"""
    uses = []
    for path in _sources() + sorted(glob.glob(os.path.join(CSRC, "*.h"))):
        text = re.sub(r"//[^\n]*", "", open(path).read())
        uses += [os.path.basename(path) for _ in re.findall(r"launch_layernorm8\(", text)]
    assert sorted(uses) == ["vit.hip", "vit_internal.h"]
    assert not any("ToE4m3" in open(p).read() for p in _sources() if not p.endswith("vit.hip"))


def test_pool_ln_table_names_every_call_site():
    seen = {}
    for path in _sources():
        found = [_policy(text, pos, args[3]) for _, args, text, pos in _launches(path, "pool_ln_kernel")]
        if found:
            seen[os.path.basename(path)] = found
    assert seen == R.POOL_LN_CALL_SITES
    assert {s for sites in R.POOL_LN_CALL_SITES.values() for s in sites} == {n for n, _ in R.POOL_SINKS}


def test_patch_gather_table_names_every_call_site():
    seen = {}
    for path in _sources():
        found = []
        for macro, args, text, pos in _launches(path, "patch_gather_kernel"):
            if macro == "HIPTS_LAUNCH_U8_F16":
                found += [(_policy(text, pos, args[0]), _policy(text, pos, args[2])), (_policy(text, pos, args[1]), _policy(text, pos, args[2]))]
            else:
                found.append((_policy(text, pos, args[0]), _policy(text, pos, args[1])))
        if found:
            seen[os.path.basename(path)] = found
    assert seen == R.GATHER_CALL_SITES
    run = set(R.GATHER_TUPLES)
    reached = {(R.PIX_NAMES[p], R.WIN_NAMES[w]) for f, sites in R.GATHER_CALL_SITES.items() if f != "rows_dbg.hip" for p, w in sites}
    assert reached == run == {(R.PIX_NAMES[p], R.WIN_NAMES[w]) for p, w in R.GATHER_CALL_SITES["rows_dbg.hip"]}
