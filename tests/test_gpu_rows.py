"""GPU: the row kernels of csrc/row_ln.h and csrc/patch_rows.h and the two LDS-tiled uint8 stems, one launch per case through the debug
entries of csrc/rows_dbg.hip (hiptsdbg_row_ln, hiptsdbg_pool_ln, hiptsdbg_patch_gather) and the two entries beside the stems
(hiptsdbg_ccip_stem_u8, hiptsdbg_vit_patchify_u8_p16), against tests/rows_ref.py.  Every output buffer is given with guard bytes behind the
launch's extent and comes back whole: the entries fill it with 0xff (0xffff / 0xffffffff are NaNs no case produces), so a guard byte that
changed was written by the kernel.
  A  row_ln_kernel, exact answers: rows of m +- s, eps = 0 -- mean, variance, rstd and the normalised +-1 are exact in float32 under any
     summation order, the output is fl(fl(+-g[c]) + b[c]); every source, affine and sink the forwards launch, bit for bit.
  B  sign of zero per affine, and constant rows.
  C  statistics on ordinary numbers against float64: |got - want| <= spacing of the output type at |want| + E32 per element, E32 = four
     times the largest error of the float32 numpy restatement of the same formula on the same case (printed with the error seen).
  D  pool_ln_kernel, exact answers; Gaussian rows, and rows that make `count` visible, with C's bound.
  E  patch_gather_kernel / patchify_u8_kernel: bit equality with the numpy restatement, pad columns and rows past the launch included.
  F  the two uint8 stems: byte for byte the generic gather of the same images.
  G  refusals: -1, nothing launched.
Both operand types wherever the tuple has one.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rows_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
FILL = 0xFF
GUARD = 256                 # guard bytes behind every buffer (and the whole size of a buffer the launch does not use)


class CaseT(ctypes.Structure):
    _fields_ = ([(f, ctypes.c_int32) for f in ("src", "affine", "sink", "f16", "blk", "H", "D", "fill")] +
                [("rows", ctypes.c_int64), ("eps", ctypes.c_float), ("in_", ctypes.c_void_p), ("in_bytes", ctypes.c_uint64), ("bias", ctypes.c_void_p),
                 ("g", ctypes.c_void_p), ("b", ctypes.c_void_p), ("x_init", ctypes.c_void_p), ("x_init_bytes", ctypes.c_uint64)])


class OutT(ctypes.Structure):
    _fields_ = [("f32", ctypes.c_void_p), ("o16", ctypes.c_void_p), ("f32_bytes", ctypes.c_uint64), ("o16_bytes", ctypes.c_uint64)]


@functools.lru_cache(maxsize=None)
def _lib():
    from hiptagsearch import _lib as L
    lib = L.load()
    I, U64, P, FL = ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_float
    lib.hiptsdbg_row_ln.argtypes = [ctypes.POINTER(CaseT), ctypes.POINTER(OutT)]
    lib.hiptsdbg_pool_ln.argtypes = [P, U64, P, P, I, I, I, I, I, FL, I, I, I, P, U64]
    lib.hiptsdbg_patch_gather.argtypes = [I, I, I, P, U64, P, I, I, I, I, I, P, U64]
    lib.hiptsdbg_ccip_stem_u8.argtypes = [P, P, I, I, I, I, P, U64]
    lib.hiptsdbg_vit_patchify_u8_p16.argtypes = [P, I, I, I, I, P, U64]

    class Entries:
        pass

    def stop_on_hip_error(f):
        def call(*args):
            st = f(*args)
            if st == -3:        # HIPTS_ERR_HIP: a runtime call or a kernel failed -- nothing more is started on this device
                pytest.exit("%s: HIP error (%s)" % (f.__name__, L.last_error()), 3)
            return st
        return call

    e = Entries()
    for name in ("hiptsdbg_row_ln", "hiptsdbg_pool_ln", "hiptsdbg_patch_gather", "hiptsdbg_ccip_stem_u8", "hiptsdbg_vit_patchify_u8_p16"):
        setattr(e, name, stop_on_hip_error(getattr(lib, name)))
    return e


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _f32c(a):
    return None if a is None else np.ascontiguousarray(a, F32)


# ---- hiptsdbg_row_ln: one variant of rows_ref.ROW_LN_VARIANTS on logical rows x [rows][D] ---------------------------------------------------
def variant(name):
    return next(v for v in R.ROW_LN_VARIANTS if v[0] == name)


def launch_row_ln(v, f16, x, g, b, eps, H=0, x0=None, bias=None, short=None, raw=None):
    """status, f32 buffer as uint32, 16-bit buffer as uint16 -- both whole, guard bytes included.  x: the rows the kernel is to normalise
    (for SRC_16_BIAS: 16-bit rows x - bias, exact by construction of the caller); short: 'f32' / 'o16' gives that buffer one byte too few"""
    _, src, aff, sink, _, blk, _ = v
    rows, D = x.shape
    n = rows * D
    c = CaseT(src=src, affine=aff, sink=sink, f16=f16, blk=blk, H=H, D=D, fill=FILL, rows=rows, eps=eps)
    g, b = _f32c(g), _f32c(b)
    keep = [g, b]
    c.g, c.b = _ptr(g), _ptr(b)
    in_place = src == R.SRC_F32_INPLACE or sink == R.SINK_F32_AND_16
    need32 = n * 4 if (in_place or sink in (R.SINK_ADD_HILO, R.SINK_F32)) else 0
    need16 = 0 if sink in (R.SINK_BACK, R.SINK_F32) else (4 * n if sink == R.SINK_ADD_HILO else 2 * n)
    if src == R.SRC_16_BIAS:
        bias = _f32c(bias)
        data = R.to_op(x - bias[None, :], f16)
        assert np.array_equal(R.from_op(data, f16) + bias[None, :], x)
        c.bias = _ptr(bias)
        keep.append(bias)
    elif src == R.SRC_F32_BLOCKED or (src == R.SRC_F32_INPLACE and blk):
        data = R.to_blocked(_f32c(x))
    else:
        data = _f32c(x).ravel()
    keep.append(data)
    if in_place:
        c.x_init, c.x_init_bytes = _ptr(data), data.nbytes
    else:
        c.in_, c.in_bytes = _ptr(data), data.nbytes
        if x0 is not None:
            x0 = _f32c(x0)
            keep.append(x0)
            c.x_init, c.x_init_bytes = _ptr(x0), x0.nbytes
    out32 = np.full((need32 + GUARD) // 4, 0x5A5A5A5A, np.uint32)            # host buffers start with a pattern of their own: a refused call leaves it
    out16 = np.full((need16 + GUARD) // 2, 0x5A5A, np.uint16)
    o = OutT(f32=_ptr(out32), o16=_ptr(out16), f32_bytes=out32.nbytes - (short == "f32") * (GUARD + 1), o16_bytes=out16.nbytes - (short == "o16") * (GUARD + 1))
    if raw:
        for k, val in raw.items():
            setattr(c, k, val)
    st = _lib().hiptsdbg_row_ln(ctypes.byref(c), ctypes.byref(o))
    return st, out32, out16


def expect_row_ln(v, f16, o, H=0, x0=None):
    """the whole buffers (uint32, uint16) a launch leaves behind when the affine's float32 result is o [rows][D]"""
    _, src, aff, sink, _, blk, _ = v
    rows, D = o.shape
    n = rows * D
    o = _f32c(o)
    e32, e16 = np.zeros(0, np.uint32), np.zeros(0, np.uint16)
    if sink in (R.SINK_16, R.SINK_F32_AND_16):
        e16 = R.to_op(o, f16).ravel()
    if sink == R.SINK_PATCH2X2:
        e16 = np.empty(n, np.uint16)
        e16[R.patch2x2_offsets(rows // (H * H), H, D).ravel()] = R.to_op(o, f16).ravel()
    if sink in (R.SINK_F32, R.SINK_F32_AND_16):
        e32 = o.view(np.uint32).ravel()
    if sink == R.SINK_BACK:
        e32 = (R.to_blocked(o) if blk else o.ravel()).view(np.uint32)
    if sink == R.SINK_ADD_HILO:
        new = _f32c(x0) + o                                             # one float32 addition
        hi, lo = R.split_hilo(new, f16)
        e32, e16 = new.view(np.uint32).ravel(), np.concatenate([hi, lo], 1).ravel()
    return (np.concatenate([e32, np.full(GUARD // 4, 0xFFFFFFFF, np.uint32)]), np.concatenate([e16, np.full(GUARD // 2, 0xFFFF, np.uint16)]))


def _diff(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d words differ, first at %d: got %#x, want %#x" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


def check_bits(v, f16, x, g, b, eps, o, H=0, x0=None, bias=None):
    st, got32, got16 = launch_row_ln(v, f16, x, g, b, eps, H, x0, bias)
    assert st == 0
    want32, want16 = expect_row_ln(v, f16, o, H, x0)
    _diff(got32, want32, "float32 buffer")
    _diff(got16, want16, "16-bit buffer")
    return got32, got16


def _ops(v):
    return (0, 1) if v[4] else (0,)


def _shapes(v):
    if v[0] == "patch2x2":
        return [(b * H * H, D, H) for b, H, D in R.LN_PATCH_SHAPES]
    if v[1] == R.SRC_F32_BLOCKED or v[5]:
        return [(r, D, 0) for r, D in R.LN_BLOCKED_SHAPES]
    return [(r, D, 0) for r, D in R.LN_SHAPES]


def _extras(v, rows, D, seed):
    """(x0: the stream AddToStreamHiLo adds to, integers; bias: From16Bias's integers k_c)"""
    rng = np.random.default_rng(seed)
    x0 = rng.integers(-64, 65, (rows, D)).astype(F32) if v[3] == R.SINK_ADD_HILO else None
    bias = rng.integers(-8, 9, D).astype(F32) if v[1] == R.SRC_16_BIAS else None
    return x0, bias


A_CASES = [pytest.param(v, f16, rows, D, H, id="%s-%s-%dx%d" % (v[0], "f16" if f16 else "bf16" if v[4] else "f32", rows, D))
           for v in R.ROW_LN_VARIANTS for f16 in _ops(v) for rows, D, H in _shapes(v)]


@pytest.mark.parametrize("v,f16,rows,D,H", A_CASES)
def test_a_row_ln_exact_placement(v, f16, rows, D, H):
    x, sg = R.exact_rows(rows, D, 1000 * rows + D)
    g, b = R.gamma_beta(D)
    b = b if v[6] else None
    x0, bias = _extras(v, rows, D, rows + D)
    check_bits(v, f16, x, g, b, 0.0, R.exact_answer(sg, g, b), H, x0, bias)


# ---- B: sign of zero ------------------------------------------------------------------------------------------------------------------------
def _zero_rows(rows, D, seed):
    """rows of m + {+2 s on an eighth of the columns, -2 s on an eighth, 0 on the rest}: mean m, variance s^2, rstd 1 / s, all exact; three
    quarters of every row sit exactly on the mean"""
    rng = np.random.default_rng(seed)
    m, s = rng.integers(-20, 21, rows), 2 ** rng.integers(0, 5, rows)
    pat = np.zeros((rows, D), np.int64)
    for r in range(rows):
        p = rng.permutation(D)
        pat[r, p[:D // 8]], pat[r, p[D // 8:D // 4]] = 2, -2
    x = (m[:, None] + s[:, None] * pat).astype(F32)
    x64 = x.astype(np.float64)
    assert np.array_equal(x64.mean(1), m) and np.array_equal(x64.var(1), s.astype(np.float64) ** 2)
    return x, pat


B_CASES = [pytest.param(v, f16, bz, id="%s-%s-beta%s" % (v[0], "f16" if f16 else "bf16" if v[4] else "f32", bz))
           for v in R.ROW_LN_VARIANTS for f16 in _ops(v) for bz in (("-0", "+0") if v[6] else ("none",))]


@pytest.mark.parametrize("v,f16,bz", B_CASES)
def test_b_sign_of_zero(v, f16, bz):
    """columns equal to the row mean under a negative g: the product is -0.  LnGamma<false> keeps it; LnGamma<true> and LnGammaOptBeta without
    beta add + 0.f and store +0; with a beta the sum is -0 only when beta is -0 too.  Through every sink, in float32 and in the 16-bit types;
    AddToStreamHiLo: -0 + -0 = -0 in the stream and in hi, lo = 16bit(-0 - -0) = +0."""
    rows, D, H = 16, 96, 2
    x, pat = _zero_rows(rows, D, 5)
    g = -R.gamma_beta(D)[0]
    b = None if bz == "none" else np.full(D, -0.0 if bz == "-0" else 0.0, F32)
    plain = v[2] == R.AFF_GAMMA_PLAIN
    o = R.layernorm32(x, g, b, 0.0, add_zero=not plain)
    zero = pat == 0
    negative = (plain or bz == "-0")
    assert np.all(o[zero] == 0) and np.all(np.signbit(o[zero]) == negative) and np.array_equal(o[~zero], (pat * g.astype(np.float64))[~zero].astype(F32))
    x0, bias = _extras(v, rows, D, 6)
    if x0 is not None:
        x0[:] = -0.0 if negative else 0.0
    got32, got16 = check_bits(v, f16, x, g, b, 0.0, o, H, x0, bias)
    # the claim itself, spelled out on the buffers (row-major sinks; the blocked and 2 x 2 layouts are covered by the comparison above)
    if v[3] in (R.SINK_F32, R.SINK_F32_AND_16, R.SINK_ADD_HILO) or (v[3] == R.SINK_BACK and not v[5]):
        assert np.all(got32[:rows * D].reshape(rows, D)[zero] == (0x80000000 if negative else 0))
    if v[3] in (R.SINK_16, R.SINK_F32_AND_16):
        assert np.all(got16[:rows * D].reshape(rows, D)[zero] == (0x8000 if negative else 0))
    if v[3] == R.SINK_ADD_HILO:
        hl = got16[:2 * rows * D].reshape(rows, 2 * D)
        assert np.all(hl[:, :D][zero] == (0x8000 if negative else 0)) and np.all(hl[:, D:][zero] == 0)


@pytest.mark.parametrize("v,f16", [pytest.param(v, f16, id="%s-%s" % (v[0], "f16" if f16 else "bf16" if v[4] else "f32")) for v in R.ROW_LN_VARIANTS for f16 in _ops(v)])
def test_b_constant_rows_store_beta(v, f16):
    """a constant row with eps > 0: x - mean = 0, so the output is exactly b (without beta: a zero, signed by the affine's rule)"""
    rows, D, H = 16, 96, 2
    rng = np.random.default_rng(8)
    x = np.repeat(rng.integers(-50, 51, (rows, 1)), D, 1).astype(F32)
    g, b = R.stat_affine(D, 9)
    b = b if v[6] else None
    o = R.layernorm32(x, g, b, 1e-5, add_zero=v[2] != R.AFF_GAMMA_PLAIN)
    if b is not None:
        assert np.array_equal(o.view(np.uint32), np.broadcast_to(b, (rows, D)).view(np.uint32))
    else:
        assert np.all(o == 0) and np.array_equal(np.signbit(o), np.broadcast_to((g < 0) & (v[2] == R.AFF_GAMMA_PLAIN), (rows, D)))
    x0, bias = _extras(v, rows, D, 10)
    check_bits(v, f16, x, g, b, 1e-5, o, H, x0, bias)


# ---- C: statistics against float64 ---------------------------------------------------------------------------------------------------------
C_CASES = [pytest.param(v, f16, kind, id="%s-%s-%s" % (v[0], "f16" if f16 else "bf16" if v[4] else "f32", kind))
           for v in R.ROW_LN_VARIANTS for f16 in _ops(v) for kind in R.STAT_KINDS]


@pytest.mark.parametrize("v,f16,kind", C_CASES)
def test_c_statistics_against_float64(v, f16, kind):
    blocked = v[1] == R.SRC_F32_BLOCKED or v[5]
    rows, D, H = 64, (256 if blocked else 260), 4
    eps = R.STAT_KINDS[kind]
    x = R.stat_rows(kind, rows, D, 21)
    g, b = R.stat_affine(D, 22)
    b = b if v[6] else None
    bias, x0 = None, None
    if v[1] == R.SRC_16_BIAS:                       # the rows the kernel normalises are fl32(16-bit value + bias)
        bias = (0.3 * np.random.default_rng(23).standard_normal(D)).astype(F32)
        x = R.from_op(R.to_op(x, f16), f16) + bias[None, :]
    if v[3] == R.SINK_ADD_HILO:
        x0 = np.random.default_rng(24).standard_normal((rows, D)).astype(F32)
    want = R.layernorm64(x, g, b, eps)
    rest = R.layernorm32(x, g, b, eps, add_zero=v[2] != R.AFF_GAMMA_PLAIN)
    if x0 is not None:
        want, rest = x0.astype(np.float64) + want, x0 + rest
    e32 = R.e32_of(rest, want)
    st, got32, got16 = launch_row_ln(v, f16, x, g, b, eps, H, x0, bias)
    assert st == 0
    n = rows * D
    assert np.all(got32[got32.size - GUARD // 4:] == 0xFFFFFFFF) and np.all(got16[got16.size - GUARD // 2:] == 0xFFFF)
    sink = v[3]
    err16 = err32 = 0.0
    if sink in (R.SINK_F32, R.SINK_F32_AND_16, R.SINK_ADD_HILO, R.SINK_BACK):
        y = got32[:n].view(F32)
        if sink == R.SINK_BACK and v[5]:
            y = y[R.blocked_offsets(rows, D).ravel()]
        y = y.reshape(rows, D)
        err32 = float(np.max(np.abs(y.astype(np.float64) - want)))
        print("C %s %s f16=%d: E32 = %.3g, float32 output error %.3g" % (v[0], kind, f16, e32, err32))
        assert np.all(np.abs(y.astype(np.float64) - want) <= e32)
        if sink == R.SINK_F32_AND_16:               # the 16-bit copy is rounded from the value stored
            _diff(got16[:n], R.to_op(y, f16).ravel(), "16-bit copy of the stored float32")
        if sink == R.SINK_ADD_HILO:                 # hi and lo are exact functions of the NEW x
            hi, lo = R.split_hilo(y, f16)
            _diff(got16[:2 * n], np.concatenate([hi, lo], 1).ravel(), "hi | lo of the stored float32")
    if sink in (R.SINK_16, R.SINK_PATCH2X2):
        h = got16[:n]
        if sink == R.SINK_PATCH2X2:
            h = h[R.patch2x2_offsets(rows // (H * H), H, D).ravel()]
        y = R.from_op(h, f16).astype(np.float64).reshape(rows, D)
        bound = R.spacing(want, "f16" if f16 else "bf16") + e32
        err16 = float(np.max(np.abs(y - want)))
        print("C %s %s f16=%d: E32 = %.3g, 16-bit output error %.3g, largest error / bound %.3g" % (v[0], kind, f16, e32, err16, np.max(np.abs(y - want) / bound)))
        assert np.all(np.abs(y - want) <= bound)


# ---- D: pool_ln_kernel ------------------------------------------------------------------------------------------------------------------------
def launch_pool(x, g, b, count, blk, eps, hilo, f16, short=False, T=None, C=None):
    batch, T0, C0 = x.shape
    T, C = T or T0, C or C0
    data = np.concatenate([R.to_blocked(x[i]) for i in range(batch)]) if blk else _f32c(x).ravel()
    g, b = _f32c(g), _f32c(b)
    out = np.full((batch * C0 * 4 + GUARD) // 2, 0x5A5A, np.uint16)
    st = _lib().hiptsdbg_pool_ln(_ptr(data), data.nbytes, _ptr(g), _ptr(b), batch, T, C, count, blk, eps, hilo, f16, FILL, _ptr(out),
                                 out.nbytes - (GUARD + 1 if short else 0))
    return st, out


def expect_pool(o, hilo, f16):
    o = _f32c(o)
    body = np.concatenate(R.split_hilo(o, f16), 1).ravel() if hilo else o.view(np.uint16).ravel()
    return np.concatenate([body, np.full(GUARD // 2, 0xFFFF, np.uint16)])


POOL_SINKS = [(0, 0, "f32"), (1, 0, "hilo-bf16"), (1, 1, "hilo-f16")]
D_CASES = ([pytest.param(T, C, 0, mult, hilo, f16, id="T%d-C%d-rowmajor-count%dT-%s" % (T, C, mult, name))
            for T in R.POOL_T for C in R.POOL_C for mult in (1, 4) for hilo, f16, name in POOL_SINKS] +
           [pytest.param(T, C, 1, mult, hilo, f16, id="T%d-C%d-blocked-count%dT-%s" % (T, C, mult, name))
            for T in R.POOL_BLK_T for C in R.POOL_BLK_C for mult in (1, 4) for hilo, f16, name in POOL_SINKS])


@pytest.mark.parametrize("T,C,blk,mult,hilo,f16", D_CASES)
def test_d_pool_ln_exact(T, C, blk, mult, hilo, f16):
    """count == T, and count == 4 T on inputs scaled by four: the quotient column sum / count is the same exact m +- s"""
    x, sg = R.exact_pool(3, T, C, 100 * T + C, mult)
    g, b = R.gamma_beta(C)
    st, got = launch_pool(x, g, b, mult * T, blk, 0.0, hilo, f16)
    assert st == 0
    _diff(got, expect_pool(R.exact_answer(sg, g, b), hilo, f16), "pooled output")


@pytest.mark.parametrize("kind,mult", [("gauss", 1), ("tiny", 4)])
@pytest.mark.parametrize("hilo,f16,name", POOL_SINKS)
def test_d_pool_ln_gaussian_against_float64(hilo, f16, name, kind, mult):
    """The exact cases cannot see `count`: with eps = 0 a LayerNorm does not change when its input is scaled.  Here it can: Gaussian rows with
    count == T, and rows whose pooled variance is far below eps with count == 4 T, where the output is proportional to 1 / count."""
    T, C, eps = 49, 260, R.STAT_KINDS[kind]
    z = np.random.default_rng(31).standard_normal((3, T, C))
    x = (1.7 * z + 0.4 if kind == "gauss" else 1.0 + 1e-3 * z).astype(F32)
    g, b = R.stat_affine(C, 32)
    want = R.pool_ln64(x, g, b, eps, mult * T)
    if kind == "tiny":
        assert np.all((x.astype(np.float64).sum(1) / (mult * T)).var(1) < 1e-2 * eps)
        assert np.max(np.abs(R.pool_ln64(x, g, b, eps, T) - want)) > 0.05                  # another count is another answer
    e32 = R.e32_of(R.pool_ln32(x, g, b, eps, mult * T), want)
    st, got = launch_pool(x, g, b, mult * T, 0, eps, hilo, f16)
    assert st == 0 and np.all(got[got.size - GUARD // 2:] == 0xFFFF)
    if not hilo:
        y = got[:3 * C * 2].view(F32).reshape(3, C).astype(np.float64)
        print("D %s count=%dT %s: E32 = %.3g, error %.3g" % (kind, mult, name, e32, np.max(np.abs(y - want))))
        assert np.all(np.abs(y - want) <= e32)
        return
    hl = got[:3 * 2 * C].reshape(3, 2 * C)
    hi, lo = R.from_op(hl[:, :C], f16).astype(np.float64), R.from_op(hl[:, C:], f16).astype(np.float64)
    print("D %s count=%dT %s: E32 = %.3g, hi error %.3g, hi + lo error %.3g" % (kind, mult, name, e32, np.max(np.abs(hi - want)), np.max(np.abs(hi + lo - want))))
    bound_hi, bound_sum = R.hilo_bounds(want, e32, f16)
    assert np.all(np.abs(hi - want) <= bound_hi)
    assert np.all(np.abs(hi + lo - want) <= bound_sum)


# ---- E: patch gather -------------------------------------------------------------------------------------------------------------------------
def u8_images(batch, S, seed):
    """every byte value, as far as the images have room for them"""
    n = batch * S * S * 3
    rng = np.random.default_rng(seed)
    v = np.concatenate([rng.permutation(256) for _ in range(n // 256 + 1)])[:n].astype(np.uint8)
    assert n < 256 or np.unique(v).size == 256
    return v.reshape(batch, S, S, 3)


def f32_planes(batch, S, seed):
    """distinct values per (b, c, y, x), with low-order bits for the lo half"""
    n = batch * 3 * S * S
    v = ((np.random.default_rng(seed).permutation(n) + 0.37) / n * 4.0 - 2.0).astype(F32)
    assert np.unique(v).size == n
    return v.reshape(batch, 3, S, S)


@functools.lru_cache(maxsize=None)
def lut():
    return (np.random.default_rng(41).standard_normal((3, 256)) * 1.3).astype(F32)


def launch_gather(pixel, win, f16, images, P, KH, row_elems, rows, extra_rows=2, fill=FILL, short=False):
    images = np.ascontiguousarray(images)
    S = images.shape[1] if images.dtype == np.uint8 else images.shape[2]
    out = np.full(((rows + extra_rows) * row_elems,), 0x5A5A, np.uint16)
    table = lut()
    st = _lib().hiptsdbg_patch_gather(pixel, win, f16, _ptr(images), images.nbytes, _ptr(table) if pixel == R.PIX_U8_TABLE else None, images.shape[0], S, P, KH,
                                      fill, _ptr(out), out.nbytes - (extra_rows * row_elems * 2 + 1 if short else 0))
    return st, out.reshape(rows + extra_rows, row_elems)


def _kh(P):
    return (3 * P * P + 64) // 64 * 64              # always leaves pad columns behind the taps


# Window7x7: S = 8, 12, 20 clip the border at both ends of a row of windows; S = 4 is one window that is clipped on both of its sides
E_CASES = ([(R.PIX_F32, R.WIN_7X7, 0, S) for S in (4, 8, 12, 20)] +
           [(p, R.WIN_4X4, 0, S) for p in (R.PIX_U8_TABLE, R.PIX_F32_FLIP) for S in (4, 8, 20)] +
           [(p, R.WIN_PATCH, P, 3 * P) for p in (R.PIX_U8_AFFINE, R.PIX_F32_FLIP) for P in (8, 14, 16)])


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("pixel,win,P,S", E_CASES)
def test_e_patch_gather_bits(pixel, win, P, S, f16):
    batch = 3
    images = u8_images(batch, S, S) if pixel in (R.PIX_U8_AFFINE, R.PIX_U8_TABLE) else f32_planes(batch, S, S)
    w = R.window(win, P, _kh(P))
    rows = batch * (S // w["stride"]) ** 2
    st, got = launch_gather(pixel, win, f16, images, P, w["half"], 2 * w["half"], rows)
    assert st == 0
    want = R.gather_expected(pixel, win, f16, images, lut(), P, w["half"], rows + 2)
    ntap = 3 * w["ks"] ** 2
    assert ntap < w["half"]
    if w["zero_pad"]:                               # pad columns of both halves: zeros of the operand type
        assert np.all(want[:rows, ntap:w["half"]] == 0) and np.all(want[:rows, w["half"] + ntap:] == 0)
    else:                                           # left to the allocation
        assert np.all(want[:, ntap:w["half"]] == 0xFFFF) and np.all(want[:, w["half"] + ntap:] == 0xFFFF)
    assert np.all(want[rows:] == 0xFFFF)
    _diff(got.ravel(), want.ravel(), "a0")
    if win == R.WIN_7X7 and S == 8:                 # token (0, 1, 1) covers rows 2 .. 8: its last tap row is outside
        assert np.all(want[3, 6 * 21:7 * 21] == 0) and not np.all(want[3, 5 * 21:6 * 21] == 0)


def test_e_bgr_flip_reads_plane_2_minus_c():
    """PixelF32Planes<true> reads plane 2 - c for memory channel c, PixelF32Planes<false> plane c: constant planes tell them apart"""
    S = 8
    planes = np.empty((3, 3, S, S), F32)
    for c in range(3):
        planes[:, c] = c + 1
    _, flip = launch_gather(R.PIX_F32_FLIP, R.WIN_4X4, 0, planes, 0, 64, 128, 12)
    _, keep = launch_gather(R.PIX_F32, R.WIN_7X7, 0, planes, 0, 160, 320, 12)
    for c in range(3):
        assert np.all(R.from_op(flip[:12, c:48:3], 0) == 3 - c)
        centre = R.from_op(keep[:12, (3 * 7 + 3) * 3 + c], 0)       # tap (3, 3) is inside the image for every token
        assert np.all(centre == c + 1)


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("P", [8, 14, 16])
def test_e_patchify_u8_bits(P, f16):
    batch, S = 3, 3 * P
    images = u8_images(batch, S, 50 + P)
    rows = batch * 9
    st, got = launch_gather(R.PIX_U8_RAW, R.WIN_PATCH, f16, images, P, 0, 3 * P * P, rows)
    assert st == 0
    _diff(got.ravel(), R.patchify_raw_expected(images, P, f16, rows + 2).ravel(), "a0")


# ---- F: the LDS-tiled uint8 stems ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("S", [8, 260, 288])
def test_f_ccip_stem_equals_generic_gather(S, f16):
    """H0 = 2: one token a row; 65: a last x-tile of one token; 72: a last x-tile of eight.  The generic gather of the same pixels is
    patch_gather_kernel with Window7x7 on the float32 planes lut[c][byte] (a table read is exact), run into zeroed memory: Window7x7 leaves
    its pad columns to the allocation, the stem must write zeros there -- its buffer starts as 0xff."""
    batch, H0 = 2, S // 4
    images = u8_images(batch, S, 60 + S)
    table = lut()
    rows = batch * H0 * H0
    out = np.full(((rows + 2) * 320,), 0x5A5A, np.uint16)
    st = _lib().hiptsdbg_ccip_stem_u8(_ptr(images), _ptr(table), batch, S, f16, FILL, _ptr(out), out.nbytes)
    assert st == 0
    out = out.reshape(rows + 2, 320)
    planes = np.ascontiguousarray(np.stack([table[c][images[..., c]] for c in range(3)], 1))
    st, generic = launch_gather(R.PIX_F32, R.WIN_7X7, f16, planes, 0, 160, 320, rows, extra_rows=0, fill=0)
    assert st == 0
    _diff(out[:rows].ravel(), generic.ravel(), "stem rows against the generic gather")
    assert np.all(out[:rows, 147:160] == 0) and np.all(out[:rows, 307:] == 0) and np.all(out[rows:] == 0xFFFF)
    want = R.gather_expected(R.PIX_F32, R.WIN_7X7, f16, planes, None, 0, 0, rows, fill16=0)
    _diff(out[:rows].ravel(), want.ravel(), "stem rows against the numpy restatement")


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("grid", [1, 3, 17, 28])
def test_f_vit_patchify_p16_equals_generic(grid, f16):
    """x-groups of 16 tokens: grid 1 and 3 are one ragged group, 17 a full group and a group of one, 28 a full group and one of twelve"""
    batch, S = 2, 16 * grid
    images = u8_images(batch, S, 70 + grid)
    rows = batch * grid * grid
    out = np.full(((rows + 2) * 768,), 0x5A5A, np.uint16)
    st = _lib().hiptsdbg_vit_patchify_u8_p16(_ptr(images), batch, grid, f16, FILL, _ptr(out), out.nbytes)
    assert st == 0
    st, generic = launch_gather(R.PIX_U8_RAW, R.WIN_PATCH, f16, images, 16, 0, 768, rows)
    assert st == 0
    _diff(out, generic.ravel(), "patchify_u8_p16_kernel against patchify_u8_kernel")
    _diff(out, R.patchify_raw_expected(images, 16, f16, rows + 2).ravel(), "patchify_u8_p16_kernel against the numpy restatement")


# ---- G: refusals -----------------------------------------------------------------------------------------------------------------------------------
def _refused(st, *buffers):
    assert st == -1
    for buf in buffers:                             # nothing was launched, nothing copied back: the host buffers keep their own pattern
        assert np.all(buf.view(np.uint8) == 0x5A)


def test_g_refusals():
    v = variant("f32and16")
    g, b = R.gamma_beta(8)
    ok = np.zeros((4, 8), F32)
    _refused(*launch_row_ln(v, 0, np.zeros((4, 6), F32), g[:6], b[:6], 0.0))                          # D = 6
    big = np.zeros((1, 1028), F32)
    _refused(*launch_row_ln(v, 0, big, big[0], big[0], 0.0))                                           # D = 1028
    for name in ("blocked16_add0", "inplace_blocked"):                                                 # a blocked layout with rows = 20
        st, o32, o16 = launch_row_ln(variant(name), 0, np.zeros((32, 16), F32), np.ones(16, F32), None, 0.0, raw=dict(rows=20))
        _refused(st, o32, o16)
    _refused(*launch_row_ln(variant("blocked16_add0"), 0, np.zeros((16, 32), F32), np.ones(32, F32), None, 0.0, raw=dict(D=24)))      # ... or D % 16 != 0
    # tuples no forward launches: LnGamma<false> into a 16-bit sink, the e4m3 sink, a blocked source in place
    _refused(*launch_row_ln(v, 0, ok, g, b, 0.0, raw=dict(affine=R.AFF_GAMMA_PLAIN, sink=R.SINK_16, b=None)))
    _refused(*launch_row_ln(variant("opt16_beta"), 0, ok, g, b, 0.0, raw=dict(sink=R.SINK_E4M3)))
    _refused(*launch_row_ln(variant("tof32"), 0, ok, g, b, 0.0, raw=dict(src=R.SRC_F32_BLOCKED)))
    _refused(*launch_row_ln(variant("tof32"), 1, ok, g, b, 0.0))                                       # no operand type to choose
    _refused(*launch_row_ln(variant("patch2x2"), 0, np.zeros((9, 8), F32), g, b, 0.0, H=3))            # odd H
    _refused(*launch_row_ln(variant("patch2x2"), 0, np.zeros((6, 8), F32), g, b, 0.0, H=2))            # rows != batch * H * H
    for name, short in (("f32and16", "f32"), ("f32and16", "o16"), ("opt16_beta", "o16"), ("tof32", "f32"), ("addhilo", "o16"), ("inplace_rowmajor", "f32")):
        vv = variant(name)                                                                                   # an output buffer one byte short
        x0 = ok if name == "addhilo" else None
        _refused(*launch_row_ln(vv, 0, ok, g, b if vv[6] else None, 0.0, x0=x0, short=short))
    assert launch_row_ln(v, 0, ok + np.arange(8, dtype=F32), g, b, 0.0)[0] == 0                         # and the same call, whole, is accepted


def test_g_refusals_pool_and_gather():
    x = np.zeros((2, 16, 16), F32)
    g = np.ones(16, F32)
    _refused(*launch_pool(x, g, g, 16, 0, 0.0, 0, 0, short=True))
    st, out = launch_pool(x, g, g, 16, 0, 0.0, 0, 1)                                                    # PooledF32 has no operand type
    _refused(st, out)
    st, out = launch_pool(x, g, g, 12, 1, 0.0, 0, 0, T=12)                                              # blocked with T % 16 != 0
    _refused(st, out)
    st, out = launch_pool(np.zeros((1, 2, 1028), F32), np.ones(1028, F32), np.ones(1028, F32), 2, 0, 0.0, 0, 0)      # C > 1024
    _refused(st, out)
    img = u8_images(1, 8, 1)
    for pixel, win in ((R.PIX_U8_TABLE, R.WIN_7X7), (R.PIX_U8_AFFINE, R.WIN_4X4), (R.PIX_F32, R.WIN_PATCH), (R.PIX_U8_RAW, R.WIN_4X4)):
        data = img if pixel != R.PIX_F32 else f32_planes(1, 8, 1)
        _refused(*launch_gather(pixel, win, 0, data, 4, 64, 320, 4))                                    # unlisted (pixel, window) tuples
    _refused(*launch_gather(R.PIX_U8_TABLE, R.WIN_4X4, 0, img, 0, 64, 128, 4, short=True))              # a0 one byte short
    _refused(*launch_gather(R.PIX_U8_AFFINE, R.WIN_PATCH, 0, img, 3, 64, 128, 4))                       # S % P != 0
    out = np.full(2 * 2 * 320, 0x5A5A, np.uint16)
    _refused(_lib().hiptsdbg_ccip_stem_u8(_ptr(img), _ptr(lut()), 1, 8, 0, FILL, _ptr(out), 2 * 2 * 320 * 2 - 1), out)
    _refused(_lib().hiptsdbg_vit_patchify_u8_p16(_ptr(u8_images(1, 16, 2)), 1, 1, 0, FILL, _ptr(out), 768 * 2 - 1), out)
