"""GPU: the small kernels at the head and tail of the five forwards, one launch per case through the debug entries beside them --
hiptsdbg_vit_pool (pool_partial_kernel + pool_finalize_kernel), hiptsdbg_eva_assemble, hiptsdbg_eva_colsum, hiptsdbg_swinv2_merge / _split_x /
_mean, hiptsdbg_ccip_ds_im2col, hiptsdbg_convnext_cast -- against tests/tokens_ref.py.  Conventions of tests/test_gpu_rows.py: every output
buffer is given with GUARD bytes behind the launch's extent and comes back whole; the entries fill it with 0xff first, so a guard byte (or a
word nobody owns) that changed was written by the kernel.  Each entry launches through the helper the forward launches through.
  A  copies, gathers, casts and the single add of the token assembly: bit for bit, fill and guard included.
  B  pooling with exact answers (sums of small integers, rows that normalise to exactly +-1): bit for bit, the partial sums too; splits that own
     no tokens hold zeros.
  C  pooling on ordinary numbers against float64: |got - want| <= spacing of the output type at |want| + E32, E32 = four times the largest
     error of the float32 numpy restatement of the same formula on the same case; hi | lo outputs on hi + lo with the spacing of the lo
     half (rows_ref.hilo_bounds).  No bound comes from a kernel's output.
  D  refusals: -1, the host buffers untouched.
tests/test_tokens_host.py shows, without a GPU, that every pooling case here sees a dropped, doubled or misplaced token, a row read that must
not be, an unwritten empty split and a missing lo half.

Printed by class C on an MI355X: E32 of the case, then the largest error seen -- partial sums (float32), then the feature's hi + lo error
for bf16 / f16 with its largest ratio to the bound.  Classes A, B and D: zero differing words; the file runs in 2.6 s.
  vit_pool norm-then-pool 196 tokens, 28 splits, D 768  gauss   partials E32 5.1e-06 err 1.22e-06   feature E32 2.37e-07 err 3.82e-06 (0.48) / 1.04e-07 (0.23)
                                                         offset  partials E32 7.46e-05 err 2.11e-05  feature E32 2.55e-06 err 3.89e-06 (0.37) / 2.81e-07 (0.11)
  vit_pool pool-then-norm 196 tokens, 28 splits, D 768  gauss   partials E32 7.87e-06 err 2.15e-06  feature E32 5.63e-06 err 1.59e-05 (0.42) / 1.75e-06 (0.31)
                                                         offset  partials E32 3.36e-04 err 6.48e-05  feature E32 1.90e-04 err 4.53e-05 (0.20) / 4.91e-05 (0.26)
  vit_pool norm-then-pool 70 tokens, 8 splits, D 260    gauss   partials E32 4.76e-06 err 1.26e-06  feature E32 2.27e-07 err 3.77e-06 (0.48) / 8.93e-08 (0.26)
                                                         offset  partials E32 1.07e-04 err 2.35e-05  feature E32 3.82e-06 err 3.60e-06 (0.31) / 3.01e-07 (0.08)
  vit_pool pool-then-norm 70 tokens, 8 splits, D 260    gauss   partials E32 7.73e-06 err 1.67e-06  feature E32 2.69e-06 err 1.50e-05 (0.43) / 1.11e-06 (0.33)
                                                         offset  partials E32 2.44e-04 err 4.58e-05  feature E32 7.19e-05 err 1.82e-05 (0.17) / 1.69e-05 (0.23)
  eva_colsum + pool_ln np 37, D 260                      gauss   partials E32 2.86e-06 err 7.15e-07  feature E32 2.93e-06 err 2.72e-05 (0.42) / 6.63e-07 (0.19)
                                                         offset  partials E32 9.16e-05 err 2.29e-05  feature E32 9.28e-05 err 2.44e-05 (0.19) / 1.87e-05 (0.20)
  sw_mean T 49, C 1024                                   gauss                                       feature E32 1.00e-06 err 7.45e-06 (0.43) / 3.03e-07 (0.24)
                                                         offset                                      feature E32 2.60e-05 err 1.25e-04 (0.39) / 6.70e-06 (0.22)
(With bf16 the hi + lo error is the lo half's rounding, 2^-18 of the value, not the kernel's arithmetic: the float32 partial sums show that.)
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rows_ref as R  # noqa: E402
import tokens_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
FILL = 0xFF
GUARD = T.GUARD

ENTRIES = {
    "hiptsdbg_vit_pool": "P U64 P P I I I FL I I I I P U64 P U64",
    "hiptsdbg_eva_assemble": "P U64 P P I I I I I I P U64 P U64",
    "hiptsdbg_eva_colsum": "P U64 I I I I I P U64",
    "hiptsdbg_swinv2_merge": "P U64 I I I I I P U64",
    "hiptsdbg_swinv2_split_x": "P U64 I64 I I I P U64",
    "hiptsdbg_swinv2_mean": "P U64 I I I I I P U64",
    "hiptsdbg_ccip_ds_im2col": "P U64 I I I I P U64",
    "hiptsdbg_convnext_cast": "P U64 I64 I I P U64",
    "hiptsdbg_pool_ln": "P U64 P P I I I I I FL I I I P U64",
}


@functools.lru_cache(maxsize=None)
def _lib():
    from hiptagsearch import _lib as L
    lib = L.load()
    types = dict(I=ctypes.c_int, I64=ctypes.c_int64, U64=ctypes.c_uint64, P=ctypes.c_void_p, FL=ctypes.c_float)

    class Entries:
        pass

    def stop_on_hip_error(f, name):
        def call(*args):
            st = f(*args)
            if st == -3:        # HIPTS_ERR_HIP: a runtime call or a kernel failed -- nothing more is started on this device
                pytest.exit("%s: HIP error (%s)" % (name, L.last_error()), 3)
            return st
        return call

    e = Entries()
    for name, sig in ENTRIES.items():
        f = getattr(lib, name)
        f.argtypes = [types[t] for t in sig.split()]
        f.restype = ctypes.c_int
        setattr(e, name[len("hiptsdbg_"):], stop_on_hip_error(f, name))
    return e


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _f32c(a):
    return np.ascontiguousarray(a, F32)


def _out(nbytes, dtype, short=False):
    """a host buffer of the launch's extent plus GUARD bytes, holding a pattern of its own (a refused call leaves it), and the size given
    to the entry: one byte less than the extent when `short`"""
    buf = np.full((nbytes + GUARD) // np.dtype(dtype).itemsize, 0x5A5A5A5A if dtype == np.uint32 else 0x5A5A, dtype)
    return buf, (nbytes - 1 if short else buf.nbytes)


def _diff(got, want, what):
    assert got.size == want.size, "%s: %d words, expected %d" % (what, got.size, want.size)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d words differ, first at %d: got %#x, want %#x" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


def _refused(st, *buffers):
    assert st == -1
    for buf in buffers:                             # nothing was launched, nothing copied back: the host buffers keep their own pattern
        assert np.all(buf.view(np.uint8) == 0x5A)


def _op(f16):
    return "f16" if f16 else "bf16"


# ---- launches ---------------------------------------------------------------------------------------------------------------------------------
def launch_merge(x, f16, short=False, H=None, C=None, x_short=0):
    batch, H0, _, C0 = x.shape
    x = _f32c(x)
    out, nbytes = _out(batch * (H0 // 2) ** 2 * 8 * C0 * 2, np.uint16, short)
    return _lib().swinv2_merge(_ptr(x), x.nbytes - x_short, batch, H or H0, C or C0, f16, FILL, _ptr(out), nbytes), out


def launch_split_x(x, f16, short=False, D=None, x_short=0):
    x = _f32c(x)
    rows, D0 = x.shape
    out, nbytes = _out(rows * 2 * D0 * 2, np.uint16, short)
    return _lib().swinv2_split_x(_ptr(x), x.nbytes - x_short, rows, D or D0, f16, FILL, _ptr(out), nbytes), out


def launch_mean(y, f16, short=False, x_short=0):
    y = _f32c(y)
    batch, tokens, C = y.shape
    out, nbytes = _out(batch * 2 * C * 2, np.uint16, short)
    return _lib().swinv2_mean(_ptr(y), y.nbytes - x_short, batch, tokens, C, f16, FILL, _ptr(out), nbytes), out


def launch_im2col(xn, short=False, H=None, C=None, x_short=0):
    xn = np.ascontiguousarray(xn, np.uint16)
    batch, H0, _, C0 = xn.shape
    out, nbytes = _out(batch * (H0 // 2) ** 2 * 9 * C0 * 2, np.uint16, short)
    return _lib().ccip_ds_im2col(_ptr(xn), xn.nbytes - x_short, batch, H or H0, C or C0, FILL, _ptr(out), nbytes), out


def launch_cast(x, f16, short=False, x_short=0):
    x = _f32c(x)
    out, nbytes = _out(x.size * 2, np.uint16, short)
    return _lib().convnext_cast(_ptr(x), x.nbytes - x_short, x.size // 4, f16, FILL, _ptr(out), nbytes), out


def launch_assemble(tmp, cls, pos0, TS, blocked, short=None, D=None, TS_arg=None, x_short=0):
    tmp, cls, pos0 = _f32c(tmp), _f32c(cls), _f32c(pos0)
    batch, n, D0 = tmp.shape
    M = batch * TS
    x, x_bytes = _out(M * D0 * 4, np.uint32, short == "x")
    blk, blk_bytes = _out((M + 15) // 16 * 16 * D0 * 4 if blocked else 0, np.uint32, short == "blk")
    st = _lib().eva_assemble(_ptr(tmp), tmp.nbytes - x_short, _ptr(cls), _ptr(pos0), batch, n, TS_arg or TS, D or D0, blocked, FILL, _ptr(x), x_bytes, _ptr(blk), blk_bytes)
    return st, x, blk


def launch_colsum(x, n, short=False, D=None, n_arg=None, x_short=0):
    x = _f32c(x)
    batch, TS, D0 = x.shape
    out, nbytes = _out(batch * T.EVA_SPLITS * D0 * 4, np.uint32, short)
    return _lib().eva_colsum(_ptr(x), x.nbytes - x_short, batch, n_arg or n, TS, D or D0, FILL, _ptr(out), nbytes), out


def launch_vit_pool(x, g, b, eps, ptn, splits, f16, short=None, D=None, x_short=0):
    x, g, b = _f32c(x), _f32c(g), _f32c(b)
    batch, tokens, D0 = x.shape
    part, part_bytes = _out(batch * max(1, min(splits, 32)) * D0 * 4, np.uint32, short == "part")
    out, out_bytes = _out(batch * 2 * D0 * 2, np.uint16, short == "out")
    st = _lib().vit_pool(_ptr(x), x.nbytes - x_short, _ptr(g), _ptr(b), batch, tokens, D or D0, eps, ptn, splits, f16, FILL, _ptr(part), part_bytes, _ptr(out), out_bytes)
    return st, part, out


def launch_pool_ln_hilo(part, g, b, eps, count, f16):
    """rows_dbg.hip's entry, as eva.hip chains it behind the column sums: T = the 16 partial rows, count = np, the PooledHiLo sink"""
    part, g, b = _f32c(part), _f32c(g), _f32c(b)
    batch, rows, D = part.shape
    out, nbytes = _out(batch * 2 * D * 2, np.uint16)
    return _lib().pool_ln(_ptr(part), part.nbytes, _ptr(g), _ptr(b), batch, rows, D, count, 0, eps, 1, f16, FILL, _ptr(out), nbytes), out


# ---- A: bit for bit ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("batch,H,C", T.MERGE_SHAPES)
def test_a_sw_merge_bits(batch, H, C, f16):
    x = T.distinct_f32(batch * H * H * C, H + C).reshape(batch, H, H, C)
    st, got = launch_merge(x, f16)
    assert st == 0
    want = T.merge_expected(x, f16)
    rows = batch * (H // 2) ** 2
    body, wbody = got[:rows * 8 * C].reshape(rows, 8 * C), want[:rows * 8 * C].reshape(rows, 8 * C)
    _diff(body[:, :4 * C].ravel(), wbody[:, :4 * C].ravel(), "hi half")
    _diff(body[:, 4 * C:].ravel(), wbody[:, 4 * C:].ravel(), "lo half")
    _diff(got[rows * 8 * C:], want[rows * 8 * C:], "fill past the last row")


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("D", T.SPLIT_D)
@pytest.mark.parametrize("rows", T.SPLIT_ROWS)
def test_a_sw_split_x_bits(rows, D, f16):
    x = T.distinct_f32(rows * D, rows + D).reshape(rows, D)
    st, got = launch_split_x(x, f16)
    assert st == 0
    _diff(got, T.split_x_expected(x, f16), "xh2")


@pytest.mark.parametrize("batch,H,C", T.IM2COL_SHAPES)
def test_a_ds_im2col_bits(batch, H, C):
    xn = T.distinct_u16(batch * H * H * C, H + C).reshape(batch, H, H, C)
    st, got = launch_im2col(xn)
    assert st == 0
    _diff(got, T.im2col_expected(xn), "col")
    Ho = H // 2
    col = got[:batch * Ho * Ho * 9 * C].reshape(batch, Ho, Ho, 3, 3, C)
    outside = np.zeros(col.shape, bool)
    outside[:, 0, :, 0] = True
    outside[:, :, 0, :, 0] = True
    assert np.array_equal(col == 0, outside)                   # the top row's and left column's taps are zero and nothing else is


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("n4", T.CAST_N4)
def test_a_cnx_cast_bits(n4, f16):
    x = T.cast_values(n4)
    st, got = launch_cast(x, f16)
    assert st == 0
    _diff(got, T.cast_expected(x, f16), "xh")


ASSEMBLE_CASES = [shape + (blocked,) for shape in T.ASSEMBLE_SHAPES for blocked in (0, 1)] + [shape + (0,) for shape in T.ASSEMBLE_ROWMAJOR_ONLY]


@pytest.mark.parametrize("batch,n,TS,D,blocked", ASSEMBLE_CASES)
def test_a_eva_assemble_bits(batch, n, TS, D, blocked):
    v = T.distinct_f32(batch * n * D + 2 * D, n + D)
    tmp, cls, pos0 = v[:batch * n * D].reshape(batch, n, D), v[-2 * D:-D], v[-D:]
    st, x, blk = launch_assemble(tmp, cls, pos0, TS, blocked)
    assert st == 0
    want_x, want_blk = T.assemble_expected(tmp, cls, pos0, TS, blocked)
    _diff(x, want_x, "row-major rows")
    _diff(blk, want_blk, "blocked copy")
    if blocked and (batch * TS) % 16:                           # the ragged last block: the rows nobody owns keep the fill
        M = batch * TS
        tail = blk[:(M + 15) // 16 * 16 * D].reshape(-1, D // 16, 16, 16)[-1, :, M % 16:, :]
        assert np.all(tail == T.FILL32)


# ---- B: pooling, exact answers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", T.COLSUM_D)
@pytest.mark.parametrize("pad", T.COLSUM_PAD)
@pytest.mark.parametrize("n", T.COLSUM_NP)
def test_b_eva_colsum_exact(n, pad, D):
    x = T.eva_exact_case(n, pad, D)
    st, got = launch_colsum(x, n)
    assert st == 0
    want = T.eva_colsum64(x, n)
    _diff(got, T.guard32(T.words(want)), "partial column sums")
    for s in T.empty_splits(n, T.EVA_SPLITS):                    # zeros, not the fill
        assert np.all(got[:2 * T.EVA_SPLITS * D].reshape(2, T.EVA_SPLITS, D)[:, s] == 0)


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("C", T.SW_MEAN_C)
@pytest.mark.parametrize("tokens", T.SW_MEAN_T)
def test_b_sw_mean_exact(tokens, C, f16):
    y = T.sw_exact_case(tokens, C)
    st, got = launch_mean(y, f16)
    assert st == 0
    _diff(got, T.guard16(T.hilo_rows(T.sw_mean64(y).astype(F32), f16)), "pooled hi | lo")


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("ptn", [0, 1])
@pytest.mark.parametrize("D", T.VIT_POOL_D)
@pytest.mark.parametrize("tokens,splits", T.VIT_POOL_TS)
def test_b_vit_pool_exact(tokens, splits, D, ptn, f16):
    x, g, b, eps = T.vit_exact_case(tokens, splits, D, ptn)
    st, part, out = launch_vit_pool(x, g, b, eps, ptn, splits, f16)
    assert st == 0
    want_part = T.vit_pool64(x, g, b, eps, ptn, splits)[0]
    feat32 = T.vit_finalize32(want_part.astype(F32), g, b, eps, tokens, ptn)
    want32, want16 = T.vit_pool_expected(want_part, feat32, f16)
    _diff(part, want32, "partial sums")
    _diff(out, want16, "feature hi | lo")
    for s in T.empty_splits(tokens, splits):
        assert np.all(part[:T.POOL_BATCH * splits * D].reshape(T.POOL_BATCH, splits, D)[:, s] == 0)


# ---- C: statistics against float64 -----------------------------------------------------------------------------------------------------------------
def _check_hilo(tag, got16, want, e32, f16):
    batch, D = want.shape
    assert np.all(got16[batch * 2 * D:] == T.FILL16)
    hl = got16[:batch * 2 * D].reshape(batch, 2 * D)
    hi, lo = R.from_op(hl[:, :D], f16).astype(np.float64), R.from_op(hl[:, D:], f16).astype(np.float64)
    bound_hi, bound_sum = R.hilo_bounds(want, e32, f16)
    err_hi, err_sum = np.abs(hi - want), np.abs(hi + lo - want)
    print("C %s %s: E32 = %.3g, hi error %.3g, hi + lo error %.3g, largest hi + lo error / bound %.3g" % (tag, _op(f16), e32, err_hi.max(), err_sum.max(), (err_sum / bound_sum).max()))
    assert np.all(err_hi <= bound_hi) and np.all(err_sum <= bound_sum)


def _check_f32(tag, got32, want, e32):
    n = want.size
    assert np.all(got32[n:] == T.FILL32)
    err = np.abs(got32[:n].view(F32).astype(np.float64).reshape(want.shape) - want)
    print("C %s: E32 = %.3g, float32 error %.3g" % (tag, e32, err.max()))
    assert np.all(err <= e32)


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("kind", T.STAT_INPUT_KINDS)
@pytest.mark.parametrize("ptn", [0, 1])
@pytest.mark.parametrize("tokens,splits,D", T.VIT_STAT)
def test_c_vit_pool_against_float64(tokens, splits, D, ptn, kind, f16):
    x, g, b, eps = T.vit_stat_case(kind, tokens, D)
    part, feat = T.vit_pool64(x, g, b, eps, ptn, splits)
    part32, feat32 = T.vit_pool32(x, g, b, eps, ptn, splits)
    st, got_part, got = launch_vit_pool(x, g, b, eps, ptn, splits, f16)
    assert st == 0
    tag = "vit_pool %s tokens=%d splits=%d D=%d %s" % ("pool-then-norm" if ptn else "norm-then-pool", tokens, splits, D, kind)
    _check_f32(tag + " partials", got_part, part, R.e32_of(part32, part))
    _check_hilo(tag, got, feat, R.e32_of(feat32, feat), f16)


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("kind", T.STAT_INPUT_KINDS)
@pytest.mark.parametrize("n,TS,D", T.EVA_STAT)
def test_c_eva_colsum_then_pool_ln_against_float64(n, TS, D, kind, f16):
    """as eva.hip chains them: the 16 partial rows the first kernel wrote are the second one's input"""
    x, g, b, eps = T.eva_stat_case(kind, n, TS, D)
    part = T.eva_colsum64(x, n)
    part32 = T.eva_colsum32(x, n)
    st, got_part = launch_colsum(x, n)
    assert st == 0
    tag = "eva_colsum + pool_ln np=%d D=%d %s" % (n, D, kind)
    _check_f32(tag + " partials", got_part, part, R.e32_of(part32, part))
    chained = got_part[:part.size].view(F32).reshape(part.shape)
    st, got = launch_pool_ln_hilo(chained, g, b, eps, n, f16)
    assert st == 0
    want = R.pool_ln64(part, g, b, eps, n)
    _check_hilo(tag, got, want, R.e32_of(R.pool_ln32(part32, g, b, eps, n), want), f16)


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("kind", T.STAT_INPUT_KINDS)
@pytest.mark.parametrize("tokens,C", T.SW_STAT)
def test_c_sw_mean_against_float64(tokens, C, kind, f16):
    y = T.sw_stat_case(kind, tokens, C)
    want = T.sw_mean64(y)
    st, got = launch_mean(y, f16)
    assert st == 0
    _check_hilo("sw_mean T=%d C=%d %s" % (tokens, C, kind), got, want, R.e32_of(T.sw_mean32(y), want), f16)


# ---- D: refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_d_refusals_swinv2_ccip_convnext():
    x = np.zeros((1, 4, 4, 8), F32)
    _refused(*launch_merge(x, 0, short=True))                                   # col one byte short
    _refused(*launch_merge(x, 0, x_short=1))                                    # x does not cover the launch
    _refused(*launch_merge(np.zeros((1, 3, 3, 8), F32), 0))                     # odd H
    _refused(*launch_merge(np.zeros((1, 4, 4, 6), F32), 0))                     # C % 4
    assert launch_merge(x, 0)[0] == 0                                           # and the same call, whole, is accepted
    r = np.zeros((5, 8), F32)
    _refused(*launch_split_x(r, 0, short=True))
    _refused(*launch_split_x(r, 0, x_short=1))
    _refused(*launch_split_x(np.zeros((5, 6), F32), 0))                         # D % 4
    assert launch_split_x(r, 0)[0] == 0
    y = np.zeros((2, 3, 8), F32)
    _refused(*launch_mean(y, 0, short=True))
    _refused(*launch_mean(y, 0, x_short=1))
    assert launch_mean(y, 0)[0] == 0
    xn = np.zeros((1, 4, 4, 8), np.uint16)
    _refused(*launch_im2col(xn, short=True))
    _refused(*launch_im2col(xn, x_short=1))
    _refused(*launch_im2col(np.zeros((1, 3, 3, 8), np.uint16)))                 # odd H
    _refused(*launch_im2col(np.zeros((1, 4, 4, 12), np.uint16)))                # C % 8
    assert launch_im2col(xn)[0] == 0
    v = np.zeros(8, F32)
    _refused(*launch_cast(v, 0, short=True))
    _refused(*launch_cast(v, 0, x_short=1))
    assert launch_cast(v, 0)[0] == 0


def test_d_refusals_eva():
    tmp, vec = np.zeros((2, 4, 16), F32), np.zeros(16, F32)
    for short in ("x", "blk"):
        _refused(*launch_assemble(tmp, vec, vec, 6, 1, short=short))
    _refused(*launch_assemble(tmp, vec, vec, 6, 0, short="x"))
    _refused(*launch_assemble(tmp, vec, vec, 6, 1, x_short=1))                  # tmp does not cover the launch
    _refused(*launch_assemble(tmp, vec, vec, 6, 0, TS_arg=4))                   # TS < np + 1
    _refused(*launch_assemble(np.zeros((2, 4, 6), F32), vec, vec, 6, 0))        # D % 4
    _refused(*launch_assemble(np.zeros((2, 4, 24), F32), np.zeros(24, F32), np.zeros(24, F32), 6, 1))      # blocked with D % 16
    assert launch_assemble(np.zeros((2, 4, 24), F32), np.zeros(24, F32), np.zeros(24, F32), 6, 0)[0] == 0  # ... which row-major takes
    assert launch_assemble(tmp, vec, vec, 6, 1)[0] == 0
    x = np.zeros((2, 6, 16), F32)
    _refused(*launch_colsum(x, 4, short=True))
    _refused(*launch_colsum(x, 4, x_short=1))
    _refused(*launch_colsum(x, 4, n_arg=6))                                      # TS < np + 1
    _refused(*launch_colsum(np.zeros((2, 6, 6), F32), 4))                        # D % 4
    _refused(*launch_colsum(np.zeros((1, 3, 1028), F32), 2))                     # D > 1024: more than 256 float4 columns
    assert launch_colsum(x, 4)[0] == 0


def test_d_refusals_vit_pool():
    x, g = np.zeros((2, 5, 8), F32), np.ones(8, F32)
    for short in ("part", "out"):
        _refused(*launch_vit_pool(x, g, g, 0.0, 0, 2, 0, short=short))
    _refused(*launch_vit_pool(x, g, g, 0.0, 0, 2, 0, x_short=1))
    _refused(*launch_vit_pool(np.zeros((2, 5, 6), F32), g[:6], g[:6], 0.0, 0, 2, 0))               # D % 4
    big = np.ones(1028, F32)
    _refused(*launch_vit_pool(np.zeros((1, 2, 1028), F32), big, big, 0.0, 0, 1, 0))                # D > 1024
    for splits in (0, 33):
        _refused(*launch_vit_pool(x, g, g, 0.0, 0, splits, 0))
    assert launch_vit_pool(x + 1, g, g, 1e-6, 0, 2, 0)[0] == 0
