"""GPU: the attention kernels on inputs whose answer is known in closed form (tests/attention_exact.py): does every key count once, is
every padded key masked, does every row land where it belongs -- at batch 2 x 3 heads, through every head_dim-64 kernel geometry and
attn.hip at both head sizes, and through one production launch with an output stride and the hi | lo output.

The bounds follow from the 16-bit output type alone (attention_exact: counting_bad, permutation_bad, split_bad), so these tests stay valid
across changes of the kernels' arithmetic that move the recorded digests; tests/test_attention_exact_host.py shows without a GPU that the
constructions are right and that each comparison rejects a dropped or doubled key, unmasked padding, exchanged rows or heads and a
missing or unscaled low half."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import attention_exact as ax  # noqa: E402
from test_gpu_attention import KERNELS64  # noqa: E402

pytestmark = pytest.mark.gpu

BATCH, HEADS = 2, 3
BH = BATCH * HEADS
LENGTHS64 = [16, 33, 64, 65, 96, 97, 127, 128, 129, 200, 257, 784, 1025]
LENGTHS32 = [16, 33, 97, 144, 576]                  # 144 and 576: the CCIP encoder's
CASES = [(t, 64) for t in LENGTHS64] + [(t, 32) for t in LENGTHS32]
LAUNCH_LENGTHS = [97, 784, 1025]
GUARD = 4
COUNTING = [(level, form) for level in (0, -16) for form in ("pos", "tile")]


def _kernels(hd):
    return KERNELS64 if hd == 64 else ["attn"]


def _pad_to(x, tp, tail=None):
    """[BH, tokens, hd] -> [BH, tp, hd]: zero rows behind the real ones, or `tail`."""
    out = np.zeros((x.shape[0], tp, x.shape[2]), np.float32)
    out[:, :x.shape[1]] = x
    if tail is not None:
        out[:, x.shape[1]:] = tail
    return out


def _run(q, k, v, f16, kernel, k_tail=None, v_tail=None):
    """q, k, v float32 [BH, tokens, hd] (16-bit values, q in the log2 domain) as BATCH images of HEADS heads through `kernel`; k_tail /
    v_tail: what the padded rows of K and V hold instead of zeros.  Returns float32 [BH, tokens, hd]."""
    from hiptagsearch import _lib
    lib = _lib.load()
    _, tokens, hd = q.shape
    tp = (tokens + 63) // 64 * 64
    qb, kb = ax.bits(_pad_to(q, tp), f16), ax.bits(_pad_to(k, tp, k_tail), f16)
    vp = _pad_to(v, tp, v_tail)
    out = np.zeros((BATCH, tokens, HEADS * hd), np.uint16)
    if kernel.startswith("attn2"):
        assert hd == 64
        variant = int(kernel.split(":")[1]) if ":" in kernel else 0
        fn = lib.hiptsdbg_attention2
        fn.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 7 + [ctypes.c_void_p]
        _lib.check(fn(_lib.ptr(qb), _lib.ptr(kb), _lib.ptr(ax.bits(vp, f16)), _lib.ptr(out), BATCH, HEADS, tokens, tp, int(f16), variant, 0, None))
    else:
        vT = ax.bits(np.ascontiguousarray(vp.transpose(0, 2, 1)), f16)
        fn = lib.hiptsdbg_attention_run
        fn.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 6
        _lib.check(fn(_lib.ptr(qb), _lib.ptr(kb), _lib.ptr(vT), _lib.ptr(out), BATCH, HEADS, tokens, tp, hd, int(f16)))
    return ax.from_bits(out, f16).reshape(BATCH, tokens, HEADS, hd).transpose(0, 2, 1, 3).reshape(BH, tokens, hd)


def _report(bad, got, want, what):
    """One line per failing case: how many entries, the first of them."""
    if not bad.any():
        return []
    i = tuple(int(x) for x in np.argwhere(bad)[0])
    return ["%s: %d of %d entries, first (bh, row, d) = %s: got %r, want %r" % (what, int(bad.sum()), bad.size, i, float(got[i]), float(want[i]))]


def _counting_failures(tokens, hd, f16, kernels):
    fails = []
    for level, form in COUNTING:
        q, k, v, want = ax.counting(BH, tokens, hd, level, form)
        for kernel in kernels:
            got = _run(q, k, v, f16, kernel)
            fails += _report(ax.counting_bad(got, want, f16), got, want, "%s tokens %d hd %d f16 %d level %d %s" % (kernel, tokens, hd, f16, level, form))
    return fails


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("tokens,hd", CASES)
def test_counting_every_key_counts_once(tokens, hd, f16):
    """Equal scores, indicator V: o[i][d] = s * count_d / tokens in every row, zeros exactly zero.  At level -16 one unmasked padded key
    would outweigh 2^16 real ones; the half fast path runs here on every row."""
    fails = _counting_failures(tokens, hd, f16, _kernels(hd))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("tokens,hd", CASES)
def test_permutation_every_row_finds_its_key(tokens, hd, f16):
    """o[i] = v[sigma(i)]: every row placed, every key addressed once.  bf16 operands stay on the fast path (2^72 < 2^100); with half
    operands the rows whose target lies far above their first keys' maximum take the classic fallback, the others the fast path."""
    q, k, v, want, _ = ax.permutation(BH, tokens, hd, f16)
    vmax = float(np.abs(v).max())
    fails = []
    for kernel in _kernels(hd):
        got = _run(q, k, v, f16, kernel)
        fails += _report(ax.permutation_bad(got, want, f16, vmax), got, want, "%s tokens %d hd %d f16 %d" % (kernel, tokens, hd, f16))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("tokens,hd", [c for c in CASES if c[0] % 64])
def test_padded_keys_data_reaches_no_real_row(tokens, hd, f16):
    """Finite noise in the padded rows of K and V (Q's stay zero, as the contract says) changes no bit: a masked key's score starts at
    -inf, which the MFMA carries through any finite product, its P is 0 and 0 x a finite V adds nothing.  (Non-finite values there would
    break this -- NaN from 0 x inf -- and are outside the contract: the forwards' GEMM epilogues write zeros into the padded rows.)"""
    tp = (tokens + 63) // 64 * 64
    k_tail = ax.pad_noise(BH, tp - tokens, hd, f16, 1 + tokens)
    v_tail = ax.pad_noise(BH, tp - tokens, hd, f16, 2 + tokens)
    for level in (0, -16):
        q, k, v, want = ax.counting(BH, tokens, hd, level, "pos")
        for kernel in _kernels(hd):
            clean = _run(q, k, v, f16, kernel)
            noisy = _run(q, k, v, f16, kernel, k_tail, v_tail)
            np.testing.assert_array_equal(noisy.view(np.uint32), clean.view(np.uint32), err_msg="%s level %d" % (kernel, level))
            assert not ax.counting_bad(noisy, want, f16).any(), (kernel, level)


def _launch(q, k, v, f16, variant, stride, split_lo):
    """One production launch through hiptsdbg_attention2_launch.  Returns the whole buffer as uint16 [BATCH * stride + GUARD, out_ld]."""
    from hiptagsearch import _lib
    lib = _lib.load()
    _, tokens, hd = q.shape
    tp = (tokens + 63) // 64 * 64
    rows = BATCH * stride + GUARD
    out = np.zeros((rows, (2 if split_lo else 1) * HEADS * hd), np.uint16)
    fn = lib.hiptsdbg_attention2_launch
    fn.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_longlong] + [ctypes.c_int] * 8
    _lib.check(fn(_lib.ptr(ax.bits(_pad_to(q, tp), f16)), _lib.ptr(ax.bits(_pad_to(k, tp), f16)), _lib.ptr(ax.bits(_pad_to(v, tp), f16)), _lib.ptr(out),
                  rows, BATCH, HEADS, tokens, tp, int(f16), stride, variant, split_lo))
    return out


def _unpack(buf, tokens, stride, f16, split_lo):
    """The launch buffer taken apart: asserts the fill convention (gap and guard rows untouched, no 0xFFFF left in a real row) and returns
    (hi, lo) float32 [BH, tokens, 64], lo None without split_lo."""
    img = buf[:BATCH * stride].reshape(BATCH, stride, -1)
    assert (img[:, tokens:] == 0xFFFF).all(), "a gap row between two images was written"
    assert (buf[BATCH * stride:] == 0xFFFF).all(), "a guard row behind the last image was written"
    real = img[:, :tokens]
    assert not (real == 0xFFFF).any(), "%d values of real rows were never written" % int((real == 0xFFFF).sum())
    halves = real.reshape(BATCH, tokens, 2 if split_lo else 1, HEADS, 64)
    f = ax.from_bits(halves, f16).transpose(2, 0, 3, 1, 4).reshape(-1, BH, tokens, 64)
    return f[0], (f[1] if split_lo else None)


@pytest.mark.parametrize("split_lo", [0, 1])
@pytest.mark.parametrize("stride_kind", ["tokens_pad", "tokens+3"])
@pytest.mark.parametrize("variant", [0, 6])
@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("tokens", LAUNCH_LENGTHS)
def test_production_launch_stride_and_split_output(tokens, f16, variant, stride_kind, split_lo):
    """launch_attention2 as the forwards call it: rows of an image out_tokens_stride apart (EVA02 passes its padded length), the output as
    a hi | lo pair with lo_scale = split_lo_scale.  From a buffer of 0xFF bytes with four guard rows: every real row written, nothing
    else.  hi alone meets the single-output bounds, hi + lo / lo_scale the split bound (|want| 2^-14 bf16, 2^-18 half; the permutation
    adds its leak term, which is no rounding of the output).  Half operands at 784 and 1025 tokens: the permutation rows whose target
    overflows the fast path come from the classic fallback, which writes both halves itself."""
    stride = (tokens + 63) // 64 * 64 if stride_kind == "tokens_pad" else tokens + 3
    scale = ax.split_lo_scale(f16)
    fails = []
    for level, form in [(-16, "pos"), (0, "tile")]:
        q, k, v, want = ax.counting(BH, tokens, 64, level, form)
        hi, lo = _unpack(_launch(q, k, v, f16, variant, stride, split_lo), tokens, stride, f16, split_lo)
        what = "counting level %d %s" % (level, form)
        fails += _report(ax.counting_bad(hi, want, f16), hi, want, what)
        if split_lo:
            fails += _report(ax.split_bad(hi, lo, want, f16, scale), hi + lo / scale, want, what + " hi + lo")
    q, k, v, want, _ = ax.permutation(BH, tokens, 64, f16)
    vmax = float(np.abs(v).max())
    if f16 and tokens > 97:
        assert len(ax.half_overflow_rows(q[0], k[0])) >= tokens // 3
    hi, lo = _unpack(_launch(q, k, v, f16, variant, stride, split_lo), tokens, stride, f16, split_lo)
    fails += _report(ax.permutation_bad(hi, want, f16, vmax), hi, want, "permutation")
    if split_lo:
        fails += _report(ax.split_bad(hi, lo, want, f16, scale, ax.LEAK * vmax), hi + lo / scale, want, "permutation hi + lo")
    assert not fails, "\n".join(fails)


def test_counting_on_the_classic_path():
    """HIPTS_ATTN_CLASSIC=1 (read once per process, hence the child interpreter): the per-tile running maximum everywhere must count the
    same keys -- every length, both operand types, attn2 and attn."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_attention_exact as t
fails = []
for tokens, hd in t.CASES:
    for f16 in (0, 1):
        fails += t._counting_failures(tokens, hd, f16, ["attn2", "attn"] if hd == 64 else ["attn"])
print("\n".join(fails))
sys.exit(1 if fails else 0)
""" % (ROOT, os.path.join(ROOT, "anime-illust-image-searcher_amd"), HERE)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, HIPTS_ATTN_CLASSIC="1"), timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
