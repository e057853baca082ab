"""No GPU: the constructions of tests/attention_exact.py are what they claim, and its comparisons reject wrong answers.

Reference check: the plain float64 softmax (test_gpu_attention._reference; swinv2_ref.window_attention for the windows) of every built
input, at every length the GPU tests use, equals the closed form -- so a GPU failure means the kernel.

Negative controls: the comparison functions that the GPU tests call must reject a float64 result computed with a defect -- a key dropped
or counted twice, padded keys left unmasked, rows or heads exchanged, a missing or unscaled low half, a window shift or the roll regions
ignored.  Nothing wrong ever runs on a GPU.

Where a defect is required to be rejected.  Counting runs as level x form; every one of the four has to reject every defect at every
length where the defect exists at all:
  * padded keys exist when tokens is no multiple of 64 (64 and 128 have none);
  * key G (the first key of the second tile) exists when tokens > G;
  * the tile form keeps a single tile's keys in one column, so with tokens <= G its answer does not depend on how many keys were summed:
    a dropped or doubled key is then the position form's to find (asserted below: it does).
LENIENT lists the only two cases that need not reject, both with bf16 output (a relative spacing of 2^-8 .. 2^-7); where one of them does
not, its counterpart (level -16, the position form) rejects the same defect at the same length -- asserted, not assumed.
Exchanged rows are invisible to counting (every row has the same answer) and a doubled key or a padded key at score 0 is invisible to
the permutation (the target keeps all the weight): those are the other construction's to find."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import attention_exact as ax  # noqa: E402
import swinv2_ref  # noqa: E402
from test_gpu_attention import _reference  # noqa: E402

LENGTHS = {64: [16, 33, 64, 65, 96, 97, 127, 128, 129, 200, 257, 784, 1025], 32: [16, 33, 97, 144, 576]}
CASES = [(t, hd) for hd in (64, 32) for t in LENGTHS[hd]]
SPLIT_LENGTHS = [97, 784, 1025]
BH = 6                                                        # batch 2 x heads 3
WINDOWS = [(4, 12, 0), (4, 12, 2), (7, 21, 0), (7, 21, 3), (8, 24, 4), (14, 42, 7), (16, 48, 0), (16, 48, 8)]

LENIENT = {("pad_unmasked", "level", 0), ("double", "form", "tile")}       # bf16 only; nothing else may be added here


def _attend(q, k, v, weight=None, pad=0):
    """Float64 softmax attention in the log2 domain with key multiplicities `weight` [tokens] (0: dropped, 2: counted twice) and `pad`
    further keys with k = 0, v = 0 that take part unmasked."""
    s = q.astype(np.float64) @ k.astype(np.float64).transpose(0, 2, 1)
    v = v.astype(np.float64)
    if pad:
        s = np.concatenate([s, np.zeros(s.shape[:2] + (pad,))], axis=2)
        v = np.concatenate([v, np.zeros((v.shape[0], pad, v.shape[2]))], axis=1)
    p = np.exp2(s - s.max(axis=2, keepdims=True))
    if weight is not None:
        p[:, :, :len(weight)] *= weight
    return (p / p.sum(axis=2, keepdims=True)) @ v


def _key_weight(tokens, key, w):
    a = np.ones(tokens)
    a[key] = w
    return a


def _pad(tokens):
    return -tokens % 64


_PERM = {}


def _perm_case(tokens, hd, f16):
    """The permutation inputs and their float64 softmax, computed once and shared (read only) by the tests that need them."""
    if (tokens, hd, f16) not in _PERM:
        q, k, v, want, sg = ax.permutation(BH, tokens, hd, f16)
        _PERM[tokens, hd, f16] = (q, k, v, want, sg, _reference(q, k, v))
    return _PERM[tokens, hd, f16]


# ------------------------------------------------------------------------------------------------------------ reference checks
@pytest.mark.parametrize("tokens,hd", CASES)
def test_counting_closed_form_is_the_float64_softmax(tokens, hd):
    for level in (0, -16):
        for form in ("pos", "tile"):
            q, k, v, want = ax.counting(BH, tokens, hd, level, form)
            for f16 in (0, 1):                                # every input value is a 16-bit value in both types
                for t in (q, k, v):
                    np.testing.assert_array_equal(ax.to_op(t, f16), t)
            ref = _reference(q, k, v)
            assert np.abs(ref - want).max() <= 1e-9
            if level:
                s = np.einsum("bqd,bkd->bqk", q.astype(np.float64), k.astype(np.float64))
                assert (s == -16.0).all()
            assert want.shape == (BH, tokens, hd) and np.abs(want.sum(axis=2) - 2.0 ** (np.arange(BH) % 4)[:, None]).max() <= 1e-12
            for f16 in (0, 1):
                assert not ax.counting_bad(ref, want, f16).any()


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("tokens,hd", CASES)
def test_permutation_closed_form_is_the_float64_softmax(tokens, hd, f16):
    q, k, v, want, sg, ref = _perm_case(tokens, hd, f16)
    assert sorted(sg) == list(range(tokens))                  # every key is some row's target, once
    for t in (q, k, v):
        np.testing.assert_array_equal(ax.to_op(t, f16), t)
    s = q[0].astype(np.float64) @ k[0].astype(np.float64).T
    assert (s[np.arange(tokens), sg] == 72.0).all()
    s[np.arange(tokens), sg] = -1.0
    assert s.max() <= 48.0 and ((s == 48.0).sum(axis=1) <= 45).all()
    assert not np.array_equal(v[0], v[1])                     # distinct per (image, head)
    vmax = float(np.abs(v).max())
    assert np.abs(ref - want).max() <= ax.LEAK * vmax
    assert not ax.permutation_bad(ref, want, f16, vmax).any()


@pytest.mark.parametrize("tokens", SPLIT_LENGTHS)
def test_permutation_has_rows_that_leave_the_half_fast_path(tokens):
    """The rows that the hi | lo GPU case counts on for the fallback (which writes both halves itself): none at 97 tokens -- every target
    there shares two digits with one of the first keys -- and at least a third of the rows of the two production lengths."""
    q, k, _, _, _ = ax.permutation(1, tokens, 64, 1)
    n = len(ax.half_overflow_rows(q[0], k[0]))
    print("%d tokens: %d rows overflow the half fast path" % (tokens, n))
    assert n == 0 if tokens == 97 else n >= tokens // 3


# ------------------------------------------------------------------------------------------------------------ negative controls
def _counting_defects(tokens, hd, q, k, v, want):
    """{name: defective float64 result} for the defects that exist at this length."""
    G = ax.tile_keys(hd)
    out = {"drop_last": _attend(q, k, v, _key_weight(tokens, tokens - 1, 0.0)),
           "double": _attend(q, k, v, _key_weight(tokens, 0, 2.0)),
           "heads_swapped": _reference(q, k, v)[[1, 0, 2, 3, 4, 5]]}
    if tokens > G:
        out["drop_key_G"] = _attend(q, k, v, _key_weight(tokens, G, 0.0))
    if _pad(tokens):
        out["pad_unmasked"] = _attend(q, k, v, pad=_pad(tokens))
    return out


@pytest.mark.parametrize("tokens,hd", CASES)
def test_counting_comparison_rejects_every_defect(tokens, hd):
    G = ax.tile_keys(hd)
    rejected = {}
    for level in (0, -16):
        for form in ("pos", "tile"):
            q, k, v, want = ax.counting(BH, tokens, hd, level, form)
            q, want = q[:, :2], want[:, :2]                   # every query row is the same: two of them lose nothing
            for name, wrong in _counting_defects(tokens, hd, q, k, v, want).items():
                for f16 in (0, 1):
                    rejected[name, level, form, f16] = bool(ax.counting_bad(wrong, want, f16).any())
    for (name, level, form, f16), rej in sorted(rejected.items(), key=str):
        if rej:
            continue
        if form == "tile" and tokens <= G and name in ("drop_last", "double"):
            assert rejected[name, level, "pos", f16], (name, level, f16)          # one tile, one column: the position form's to find
            continue
        assert f16 == 0 and ((name, "level", level) in LENIENT or (name, "form", form) in LENIENT), (name, level, form, f16)
        other = (name, -16, form, f16) if name == "pad_unmasked" else (name, level, "pos", f16)
        assert rejected[other], other


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("tokens,hd", CASES)
def test_permutation_comparison_rejects_every_defect(tokens, hd, f16):
    q, k, v, want, sg, ref = _perm_case(tokens, hd, f16)
    vmax = float(np.abs(v).max())
    r = tokens // 2
    swapped = ref.copy()
    swapped[:, [r, r + 1]] = ref[:, [r + 1, r]]
    wrong = {"rows_swapped": swapped, "heads_swapped": ref[[1, 0, 2, 3, 4, 5]],
             "drop_last": _attend(q, k, v, _key_weight(tokens, tokens - 1, 0.0))}
    if tokens > ax.tile_keys(hd):
        wrong["drop_key_G"] = _attend(q, k, v, _key_weight(tokens, ax.tile_keys(hd), 0.0))
    for name, w in wrong.items():
        assert ax.permutation_bad(w, want, f16, vmax).any(), name


def _split(x, f16, scale):
    """A correct hi | lo pair of float64 values: the value rounded to 16 bits, and the rest times `scale` rounded to 16 bits."""
    hi = ax.to_op(x.astype(np.float32), f16)
    lo = ax.to_op(((x - hi.astype(np.float64)) * scale).astype(np.float32), f16)
    return hi, lo


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("tokens", SPLIT_LENGTHS)
def test_split_comparison_rejects_a_missing_or_unscaled_low_half(tokens, f16):
    """The position form is the one held to this: its answers 1 / tokens and 2 / tokens (16 and 17 at 1025) need their low half.  The tile
    form's few values can lie next to a 16-bit number by accident (64 / 1025 is within 2^-20 of an IEEE half), the permutation's are 16-bit
    numbers to begin with; they are only shown to pass."""
    scale = ax.split_lo_scale(f16)
    for level in (0, -16):
        for form in ("pos", "tile"):
            q, k, v, want = ax.counting(BH, tokens, 64, level, form)
            q, want = q[:, :2], want[:, :2]
            ref = _reference(q, k, v)
            hi, lo = _split(ref, f16, scale)
            assert not ax.split_bad(hi, lo, want, f16, scale).any()
            if form == "tile":
                continue
            assert ax.split_bad(hi, np.zeros_like(lo), want, f16, scale).any()                  # the low half absent
            assert ax.counting_bad(hi, want, f16).sum() == 0                                    # ... which the single-half bound cannot see
            if scale != 1.0:
                assert ax.split_bad(hi, _split(ref, f16, 1.0)[1], want, f16, scale).any()       # written without lo_scale
    q, k, v, want, _, ref = _perm_case(tokens, 64, f16)
    hi, lo = _split(ref, f16, scale)
    assert not ax.split_bad(hi, lo, want, f16, scale, ax.LEAK * float(np.abs(v).max())).any()


# ------------------------------------------------------------------------------------------------------------ SwinV2 windows
def _window_ref(q, k, v, ls, cpb, side, window, shift, **kw):
    t = [torch.from_numpy(np.ascontiguousarray(a)).double() for a in (q, k, v, ls, cpb)]
    return swinv2_ref.window_attention(*t, side, window, shift, **kw).numpy()


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("window,side,shift", WINDOWS)
def test_window_constructions_match_the_float64_window_attention(window, side, shift, f16):
    regions = swinv2_ref.raster_regions(side, window, shift).numpy()
    _, local, grp = ax.window_groups(side, window, shift, regions)
    n_groups = len(np.unique(grp))
    assert n_groups == (16 if shift else 9) and local.max() == window * window - 1      # 3 x 3 windows; shifted: all nine roll regions
    if shift:
        assert len(np.unique(regions)) == 9

    q, k, v, ls, cpb, want = ax.window_counting(2, 2, side, window, shift, regions, f16)
    vmax = float(np.abs(v).max())
    ref = _window_ref(q, k, v, ls, cpb, side, window, shift)
    assert np.abs(ref - want).max() <= 1e-9
    assert not ax.window_counting_bad(ref, want, f16, vmax).any()
    if shift:
        assert ax.window_counting_bad(_window_ref(q, k, v, ls, cpb, side, window, 0), want, f16, vmax).any()                    # shift ignored
        assert ax.window_counting_bad(_window_ref(q, k, v, ls, cpb, side, window, shift, mask_value=0.0), want, f16, vmax).any()  # regions ignored

    q, k, v, ls, cpb, want = ax.window_placement(2, 2, side, window, shift, regions, f16)
    ref = _window_ref(q, k, v, ls, cpb, side, window, shift)
    assert np.abs(ref - want).max() <= 1e-9
    assert not ax.window_placement_bad(ref, want, f16).any()
    if shift:       # the roll regions ignored leave the target its weight (100 against 50): that defect is the counting case's to find
        assert ax.window_placement_bad(_window_ref(q, k, v, ls, cpb, side, window, 0), want, f16).any()
