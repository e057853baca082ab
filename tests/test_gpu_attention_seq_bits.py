"""GPU: the output BITS of the sequential attention body (csrc/attn2.hip, attn2_seq_body: variant 5, the default geometry), pinned over its tile walk.

test_gpu_attention_bits.py pins every head_dim-64 kernel at six sizes; this file walks the ONE body the ViT and EVA02 forwards run through every
shape of its first / middle / last walk over the 64-key tiles, whose middle part is unrolled by two (the ring slot is a constant of each copy):

  tokens   20   40   80  100  150  190  200  250  300
  nkv       1    1    2    2    3    3    4    4    5      tiles: middle-loop trip counts 0, 1, 2, 3 -- odd and even, and no loop at all
  tail     20   40   16   36   22   62    8   58   44      valid keys of the last tile: <= 32 (its second half is skipped) and > 32

and the last 32-row query block is ragged at every one of them (tokens % 32 != 0); from 150 tokens on an (image, head) takes two workgroups.
Batch 2 x 2 heads, both operand types, through hiptsdbg_attention2 with variant 5 named; plus the forced fallback at 300 tokens (a +300 score
on a late key: the fast pass reports the row, its workgroup repeats its blocks classically).

The digests in tests/golden/attention_seq_bits.json were recorded twice, in two processes, from the library of the commit BEFORE the tile walk
was unrolled, and the two recordings were equal: the walk, the LDS-DMA addressing and the row-sum partials may change, the bits may not.
A pull request that changes the arithmetic on purpose regenerates them on an MI355X and says so:

    HIPTS_ATTN_SEQ_BITS_REGEN=tests/golden/attention_seq_bits.json python -m pytest tests/test_gpu_attention_seq_bits.py -m gpu"""
import ctypes
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_gpu_attention import _bits, _op, _spike  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "attention_seq_bits.json")
REGEN = os.environ.get("HIPTS_ATTN_SEQ_BITS_REGEN")
BATCH, HEADS, HD, VARIANT = 2, 2, 64, 5
TOKENS = (20, 40, 80, 100, 150, 190, 200, 250, 300)

CASES = ["t%d-%s" % (t, op) for t in TOKENS for op in ("bf16", "f16")]
CASES += ["t300-%s-spike" % op for op in ("bf16", "f16")]


@functools.lru_cache(maxsize=None)
def _inputs(tokens, f16, spike):
    bh = BATCH * HEADS
    rng = np.random.RandomState(77000 + 2 * tokens + f16)             # the legacy generator: its stream is frozen across numpy versions
    q = _op(rng.standard_normal((bh, tokens, HD)) * 0.6, f16)          # scores of a few units, like the ViT's
    k = _op(rng.standard_normal((bh, tokens, HD)), f16)
    v = _op(rng.standard_normal((bh, tokens, HD)), f16)
    if spike:
        _spike(q, k, 2, 5, tokens - 20, 300.0, f16)                    # the last of five tiles: the row sum leaves the window late
    tp = (tokens + 63) // 64 * 64
    pad = lambda x: np.concatenate([x, np.zeros((bh, tp - tokens, HD), np.float32)], axis=1)
    return _bits(pad(q), f16), _bits(pad(k), f16), _bits(pad(v), f16), tp


def _digest(case):
    """sha256 of the kernel's raw 16-bit output [BATCH][tokens][HEADS * 64] for the case named `case`."""
    from hiptagsearch import _lib
    lib = _lib.load()
    parts = case.split("-")
    tokens, f16 = int(parts[0][1:]), int(parts[1] == "f16")
    qb, kb, vb, tp = _inputs(tokens, f16, "spike" in parts[2:])
    out = np.zeros((BATCH, tokens, HEADS * HD), np.uint16)
    fn = lib.hiptsdbg_attention2
    fn.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 7 + [ctypes.c_void_p]
    _lib.check(fn(_lib.ptr(qb), _lib.ptr(kb), _lib.ptr(vb), _lib.ptr(out), BATCH, HEADS, tokens, tp, f16, VARIANT, 0, None))
    return hashlib.sha256(out.tobytes()).hexdigest()


@pytest.mark.parametrize("case", CASES)
def test_sequential_attention_output_bits(case):
    digest = _digest(case)
    if REGEN:
        rec = {}
        if os.path.exists(REGEN):
            with open(REGEN) as f:
                rec = json.load(f)
        rec[case] = digest
        with open(REGEN, "w") as f:
            json.dump(rec, f, indent=0, sort_keys=True)
            f.write("\n")
        return
    with open(GOLDEN) as f:
        want = json.load(f)
    assert digest == want[case], case
