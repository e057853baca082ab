"""GPU: the attention kernels' output BITS, pinned (csrc/attn.hip, csrc/attn2.hip, csrc/attn3.h).

test_gpu_attention.py holds the kernels to a float64 softmax within a tolerance; this file holds them to themselves: seeded inputs go through
hiptsdbg_attention2 / hiptsdbg_attention_run and the sha256 of the raw 16-bit output must equal the digest in tests/golden/attention_bits.json.
A refactor of the kernels ("same bits out") passes it unchanged.  The per-element arithmetic is fixed by source order (-ffp-contract=off, no
reassociation, the MFMA chain order), so the digests do not move with a rebuild.

A pull request that changes the arithmetic ON PURPOSE (another summation order, another reference exponent, another conversion) regenerates
them on an MI355X, from the commit that holds the new arithmetic, and says so:

    HIPTS_ATTN_BITS_REGEN=tests/golden/attention_bits.json python -m pytest tests/test_gpu_attention_bits.py -m gpu

(the variable names the file to write; every case then records its digest instead of comparing it).

Cases (6 (image, head) pairs, both operand types):
  head_dim 64, kernels attn2 (variant 5), attn2:1, attn2:3, attn2:6, attn: tokens 16 (half a tile), 64, 96 (the last tile holds exactly 32
      keys), 97 (masked last tile, both halves), 300 (two workgroups per (image, head) for every 4-wave geometry), 450 (two chunks for
      variant 6, whose workgroup takes up to 13 blocks; below tokens_pad 128 variant 6 runs variant 5's body);
  head_dim 32, kernel attn: tokens 16, 128, 144;
  "spike": tokens 300 with a +300 score on a late key -- the fast pass reports the row, the workgroup repeats its blocks classically;
  "classic": HIPTS_ATTN_CLASSIC=1 in a child process (the switch is read once per process), attn2 and attn."""
import ctypes
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_gpu_attention import KERNELS64, _bits, _op, _spike  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "attention_bits.json")
REGEN = os.environ.get("HIPTS_ATTN_BITS_REGEN")
BH = 6

CASES = ["%s-hd64-t%d-%s" % (kern, t, op) for kern in KERNELS64 for t in (16, 64, 96, 97, 300, 450) for op in ("bf16", "f16")]
CASES += ["attn-hd32-t%d-%s" % (t, op) for t in (16, 128, 144) for op in ("bf16", "f16")]
CASES += ["%s-hd64-t300-%s-spike" % (kern, op) for kern in KERNELS64 for op in ("bf16", "f16")]
CLASSIC = ["%s-hd64-t300-%s-classic" % (kern, op) for kern in ("attn2", "attn") for op in ("bf16", "f16")]


@functools.lru_cache(maxsize=None)
def _inputs(tokens, hd, f16, spike):
    rng = np.random.RandomState(1000 * hd + 2 * tokens + f16)         # the legacy generator: its stream is frozen across numpy versions
    q = _op(rng.standard_normal((BH, tokens, hd)) * 0.6, f16)          # scores of a few units, like the ViT's
    k = _op(rng.standard_normal((BH, tokens, hd)), f16)
    v = _op(rng.standard_normal((BH, tokens, hd)), f16)
    if spike:
        _spike(q, k, 2, 5, tokens - 20, 300.0, f16)                    # the last of five tiles: the row sum leaves the window late
    tp = (tokens + 63) // 64 * 64
    pad = lambda x: np.concatenate([x, np.zeros((BH, tp - tokens, hd), np.float32)], axis=1)
    qb, kb, vb = (_bits(pad(x), f16) for x in (q, k, v))
    vtb = np.ascontiguousarray(vb.transpose(0, 2, 1))                  # attn.hip takes V transposed: [BH][hd][tokens_pad]
    return qb, kb, vb, vtb, tp


def _digest(case):
    """sha256 of the kernel's raw 16-bit output [tokens][BH * hd] for the case named `case`."""
    from hiptagsearch import _lib
    lib = _lib.load()
    parts = case.split("-")
    kernel, hd, tokens, f16 = parts[0], int(parts[1][2:]), int(parts[2][1:]), int(parts[3] == "f16")
    qb, kb, vb, vtb, tp = _inputs(tokens, hd, f16, "spike" in parts[4:])
    out = np.zeros((1, tokens, BH * hd), np.uint16)
    if kernel.startswith("attn2"):
        variant = int(kernel.split(":")[1]) if ":" in kernel else 0
        fn = lib.hiptsdbg_attention2
        fn.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 7 + [ctypes.c_void_p]
        _lib.check(fn(_lib.ptr(qb), _lib.ptr(kb), _lib.ptr(vb), _lib.ptr(out), 1, BH, tokens, tp, f16, variant, 0, None))
    else:
        fn = lib.hiptsdbg_attention_run
        fn.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 6
        _lib.check(fn(_lib.ptr(qb), _lib.ptr(kb), _lib.ptr(vtb), _lib.ptr(out), 1, BH, tokens, tp, hd, f16))
    return hashlib.sha256(out.tobytes()).hexdigest()


def _check(case, digest):
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


@pytest.mark.parametrize("case", CASES)
def test_attention_output_bits(case):
    _check(case, _digest(case))


@pytest.mark.parametrize("kernel", ["attn2", "attn"])
def test_attention_output_bits_classic_switch(kernel):
    """HIPTS_ATTN_CLASSIC=1: the per-tile-maximum body everywhere, both operand types in one child process."""
    cases = [c for c in CLASSIC if c.startswith(kernel + "-")]
    code = "import sys; sys.path.insert(0, %r); import conftest, test_gpu_attention_bits as t\nfor c in sys.argv[1:]: print('DIGEST', c, t._digest(c))" % HERE
    r = subprocess.run([sys.executable, "-c", code] + cases, capture_output=True, text=True, env=dict(os.environ, HIPTS_ATTN_CLASSIC="1"), timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    got = dict(line.split()[1:] for line in r.stdout.splitlines() if line.startswith("DIGEST "))
    assert sorted(got) == sorted(cases), r.stdout[-1000:]
    for c in cases:
        _check(c, got[c])
