"""GPU: how a GEMM work item starts.  The ping-pong loop (gemm_pp_kernel) and the two-workgroups-per-CU loop (gemm_dw_kernel) do not clear
their accumulators: the first product into an accumulator block of a work item multiplies onto a literal zero, in a peeled first K-tile
(first step).  What can go wrong with that is tested here, one production launch each through hiptsdbg_gemm_epilogue:

  * the first K-tile itself -- K = 64, 128, 192: the only K-tile, the stage-ahead path (nt > 1) and the first restage (t + 2 < nt) -- for
    both operand types, every tile height the plan gives, the interior residual form, a staged epilogue and the dw loop's first step
    (nt = 2, 4, 6 steps: each of its three entry points); every element against float64 with the derived bound of tests/gemm_epi_ref.py;
  * split-K slices that start in the middle of K (the tag head's shape shrunk, in a child process: the split is an opt-in of the environment);
  * nothing carries over to a workgroup's next tile: more tiles than workgroups, the A rows of the last row panel and of every row panel
    that is a second tile all zero -- those panels must come out as x + bias EXACTLY;
  * the hot instantiations use no scratch (hiptsdbg_gemm_kernel_resources): a spilled register's reload drains the residual epilogue's
    stores.

The plan is asserted per case (hiptsdbg_gemm_plan), so a case cannot silently take another loop.  e4m3 operands: hiptsdbg_gemm_epilogue
does not reach that instantiation (it passes 16-bit operands only); the CCIP forward's tests run it.
"""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_epi_ref as R  # noqa: E402
import test_gpu_gemm_epi as E  # noqa: E402  (the debug entry's structs and the 16-bit conversions)

pytestmark = pytest.mark.gpu

FILL32 = np.frombuffer(bytes([E.FILL] * 4), np.float32)[0]


@functools.lru_cache(maxsize=4)
def operands(f16, M, N, K, seed=0):
    """|a| ~ 1, |w| ~ 0.05 as (bit patterns, float64) pairs; float32 vectors"""
    rng = np.random.default_rng(104729 * seed + 2 * K + f16)
    a16, a64 = E._to16(rng.standard_normal((M, K), dtype=np.float32), f16)
    w16, w64 = E._to16(rng.standard_normal((N, K), dtype=np.float32) * np.float32(0.05), f16)
    vec = dict(bias=(rng.standard_normal(N) * 0.1).astype(np.float32), gamma=rng.uniform(0.5, 1.5, N).astype(np.float32),
               rowv=rng.uniform(-0.5, 0.5, M).astype(np.float32), colv=rng.standard_normal(N).astype(np.float32))
    return a16, a64, w16, w64, vec


def launch(epi, f16, a16, w16, bias, x0=None, xb=0, feat=0, gamma=None, shared=0):
    """one launch_gemm on the given operands: {x, o0, stat, probs} as logical [M][N] arrays (those the epilogue writes)"""
    M, K = a16.shape
    N = w16.shape[0]
    keep = [np.ascontiguousarray(a16), np.ascontiguousarray(w16), np.ascontiguousarray(bias, np.float32)]
    c = E.CaseT()
    c.epi, c.M, c.N, c.K, c.f16, c.shared_chip = epi, M, N, K, f16, shared
    c.a, c.w, c.bias = (k.ctypes.data for k in keep)
    c.hd_log2, c.x_blocked, c.sk_ws, c.fill = 6, xb, int(bool(feat & R.SK_WS)), E.FILL
    c.qscale, c.ln_eps, c.star_scale, c.star_bias = 1.0, 1e-6, 0.9, -0.45
    if gamma is not None:
        keep.append(np.ascontiguousarray(gamma, np.float32))
        c.ln_gamma = keep[-1].ctypes.data
    o = E.OutT()
    raw, index = {}, {}
    rows = (M + 15) // 16 * 16 if xb else M
    if epi != R.GELU:
        raw["x"], index["x"] = np.full(rows * N + 64, FILL32, np.float32), R.x_index(M, N, N, xb)
        o.x, o.x_bytes = raw["x"].ctypes.data, raw["x"].nbytes
        if x0 is not None:
            raw["x"][index["x"]] = x0
            x_init = raw["x"].copy()
            c.x_init, c.x_init_bytes = x_init.ctypes.data, x_init.nbytes
    if epi == R.GELU or feat & R.COPY16:
        raw["o0"], index["o0"] = np.zeros(M * N + 64, np.uint16), R.x_index(M, N, N, 0)
        o.out16[0], o.out16_bytes[0] = raw["o0"].ctypes.data, raw["o0"].nbytes
    if feat & R.STAT_PART:
        tiles, stride = (N + 255) // 256, M + 8
        c.stat_stride = stride
        raw["stat"], index["stat"] = np.zeros(2 * tiles * stride + 64, np.float32), R.stat_index(M, tiles, stride)
        o.stat_part, o.stat_part_bytes = raw["stat"].ctypes.data, raw["stat"].nbytes
    if epi == R.HEAD:
        raw["probs"], index["probs"] = np.zeros(M * N + 64, np.float32), R.x_index(M, N, N, 0)
        o.probs, o.probs_bytes = raw["probs"].ctypes.data, raw["probs"].nbytes
    st = E._entry()(ctypes.byref(c), ctypes.byref(o))
    if st != 0:         # valid by construction: a refusal or a HIP error ends the session (nothing more is launched after a fault)
        from hiptagsearch import _lib
        pytest.exit("hiptsdbg_gemm_epilogue failed (%d): %s" % (st, _lib.last_error()), returncode=3)
    return {name: raw[name][index[name]] for name in raw}


def plan_of(epi, M, N, K, f16, shared=0, feat=0):
    return R.plan(epi, M, N, K, f16, shared, feat, 0, 0, E._cus())


def check_against_float64(epi, f16, got, a64, w64, vec, K, x0=None, feat=0):
    """every element within the derived bound; the residual forms' 16-bit copy and row sums as functions of the stored rows"""
    v = dict(K=K, M=a64.shape[0], bias=vec["bias"], x0=x0, gelu_tanh=0, ln_eps=1e-6)
    want = R.reference(epi, a64 @ w64.T, np.abs(a64) @ np.abs(w64).T, v)
    fmt = "f16" if f16 else "bf16"
    worst = {}
    for name, q in want.items():
        is16 = name == "o0"
        g = E._from16(got[name], f16) if is16 else got[name].astype(np.float64)
        worst[name] = float((np.abs(g - q.val) / q.bound(K, fmt if is16 else None)).max())      # a NaN fails the comparison below
    print("error / bound:", {k: round(x, 4) for k, x in worst.items()})
    assert all(x <= 1.0 for x in worst.values()), worst
    if feat & R.COPY16:
        assert np.array_equal(got["o0"], E._round16(got["x"] * vec["gamma"][None, :], f16)), "out_bf16 != 16bit(x * gamma) of the stored x"
    if feat & R.STAT_PART:
        q = R.stats_of_stored(got["x"], got["x"].shape[1])
        assert (np.abs(got["stat"].astype(np.float64) - q.val) <= q.bound(0)).all(), "stat_part is not the row sums of the stored x"


XG = R.STAT_PART | R.COPY16
# (id, epilogue, M, N, features, x_blocked, loop, interior)
FIRST_TILE = [
    ("RESID-M1-N16", R.RESID, 1, 16, 0, 0, R.PP, 0),
    ("RESID-M192", R.RESID, 192, 256, 0, 0, R.PP, 0),
    ("RESID-M224", R.RESID, 224, 256, 0, 0, R.PP, 0),
    ("RESID-M256", R.RESID, 256, 256, 0, 0, R.PP, 0),
    # one 256-row panel is never the interior form: the plan cuts a launch smaller than the chip into 192- / 224-row tiles; the interior
    # form's first K-tile runs at its smallest shape in test_nothing_carries_over_to_the_next_tile below
    ("RESID_XG-M256", R.RESID_XG, 256, 256, XG, 1, R.PP, 0),
    ("GELU-M256", R.GELU, 256, 256, 0, 0, R.PP, 0),
]


@pytest.mark.parametrize("f16", [1, 0], ids=["f16", "bf16"])
@pytest.mark.parametrize("K", [64, 128, 192])
@pytest.mark.parametrize("case", FIRST_TILE, ids=[c[0] for c in FIRST_TILE])
def test_first_k_tile(case, K, f16):
    _, epi, M, N, feat, xb, loop, interior = case
    p = plan_of(epi, M, N, K, f16, 0, feat)
    assert (p["loop"], p["interior"], p["sk_slices"]) == (loop, interior, 1) and p["mr"] in (6, 7, 8) and p["grid"] == p["tiles_m"] * p["tiles_n"], p
    print("tile height", 32 * p["mr"])
    a16, a64, w16, w64, vec = operands(f16, M, N, K)
    x0 = None if epi == R.GELU else vec["rowv"][:, None] + vec["colv"][None, :]
    got = launch(epi, f16, a16, w16, vec["bias"], x0, xb, feat, vec["gamma"] if feat & R.COPY16 else None)
    check_against_float64(epi, f16, got, a64, w64, vec, K, x0, feat)


@pytest.mark.parametrize("f16", [1, 0], ids=["f16", "bf16"])
@pytest.mark.parametrize("K", [64, 128, 192])
def test_first_step_of_the_dw_loop(K, f16):
    """K = 64, 128, 192 are 2, 4 and 6 steps: the first step is the last pair's, the pair before it's, a full pair's"""
    M, N = 300, 272
    p = plan_of(R.RESID, M, N, K, f16)
    assert p["loop"] == R.DW and p["grid"] == 2 * 3, p
    a16, a64, w16, w64, vec = operands(f16, M, N, K)
    x0 = vec["rowv"][:, None] + vec["colv"][None, :]
    got = launch(R.RESID, f16, a16, w16, vec["bias"], x0)
    check_against_float64(R.RESID, f16, got, a64, w64, vec, K, x0)


def xcd_work_id(i, n):
    """csrc/vit_internal.h: the tile a persistent workgroup's work item i stands for among n"""
    q, r, xcd, loc = n >> 3, n & 7, i & 7, i >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + loc


@pytest.mark.parametrize("f16", [1, 0], ids=["f16", "bf16"])
@pytest.mark.parametrize("epi,feat,xb,interior,K", [(R.RESID, 0, 0, 0, 64), (R.RESID_XG, XG, 1, 1, 64), (R.RESID_XG, XG, 1, 1, 128), (R.RESID_XG, XG, 1, 1, 192)],
                         ids=["RESID-K64", "RESID_XG-interior-K64", "RESID_XG-interior-K128", "RESID_XG-interior-K192"])
def test_nothing_carries_over_to_the_next_tile(epi, feat, xb, interior, K, f16):
    """257 row panels of 256 rows on fewer workgroups (the smallest launch that takes 256-row tiles and the interior form on a shared chip).
    Zero A rows in the last row panel and in every panel that is some workgroup's second tile -- which panels those are follows from the
    work-id remap, not from their position --: an accumulator that kept anything of the tile before shows as a difference from x + bias."""
    tiles, N = 257, 256
    M = tiles * 256
    p = plan_of(epi, M, N, K, f16, 1, feat)
    assert (p["loop"], p["mr"], p["interior"], p["tiles_m"], p["tiles_n"]) == (R.PP, 8, interior, tiles, 1) and p["grid"] < tiles, p
    second = sorted({xcd_work_id(i, tiles) for i in range(p["grid"], tiles)})
    assert second, "no workgroup has a second tile"
    zero = sorted(set(second) | {tiles - 1})
    a16, a64, w16, w64, vec = operands(f16, M, N, K, seed=1)
    a16, a64 = a16.copy(), a64.copy()
    for t in zero:
        a16[t * 256:(t + 1) * 256] = 0
        a64[t * 256:(t + 1) * 256] = 0
    x0 = vec["rowv"][:, None] + vec["colv"][None, :]
    got = launch(epi, f16, a16, w16, vec["bias"], x0, xb, feat, vec["gamma"] if feat else None, shared=1)
    for t in zero:
        rows = slice(t * 256, (t + 1) * 256)
        want = x0[rows] + (np.float32(0) + vec["bias"][None, :])
        diff = got["x"][rows].view(np.uint32) != want.view(np.uint32)
        assert not diff.any(), "row panel %d: %d elements differ from x + bias, first at %s" % (t, int(diff.sum()), np.argwhere(diff)[0])
        if feat:
            assert np.array_equal(got["o0"][rows], E._round16(want * vec["gamma"][None, :], f16))
    # the panels in front of the second tiles did multiply: the first panel of workgroup 0 and its successor's predecessor against float64
    for t in (0, second[0] - 1 if second[0] - 1 not in zero else 1):
        rows = slice(t * 256, (t + 1) * 256)
        check_against_float64(epi, f16, {k: g[rows] for k, g in got.items()}, a64[rows], w64,
                              dict(vec, rowv=vec["rowv"][rows]), K, x0[rows], feat)
        assert np.abs(got["x"][rows] - x0[rows] - vec["bias"][None, :]).max() > 0.01, "row panel %d has no product to leak" % t


def _split_k_check():
    """child process (HIPTS_GEMM_SPLITK_HEAD=4): the tag head's launch shrunk, one row panel x two column tiles x four K slices"""
    M, N, K = 32, 512, 1536
    out = {}
    for f16 in (1, 0):
        p = plan_of(R.HEAD, M, N, K, f16, 0, R.SK_WS)
        assert (p["loop"], p["mr"], p["sk_first"], p["sk_slices"]) == (R.PP, 8, 0, 4), p       # slices start at K-tiles 0, 6, 12, 18
        a16, a64, w16, w64, vec = operands(f16, M, N, K)
        got = launch(R.HEAD, f16, a16, w16, vec["bias"], feat=R.SK_WS)
        q = R.reference(R.HEAD, a64 @ w64.T, np.abs(a64) @ np.abs(w64).T, dict(K=K, M=M, bias=vec["bias"]))["x"]
        ratio = float((np.abs(got["x"].astype(np.float64) - q.val) / q.bound(K)).max())
        assert ratio <= 1.0, (f16, ratio)
        again = launch(R.HEAD, f16, a16, w16, vec["bias"], feat=R.SK_WS)
        assert np.array_equal(got["x"].view(np.uint32), again["x"].view(np.uint32)), "two launches differ"
        out["f16" if f16 else "bf16"] = ratio
    print("SPLITK " + json.dumps(out))


def test_split_k_slices_start_in_the_middle_of_k():
    env = {k: v for k, v in os.environ.items() if not k.startswith(("HIPTS_GEMM", "HIPTS_EPI_"))}
    env["HIPTS_GEMM_SPLITK_HEAD"] = "4"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--split-k-child"], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    ratios = json.loads([l for l in r.stdout.splitlines() if l.startswith("SPLITK ")][-1][7:])
    assert set(ratios) == {"f16", "bf16"}


def test_hot_kernels_use_no_scratch():
    """(epilogue, tile rows / 32, interior) of the ViT forward's three ping-pong kernels, both operand types"""
    from hiptagsearch import _lib
    f = _lib.load().hiptsdbg_gemm_kernel_resources
    f.argtypes = [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_int)] * 3
    for epi, mr, interior in ((R.RESID_XG, 8, 1), (R.QK, 8, 0), (R.GELU, 8, 0)):
        for f16 in (1, 0):
            regs, scratch, lds = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
            assert f(epi, mr, f16, 0, 0, interior, ctypes.byref(regs), ctypes.byref(scratch), ctypes.byref(lds)) == 0, _lib.last_error()
            print(R.EPI_NAMES[epi], "f16" if f16 else "bf16", "registers", regs.value, "scratch", scratch.value, "static LDS", lds.value)
            assert 0 < regs.value <= 256 and lds.value > 0
            assert scratch.value == 0, "%s spills: %d bytes of scratch per lane" % (R.EPI_NAMES[epi], scratch.value)
    # a combination nothing is built for is refused, not answered
    assert f(R.GELU, 8, 1, 0, 0, 1, ctypes.byref(regs), ctypes.byref(scratch), ctypes.byref(lds)) != 0


if __name__ == "__main__" and sys.argv[1:] == ["--split-k-child"]:
    _split_k_check()
