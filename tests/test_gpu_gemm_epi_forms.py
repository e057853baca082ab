"""GPU: the GELU form, which a GEMM tile's epilogue decides once per tile (gelu_tanh 0: erf, SwinV2 and ConvNeXt; 1: tanh, the ViT), and
the q | k | v split for tiles that lie wholly in one of the three (dim % 256 == 0) and for tiles that straddle two -- through
hiptsdbg_gemm_epilogue, with the case builder, the launcher and the float64 references of tests/test_gpu_gemm_epi.py /
tests/gemm_epi_ref.py.

  * GELU, both forms x both operand types x with and without a folded LayerNorm (stat_in) x K = 128 / 192, on three paths of one shape
    (N = 256; the smallest persistent launch whose workgroup 0 carries over to a second tile, the `...-persist-K128` shape of
    test_gpu_gemm_epi.py):  the staged store of whole tiles (M = 65792);  its predicated read-back (M one row short of a whole tile);
    and, without stat_in, the direct store that a row stride of N + 4 takes (no LDS image).  The plan must be `pp` and persistent
    (hiptsdbg_gemm_plan).  "A value does not depend on its path": the rows two launches share are equal bit for bit.  Every row is
    within gemm_epi_ref's bound of the float64 GELU, guards and pad keep the fill pattern, every element inside [M][N] is written.
  * q | k | v: dim 256 (N = 768: a tile lies in one of q, k, v -- M = 512, which the launcher gives the two-workgroups-per-CU loop with
    128-column tiles, and M = 11008, the smallest M it gives the 256-column ping-pong loop), and dim 192 (N = 576: tiles straddle q | k
    and k | v, the per-wave form).  q, k and v each land in their own buffer, the pad rows of every image (tokens_pad > tokens) and the
    guards keep the fill pattern; float64 bound.
  * the output BITS of every launch above, pinned in tests/golden/gemm_epi_forms_bits.json (gemm_epi_bits.json holds the erf form
    only without stat_in and the tanh form only with it, and none of these q | k | v shapes).  The digests were recorded from the
    library of the commit BEFORE the GELU form became a per-tile decision, twice, and the two recordings agreed: that change moved no
    bit, and a later one that treats tiles inside q, k or v on their own (tried with it and dropped, LABNOTES) must not either.
    Regenerate like gemm_epi_bits.json, and only for a change of arithmetic made on purpose:

        HIPTS_FORMS_BITS_REGEN=tests/golden/gemm_epi_forms_bits.json python -m pytest tests/test_gpu_gemm_epi_forms.py -m gpu

  * no scratch: the three hot instantiations and the GELU instantiations of the default paths (each now holds both forms).
"""
import ctypes
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_epi_ref as R  # noqa: E402
import test_gpu_gemm_epi as T  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_epi_forms_bits.json")
REGEN = os.environ.get("HIPTS_FORMS_BITS_REGEN")
GELU_M, GELU_N = 65792, 256          # 257 row tiles on 256 CUs: workgroup 0 runs tiles 0 and 256


def check_bits(key, raw):
    h = hashlib.sha256()
    for name in ("o0", "o1", "o2"):
        if raw.get(name) is not None:
            h.update(raw[name].tobytes())
    if REGEN:
        rec = {}
        if os.path.exists(REGEN):
            with open(REGEN) as f:
                rec = json.load(f)
        rec[key] = h.hexdigest()
        with open(REGEN, "w") as f:
            json.dump(rec, f, indent=0, sort_keys=True)
            f.write("\n")
        return
    with open(GOLDEN) as f:
        assert h.hexdigest() == json.load(f)[key], "%s: the launch's output bits differ from tests/golden/gemm_epi_forms_bits.json" % key


@functools.lru_cache(maxsize=1)
def products(epi, f16, M, N, K):
    """(A W^T, |A| |W|^T) in float64 of the case master's first M rows and N columns: shared by the cases of an (operand type, K)"""
    m = T.master(epi, f16)
    a64, w64 = m["a64"][:M, :K], m["w64"][:N, :K]
    return a64 @ w64.T, np.abs(a64) @ np.abs(w64).T


def check_against_float64(v, got, f16, rows):
    """every output of a launch of `rows` rows against gemm_epi_ref.reference, in blocks of rows; returns the worst error / bound"""
    acc, mag = products(v["epi"], f16, max(rows, GELU_M if v["epi"] == R.GELU else rows), v["N"], v["K"])
    fmt = "f16" if f16 else "bf16"
    worst = 0.0
    for r0 in range(0, rows, 8192):
        r1 = min(rows, r0 + 8192)
        vv = dict(v, M=r1 - r0, row0=r0)
        if v.get("stat_in") is not None:
            vv["stat_in"] = v["stat_in"][:, r0:r1]
        for name, q in R.reference(v["epi"], acc[r0:r1], mag[r0:r1], vv).items():
            ratio = np.abs(T._from16(got[name][r0:r1], f16) - q.val) / q.bound(v["K"], fmt)
            worst = max(worst, float(ratio.max()))
    return worst


def _gelu_ids():
    out = []
    for f16 in (1, 0):
        for K in (128, 192):            # outermost: the float64 products are shared by the eight cases of an (operand type, K)
            for tanh in (0, 1):
                for statin in (0, 1):
                    out.append(pytest.param(f16, K, tanh, statin, id="%s-K%d-%s%s" % ("f16" if f16 else "bf16", K, "tanh" if tanh else "erf", "-statin" if statin else "")))
    return out


@pytest.mark.parametrize("f16,K,tanh,statin", _gelu_ids())
def test_gelu_form_does_not_depend_on_the_path(f16, K, tanh, statin):
    T._default_environment()
    feat = R.STAT_IN if statin else 0
    launches = [("tiles", GELU_M, 0), ("rM", GELU_M - 1, 0)] + ([] if statin else [("direct", GELU_M, GELU_N + 4)])
    got, key = {}, "GELU-%s-K%d-%s%s" % ("f16" if f16 else "bf16", K, "tanh" if tanh else "erf", "-statin" if statin else "")
    for name, M, ld_out in launches:
        p = R.plan(R.GELU, M, GELU_N, K, f16, 1, feat, ld_out, 0, T._cus())
        assert p["loop"] == R.PP and p["mr"] == 8 and p["grid"] < p["tiles_m"] * p["tiles_n"], "%s is not a persistent pp launch: %s" % (name, p)
        v, spec = T.build((R.GELU, f16, M, GELU_N, 1, feat, 0, None), K)
        v["gelu_tanh"] = tanh
        if ld_out:                      # a row stride that is no multiple of 8: the store without the LDS image
            v["ld_out"] = ld_out
            spec["o0"] = (np.uint16, M * ld_out + 2 * ld_out + 64, R.x_index(M, GELU_N, ld_out, 0))
        raw = T.run(v, spec)
        T.check_guards_and_coverage(raw, spec, v)
        got[name] = T.logical(raw, spec, "o0")
        if name == "tiles":             # the other launches must hold the same bits (below), so they are as far from float64
            worst = check_against_float64(v, {"o0": got[name]}, f16, M)
            print("%s %s: error / bound %.4f" % (key, name, worst))
            assert worst <= 1.0
        check_bits("%s-%s" % (key, name), raw)
    assert np.array_equal(got["tiles"][:GELU_M - 1], got["rM"]), "the predicated read-back stores other bits than the store of whole tiles"
    if "direct" in got:
        assert np.array_equal(got["tiles"], got["direct"]), "the direct store holds other bits than the staged store"


QK_SHAPES = [(512, 768, R.DW, "tile"), (11008, 768, R.PP, "tile"), (512, 576, R.DW, "straddle")]


@pytest.mark.parametrize("statin", (0, 1), ids=("", "statin"))
@pytest.mark.parametrize("f16", (1, 0), ids=("f16", "bf16"))
@pytest.mark.parametrize("M,N,loop,kind", QK_SHAPES, ids=["M%d-N%d" % s[:2] for s in QK_SHAPES])
def test_qkv_tile_in_one_third_and_straddling(M, N, loop, kind, f16, statin):
    T._default_environment()
    K, feat, dim = 128, (R.STAT_IN if statin else 0), N // 3
    assert (dim % 256 == 0) == (kind == "tile") and dim % 64 == 0
    p = R.plan(R.QK, M, N, K, f16, 1, feat, 0, dim, T._cus())
    assert p["loop"] == loop, p
    v, spec = T.build((R.QK, f16, M, N, 1, feat, 0, None), K)
    assert v["dim"] == dim and v["heads"] == dim // 64 and v["tokens_pad"] > v["tokens"] and set(spec) == {"o0", "o1", "o2"}
    raw = T.run(v, spec)
    T.check_guards_and_coverage(raw, spec, v)           # the fill pattern in every pad row and guard, every (token, d) of q, k and v written
    got = {name: T.logical(raw, spec, name) for name in spec}
    worst = check_against_float64(v, got, f16, M)
    print("error / bound %.4f" % worst)
    assert worst <= 1.0
    check_bits("QK-%s-M%d-N%d%s-K%d" % ("f16" if f16 else "bf16", M, N, "-statin" if statin else "", K), raw)


def test_no_scratch_in_the_hot_and_the_gelu_instantiations():
    from hiptagsearch import _lib
    f = _lib.load().hiptsdbg_gemm_kernel_resources
    f.argtypes = [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_int)] * 3
    for epi, mr, f16, interior in ((R.RESID_XG, 8, 1, 1), (R.RESID_XG, 8, 0, 1), (R.QK, 8, 1, 0), (R.QK, 8, 0, 0), (R.GELU, 8, 1, 0), (R.GELU, 8, 0, 0),
                                   (R.GELU, 7, 1, 0), (R.GELU, 7, 0, 0), (R.GELU, 6, 1, 0)):
        regs, scratch, lds = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
        assert f(epi, mr, f16, 0, 0, interior, ctypes.byref(regs), ctypes.byref(scratch), ctypes.byref(lds)) == 0, _lib.last_error()
        print(R.EPI_NAMES[epi], 32 * mr, "f16" if f16 else "bf16", "registers", regs.value, "scratch", scratch.value)
        assert scratch.value == 0, "%s (%d rows) spills: %d bytes of scratch per lane" % (R.EPI_NAMES[epi], 32 * mr, scratch.value)
