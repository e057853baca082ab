"""GPU: every GEMM epilogue arm the model forwards can reach, one production launch each (hiptsdbg_gemm_epilogue), against the float64
references of tests/gemm_epi_ref.py.  Per case (an arm of gemm_epi_ref.CASES x K):
  * the plan for the device's CU count must be the arm the case claims (a failure, not a skip);
  * every output element against float64 with the derived bound (K + 16) 2^-24 S + F (gemm_epi_ref.Q.bound);
  * exact: (a) guard and pad bytes keep the fill pattern (0xff: a NaN in every format) and every element inside [M][N] was written;
    (b) a 16-bit tensor the header defines as a function of the stored fp32 value equals numpy's float32 evaluation of the kernel's own
    fp32 output; (c) resid_rowmajor_out holds the bits the blocked stream would; (d) probs is the sigmoid of the kernel's logits; (e) two
    launches give identical bytes;
  * cross-arm invariance: the arm's outputs equal, bit for bit, those of the epilogue's general 256-row persistent arm on the rows and
    columns they share -- batch invariance at kernel level;
  * the launch's output BITS, pinned: one sha256 over every buffer the launch returns (x, rowmajor, probs, out16[0..2], stat_part, each whole,
    guard and pad bytes included) must equal the digest in tests/golden/gemm_epi_bits.json under the case's id.  A refactor of the epilogues
    ("same bits out") passes it unchanged: the plan is fixed for the device's CU count, split-K slabs are summed in slice order and the
    arithmetic by source order (-ffp-contract=off), so the digests do not move with a rebuild.
Inputs come from one master per (epilogue, operand type): |a| ~ 1, |w| ~ 0.05, folded LayerNorm rows with |mean| <= 0.5 sigma.

A pull request that changes an epilogue's arithmetic ON PURPOSE (another summation order, another conversion, another plan for a case's
shape) regenerates the digests on an MI355X, from the commit that holds the new arithmetic, and says so:

    HIPTS_GEMM_EPI_BITS_REGEN=tests/golden/gemm_epi_bits.json python -m pytest tests/test_gpu_gemm_epi.py -m gpu

(the variable names the file to write; every case then records its digest instead of comparing it).
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

pytestmark = pytest.mark.gpu

FILL = 0xFF
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_epi_bits.json")
REGEN = os.environ.get("HIPTS_GEMM_EPI_BITS_REGEN")
CHUNK = 2048            # rows of a float64 reference block


class CaseT(ctypes.Structure):
    _fields_ = ([(f, ctypes.c_int32) for f in ("epi", "M", "N", "K", "f16", "shared_chip")] +
                [(f, ctypes.c_void_p) for f in ("a", "w", "bias", "pos", "res_scale", "ln_gamma", "ln_beta", "col_u", "rowstat", "stat_in", "rope", "x_init")] +
                [("x_init_bytes", ctypes.c_uint64)] +
                [(f, ctypes.c_int32) for f in ("tokens", "tokens_pad", "heads", "dim", "hd_log2", "stat_in_blocks", "stat_in_stride", "ln_dim", "rope_tokens",
                                               "stat_stride", "gelu_tanh", "star_kind", "ld_out", "x_blocked", "sk_ws", "fill")] +
                [(f, ctypes.c_float) for f in ("qscale", "ln_eps", "star_scale", "star_bias")])


class OutT(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p), ("rowmajor", ctypes.c_void_p), ("probs", ctypes.c_void_p), ("out16", ctypes.c_void_p * 3), ("stat_part", ctypes.c_void_p),
                ("x_bytes", ctypes.c_uint64), ("rowmajor_bytes", ctypes.c_uint64), ("probs_bytes", ctypes.c_uint64), ("out16_bytes", ctypes.c_uint64 * 3),
                ("stat_part_bytes", ctypes.c_uint64)]


@functools.lru_cache(maxsize=None)
def _entry():
    from hiptagsearch import _lib
    f = _lib.load().hiptsdbg_gemm_epilogue
    f.argtypes = [ctypes.POINTER(CaseT), ctypes.POINTER(OutT)]
    return f


@functools.lru_cache(maxsize=None)
def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _to16(x32, f16):
    """(bit patterns, widened float64) of float32 values rounded to the operand type"""
    if f16:
        h = x32.astype(np.float16)
        return h.view(np.uint16), h.astype(np.float64)
    from hiptagsearch import synth
    r = synth.round_to_bf16(x32)
    return (r.view(np.uint32) >> 16).astype(np.uint16), r.astype(np.float64)


def _from16(bits, f16):
    if f16:
        return bits.view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _round16(x32, f16):
    """float32 -> 16-bit patterns, round to nearest even"""
    return _to16(np.ascontiguousarray(x32, np.float32), f16)[0]


MAX_M = max([c[2] for c in R.CASES] + [70000])
MAX_N = max([c[3] for c in R.CASES] + [3072])
TOKENS, ROPE_TOKENS, TOKENS_PAD = 200, 196, 256


@functools.lru_cache(maxsize=2)
def master(epi, f16):
    """every case of an (epilogue, operand type) draws its rows and columns from here"""
    rng = np.random.default_rng(7919 * epi + f16)
    m = {}
    m["a16"], m["a64"] = _to16(rng.standard_normal((MAX_M, 192), dtype=np.float32), f16)
    m["w16"], m["w64"] = _to16(rng.standard_normal((MAX_N, 192), dtype=np.float32) * np.float32(0.05), f16)
    m["bias"] = (rng.standard_normal(MAX_N) * 0.1).astype(np.float32)
    m["res_scale"] = rng.uniform(0.05, 0.5, MAX_N).astype(np.float32) if epi == R.RESID_LS else rng.uniform(0.8, 1.2, MAX_N).astype(np.float32)
    m["ln_gamma"] = rng.uniform(0.5, 1.5, MAX_N).astype(np.float32)
    m["col_u"] = (rng.standard_normal(MAX_N) * 0.3).astype(np.float32)
    m["pos"] = (rng.standard_normal((TOKENS, MAX_N)) * 0.02).astype(np.float32)
    ang = rng.uniform(-np.pi, np.pi, (ROPE_TOKENS, 32))
    m["rope"] = np.stack([np.sin(ang), np.cos(ang)], -1).astype(np.float32)
    # the initial fp32 stream x0[m][n] = rowv[m] + colv[n]: rows of mean ~ rowv, sigma ~ 1
    m["rowv"] = rng.uniform(-0.5, 0.5, MAX_M).astype(np.float32)
    m["colv"] = rng.standard_normal(MAX_N).astype(np.float32)
    # row statistics of a folded input LayerNorm: sigma in [0.5, 2], |mean| <= 0.5 sigma, as partial (sum, sum of squares) pairs per block
    sigma, mu = rng.uniform(0.5, 2.0, MAX_M), rng.uniform(-0.5, 0.5, MAX_M)
    mu = mu * sigma
    m["sigma"], m["mu"] = sigma, mu
    m["jit"] = rng.uniform(0.95, 1.05, (2, 22, 64))           # per (kind, block, row % 64) factor on the partials
    return m


def stat_partials(m, M, blocks, ln_dim, stride):
    nb = ln_dim / blocks
    j = m["jit"][:, :blocks, np.arange(M) % 64]                  # [2][blocks][M]
    part = np.zeros((blocks, stride, 2), np.float32)
    part[:, :M, 0] = nb * m["mu"][None, :M] * j[0]
    part[:, :M, 1] = nb * (m["sigma"][None, :M] ** 2 + m["mu"][None, :M] ** 2) * j[1]
    return part


def build(case, K, blocks=0):
    """(inputs dict for the references, output specs {name: (dtype, raw elements, index [M][cols])}) of a case"""
    epi, f16, M, N, shared, feat, xb, _ = case
    m = master(epi, f16)
    v = dict(epi=epi, f16=f16, M=M, N=N, K=K, shared=shared, feat=feat, xb=xb, bias=m["bias"][:N], qscale=1.0, ln_eps=1e-6, gelu_tanh=0, star_kind=0,
             star_scale=0.9, star_bias=-0.45, tokens=0, tokens_pad=0, heads=0, dim=0, hd_log2=6, ld_out=0, stat_stride=0,
             stat_in_blocks=0, stat_in_stride=0, ln_dim=0, rope_tokens=0)
    ncols = N // 2 if epi == R.SWIGLU else N
    ld = ncols + 16 if feat & R.LDOUT else ncols
    if feat & R.LDOUT:
        v["ld_out"] = ld
    spec = {}
    guard = 2 * ld + 64

    def xspec():
        rows = (M + 15) // 16 * 16 if xb else M
        spec["x"] = (np.float32, rows * ld + guard, R.x_index(M, N, ld, xb))

    resid = epi in (R.RESID, R.RESCALE, R.RESID_LN, R.RESID_ROWSTAT, R.RESID_XG, R.RESID_XGI, R.RESID_LS) and not feat & R.POS
    if resid:
        v["x0"] = m["rowv"][:M, None] + m["colv"][None, :N]           # float32
    if feat & R.POS or epi == R.PATCH:
        v["pos"], v["tokens"], v["qscale"] = m["pos"][:, :N].copy(), TOKENS, 0.5
    if feat & R.RES_SCALE or epi in (R.RESCALE, R.RESID_LS):
        v["res_scale"] = m["res_scale"][:N]
    if feat & R.STAT_IN:
        blocks = blocks or stat_blocks(case)[0]
        # 22 pairs: EVA02-L's fc2 (one per 256-column tile of the SwiGLU launch, 2730 hidden units); else one per 256 columns of the stream
        v["stat_in_blocks"], v["ln_dim"], v["stat_in_stride"] = blocks, (2730 if blocks == 22 else 256 * blocks), M + 8
        v["stat_in"] = stat_partials(m, M, v["stat_in_blocks"], v["ln_dim"], M + 8)
        v["col_u"] = m["col_u"][:N]
    if epi in (R.QK, R.QK_ROPE, R.VT):
        dim = R.case_dim(epi, N)
        hd = 64 if (epi == R.QK_ROPE or (epi == R.QK and N % 192 == 0)) else 32
        v.update(tokens=TOKENS, tokens_pad=TOKENS_PAD, dim=dim, heads=dim // hd, hd_log2=6 if hd == 64 else 5, qscale=0.125 * 1.4426950408889634)
        images = (M + TOKENS - 1) // TOKENS
        raw = images * TOKENS_PAD * dim + 4096
        index = R.vt_index if epi == R.VT else R.qk_index
        for i, name in enumerate(("o0", "o1", "o2")):
            if N > i * dim:
                spec[name] = (np.uint16, raw, index(M, min(N, (i + 1) * dim) - i * dim, TOKENS, TOKENS_PAD, dim // hd, hd))
        if epi == R.QK_ROPE:
            v["rope"], v["rope_tokens"] = m["rope"], ROPE_TOKENS
    elif epi in (R.GELU, R.STAR, R.SWIGLU):
        spec["o0"] = (np.uint16, M * ld + guard, R.x_index(M, ncols, ld, 0))
        v["gelu_tanh"] = 1 if feat & R.STAT_IN else 0           # the ViT's fc1 (tanh form, folded) / ConvNeXt's and SwinV2's (erf form)
        if epi == R.SWIGLU:
            v["ln_gamma"] = m["ln_gamma"][:ncols]
    elif epi == R.HEAD:
        xspec()
        spec["probs"] = (np.float32, M * ld + guard, R.x_index(M, N, ld, 0))
    else:
        xspec()
        if epi == R.RESID_LN or (feat & R.COPY16):
            spec["o0"] = (np.uint16, M * ld + guard, R.x_index(M, N, ld, 0))
            if epi != R.RESID_LS:
                v["ln_gamma"] = m["ln_gamma"][:N]
        if feat & R.ROWMAJOR:
            spec["rowmajor"] = (np.float32, M * ld + guard, R.x_index(M, N, ld, 0))
    if feat & R.STAT_PART:
        tiles, stride = (N + 255) // 256, M + 8
        v["stat_stride"], v["want_stat"] = stride, True
        spec["stat"] = (np.float32, 2 * tiles * stride + 64, R.stat_index(M, tiles, stride))
    return v, spec


def stat_blocks(case):
    """stat_in_blocks of a case's runs.  The kernels branch on stat_in_blocks > 4 (one row_stat loop against request / finish of four
    pairs): the residual epilogues run EVA02-L's 22 pairs and EVA02 tiny's 3, the staged ones 4 (EVA02-L's q|k|v and fc1: dim 1024) or 3
    (the ViT's and the CAFormer's 768-wide streams)."""
    if not case[5] & R.STAT_IN:
        return (0,)
    if case[0] in (R.RESID_ROWSTAT, R.RESID_XGI):
        return (22, 3)
    return (4,) if case[0] in (R.QK_ROPE, R.SWIGLU) else (3,)


def run(v, spec, rowmajor=True):
    """one launch: {name: raw array as copied back}"""
    epi, M, N, K, f16 = v["epi"], v["M"], v["N"], v["K"], v["f16"]
    m = master(epi, f16)
    keep = [np.ascontiguousarray(m["a16"][:M, :K]), np.ascontiguousarray(m["w16"][:N, :K])]
    c = CaseT()
    c.epi, c.M, c.N, c.K, c.f16, c.shared_chip = epi, M, N, K, f16, v["shared"]
    c.a, c.w = keep[0].ctypes.data, keep[1].ctypes.data
    for name in ("bias", "pos", "res_scale", "ln_gamma", "col_u", "stat_in", "rope"):
        if v.get(name) is not None:
            keep.append(np.ascontiguousarray(v[name], np.float32))
            setattr(c, name, keep[-1].ctypes.data)
    for name in ("tokens", "tokens_pad", "heads", "dim", "hd_log2", "stat_in_blocks", "stat_in_stride", "ln_dim", "rope_tokens", "stat_stride", "gelu_tanh",
                 "star_kind", "ld_out"):
        setattr(c, name, int(v[name]))
    c.x_blocked, c.sk_ws, c.fill = v["xb"], int(bool(v["feat"] & R.SK_WS)), FILL
    c.qscale, c.ln_eps, c.star_scale, c.star_bias = v["qscale"], v["ln_eps"], v["star_scale"], v["star_bias"]
    raw = {}
    o = OutT()
    for name, (dtype, elems, index) in spec.items():
        if name == "rowmajor" and not rowmajor:
            continue
        raw[name] = np.zeros(elems, dtype)
        field = {"x": "x", "rowmajor": "rowmajor", "probs": "probs", "stat": "stat_part"}.get(name)
        if field:
            setattr(o, field, raw[name].ctypes.data)
            setattr(o, field + "_bytes", raw[name].nbytes)
        else:
            i = int(name[1])
            o.out16[i] = raw[name].ctypes.data
            o.out16_bytes[i] = raw[name].nbytes
    x_init = None
    if v.get("x0") is not None:            # the stream's initial contents in its layout; everything around it keeps the fill pattern
        x_init = np.full(spec["x"][1], np.frombuffer(bytes([FILL] * 4), np.float32)[0], np.float32)
        x_init[spec["x"][2]] = v["x0"]
        c.x_init, c.x_init_bytes = x_init.ctypes.data, x_init.nbytes
    st = _entry()(ctypes.byref(c), ctypes.byref(o))
    if st != 0:         # the arguments are valid by construction: a refusal or a HIP error ends the session (nothing more is launched after a fault)
        from hiptagsearch import _lib
        pytest.exit("hiptsdbg_gemm_epilogue failed (%d): %s" % (st, _lib.last_error()), returncode=3)
    raw["x_init"] = x_init
    return raw


def bits_of(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def check_bits(key, raw):
    """the launch's buffers in OutT's order (x, rowmajor, probs, out16[0..2], stat_part), each whole, against the pinned digest"""
    h = hashlib.sha256()
    for name in ("x", "rowmajor", "probs", "o0", "o1", "o2", "stat"):
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
    assert h.hexdigest() == _golden()[key], "%s: the launch's output bits differ from tests/golden/gemm_epi_bits.json" % key


def logical(raw, spec, name):
    return raw[name][spec[name][2]]


def check_guards_and_coverage(raw, spec, v):
    """(a)"""
    for name, (dtype, elems, index) in spec.items():
        if name not in raw:
            continue
        outside = np.ones(elems, bool)
        outside[index.ravel()] = False
        fillbits = 0xFFFFFFFF if dtype == np.float32 else 0xFFFF
        if name == "x" and "rowmajor" in raw:       # the new rows left row-major: the blocked stream keeps its contents
            assert np.array_equal(bits_of(raw["x"]), bits_of(raw["x_init"])), "the blocked stream changed although resid_rowmajor_out was given"
            continue
        assert (bits_of(raw[name])[outside] == fillbits).all(), "%s: %d guard / pad elements were written" % (
            name, int((bits_of(raw[name])[outside] != fillbits).sum()))
        assert (bits_of(raw[name])[index.ravel()] != fillbits).all(), "%s: elements inside [M][N] still hold the fill pattern" % name


def reference_shape(case):
    """the general 256-row persistent arm of the case's epilogue, features and stream layout: shared_chip launches of at least as many
    256-row tiles as CUs keep 256 rows (gemm_plan.h); ragged M, so never the interior instantiation"""
    epi, f16, M, N, shared, feat, xb, _ = case
    same = [c for c in R.CASES if (c[0], c[1], c[5] & (R.POS | R.RES_SCALE | R.STAT_IN)) == (epi, f16, feat & (R.POS | R.RES_SCALE | R.STAT_IN))]
    # outputs defined over a whole row / column tile: equal N only; q | k | v: equal N too, so that the split of the columns into the
    # three tensors, the head size and the columns qscale applies to are the case's own
    per_n = epi == R.RESID_LN or bool(feat & R.STAT_PART) or epi in (R.QK, R.QK_ROPE)
    Nref = N if per_n else max(c[3] for c in same)
    tn = (Nref + 255) // 256
    Mref = (_cus() // tn + 1) * 256 - 40        # ragged, and whole groups of 8 rows (EPI_VT)
    return (epi, f16, Mref, Nref, 1, feat & ~R.ROWMAJOR, xb, (R.PP, 8, 0, 1, int(Nref % 256 != 0), 1))


@functools.lru_cache(maxsize=12)
def reference_run(ref_case, K, blocks):
    epi, f16, M, N, shared, feat, xb, claim = ref_case
    p = R.plan(epi, M, N, K, f16, shared, feat, 0, R.case_dim(epi, N), _cus())
    assert R.arm_key(epi, f16, M, N, feat, xb, p) == R.case_key(ref_case), "the reference shape does not take the general persistent arm"
    v, spec = build(ref_case, K, blocks)
    raw = run(v, spec)
    return {name: logical(raw, spec, name) for name in spec}


def _ids():
    out = []
    for case in R.CASES:
        for K in R.case_ks(case):
            for b in stat_blocks(case):
                out.append(pytest.param(case, K, b, id="%s-K%d%s" % (R.key_name(R.case_key(case)), K, "-b%d" % b if b else "")))
    for case in R.k64_cases():
        out.append(pytest.param(case, 64, stat_blocks(case)[0], id="%s-K64" % R.key_name(R.case_key(case))))
    return out


def _default_environment():
    """the plan is asked with the 4-wave mask 0 and the default switches: the launch must run under the same"""
    switches = [k for k in os.environ if k.startswith(("HIPTS_GEMM", "HIPTS_EPI_", "HIPTS_RESID_GENERAL")) and k != "HIPTS_GEMM_EPI_BITS_REGEN"]
    assert switches == [], "the cases are for the default environment, the 4-wave loop (HIPTS_GEMM_Q4) off: %s" % switches


@pytest.mark.parametrize("case,K,blocks", _ids())
def test_epilogue_arm(case, K, blocks):
    _default_environment()
    epi, f16, M, N, shared, feat, xb, claim = case
    p = R.plan(epi, M, N, K, f16, shared, feat, 0, R.case_dim(epi, N), _cus())
    assert R.arm_key(epi, f16, M, N, feat, xb, p) == R.case_key(case), "on %d CUs this shape takes another arm: %s" % (
        _cus(), R.key_name(R.arm_key(epi, f16, M, N, feat, xb, p)))
    v, spec = build(case, K, blocks)
    raw = run(v, spec)
    again = run(v, spec)
    for name in spec:                                                   # (e)
        assert np.array_equal(bits_of(raw[name]), bits_of(again[name])), "%s differs between two launches" % name
    check_guards_and_coverage(raw, spec, v)
    got = {name: logical(raw, spec, name) for name in spec}
    xk = got["rowmajor"] if "rowmajor" in got else got.get("x")       # the float32 rows the kernel stored
    fmt = "f16" if f16 else "bf16"

    # ---- float64, element by element, in blocks of rows
    m = master(epi, f16)
    w64 = m["w64"][:N, :K]
    worst = {}
    for r0 in range(0, M, CHUNK):
        r1 = min(M, r0 + CHUNK)
        a64 = m["a64"][r0:r1, :K]
        vv = dict(v, M=r1 - r0, row0=r0)
        if v.get("x0") is not None:
            vv["x0"] = v["x0"][r0:r1]
        if v.get("stat_in") is not None:
            vv["stat_in"] = v["stat_in"][:, r0:r1]
        want = R.reference(epi, a64 @ w64.T, np.abs(a64) @ np.abs(w64).T, vv)
        for name, q in want.items():
            g = xk[r0:r1] if name == "x" else got[name][r0:r1]
            is16 = name in ("o0", "o1", "o2")
            if is16 and epi in (R.RESID_XG, R.RESID_XGI, R.RESID_LS, R.RESID_LN):
                continue                                                # functions of the stored fp32 rows: checked below
            gv = _from16(g, f16) if is16 else g.astype(np.float64)
            ratio = np.abs(gv - q.val) / q.bound(K, fmt if is16 else None)
            worst[name] = max(worst.get(name, 0.0), float(ratio.max()))
    print("error / bound:", {k: round(x, 4) for k, x in worst.items()})
    assert all(x <= 1.0 for x in worst.values()), worst

    # ---- (b) 16-bit tensors that are functions of the stored fp32 value
    if "o0" in got and epi in (R.RESID_XG, R.RESID_XGI):
        assert np.array_equal(got["o0"], _round16(xk * v["ln_gamma"][None, :], f16)), "out_bf16 != 16bit(x * gamma) of the stored x"
    if "o0" in got and epi == R.RESID_LS:
        assert np.array_equal(got["o0"], _round16(xk, f16)), "out_bf16 != 16bit(x) of the stored x"
    if epi == R.RESID_LN:
        q = R.layernorm_of_stored(xk, v["ln_gamma"], None, v["ln_eps"])
        ratio = np.abs(_from16(got["o0"], f16) - q.val) / q.bound(0, fmt)
        print("RESID_LN xn error / bound:", float(ratio.max()))
        assert ratio.max() <= 1.0
    if "stat" in got and epi in (R.RESID_XG, R.RESID_XGI):
        q = R.stats_of_stored(xk, N)
        ratio = np.abs(got["stat"].astype(np.float64) - q.val) / np.maximum(q.bound(0), 1e-300)
        print("stat_part error / bound:", float(ratio.max()))
        assert ratio.max() <= 1.0
    # ---- (c) the row-major rows are the bits the blocked stream would hold
    if "rowmajor" in got:
        plain = run(v, spec, rowmajor=False)
        assert np.array_equal(bits_of(logical(plain, spec, "x")), bits_of(got["rowmajor"])), "resid_rowmajor_out != the blocked stream's new rows"
    # ---- (d)
    if epi == R.HEAD:
        z = got["x"].astype(np.float64)
        pw = R.sigmoid64(z)
        assert (np.abs(got["probs"] - pw) <= ((8.0 + np.abs(z)) * R.U + R.U) * pw + 2.0 ** -149).all(), "probs is not the sigmoid of the stored logits"

    # ---- cross-arm invariance
    ref_case = reference_shape(case)
    ref = reference_run(ref_case, K, blocks)
    rows, Nr = min(M, ref_case[2]), ref_case[3]
    for name in spec:
        if name == "rowmajor":          # compared as x: the reference writes the same rows into its blocked stream
            continue
        mine = xk if name == "x" else got[name]
        if name == "stat" or (name == "o0" and epi == R.RESID_LN) or epi in (R.QK, R.QK_ROPE):
            assert Nr == N, "the reference of an output defined per row / column tile or per q | k | v split must have the case's N"
        cols = min(mine.shape[1], ref[name].shape[1])
        assert rows > 0 and cols > 0 and cols == (mine.shape[1] if Nr >= N else cols), "%s is compared with nothing" % name
        assert np.array_equal(bits_of(np.ascontiguousarray(mine[:rows, :cols])), bits_of(np.ascontiguousarray(ref[name][:rows, :cols]))), \
            "%s differs from the general 256-row persistent arm on shared rows and columns" % name

    check_bits("%s-K%d%s" % (R.key_name(R.case_key(case)), K, "-b%d" % blocks if blocks else ""), raw)


def test_vt_unstaged_small_images():
    """tokens % 8 != 0 (the CAFormer test geometry's last stage: 4 tokens per image) takes EPI_VT's store path without the LDS image"""
    case = (R.VT, 1, 256, 128, 0, 0, 0, (R.PP, 6, 0, 1, 1, 0))
    v, spec = build(case, 128)
    images = 256 // 4
    v.update(tokens=4, tokens_pad=64)
    spec["o0"] = (np.uint16, images * 64 * 128 + 4096, R.vt_index(256, 128, 4, 64, 4, 32))
    raw = run(v, spec)
    check_guards_and_coverage(raw, spec, v)
    m = master(R.VT, 1)
    a64, w64 = m["a64"][:256, :128], m["w64"][:128, :128]
    q = R.reference(R.VT, a64 @ w64.T, np.abs(a64) @ np.abs(w64).T, v)["o0"]
    assert (np.abs(_from16(logical(raw, spec, "o0"), 1) - q.val) <= q.bound(128, "f16")).all()
    check_bits("test_vt_unstaged_small_images-K128", raw)


def _refused(case, K, blocks, **over):
    """the status and message of a launch the launcher must refuse before anything runs"""
    from hiptagsearch import _lib
    v, spec = build(case, K, blocks)
    v.update(over)
    seen = {}
    real_exit = pytest.exit
    try:
        pytest.exit = lambda msg, returncode=0: seen.setdefault("msg", msg)
        run(v, spec)
    finally:
        pytest.exit = real_exit
    return seen.get("msg", "")


def test_launcher_refuses_what_its_kernels_do_not_do():
    """Two preconditions of the kernels are the launcher's to check: the two-workgroups-per-CU loop's staged epilogues finish a folded
    LayerNorm from four partial pairs at most, and the staged V^T store writes eight tokens at a time."""
    dw_gelu = (R.GELU, 1, 384, 128, 0, R.STAT_IN, 0, (R.DW, 8, 0, 1, 0, 0))
    p = R.plan(R.GELU, 384, 128, 128, 1, 0, R.STAT_IN, 0, 0, _cus())
    assert p["loop"] == R.DW
    assert "at most 4 stat_in pairs" in _refused(dw_gelu, 128, 5)
    vt = (R.VT, 1, 36, 128, 0, 0, 0, (R.PP, 6, 0, 1, 1, 0))
    assert "M % 8 == 0" in _refused(vt, 128, 0)
