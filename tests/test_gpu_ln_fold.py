"""GPU: the folded LayerNorm as the forwards run it -- a producer launch, then a consumer launch on exactly what the producer wrote --
and its two kernels that no GEMM launch contains, against float64 (tests/ln_fold_ref.py; tests/test_ln_fold_host.py is the host twin).

  fold_ln_kernel   (hiptsdbg_fold_ln)  u = W gamma, c = W beta + b from the 16-bit W, both operand types, N not a multiple of a workgroup's
                   four rows, K not a multiple of 64, with beta and bias and without (c must be 0): 2^-24 |u| + K 2^-53 sum |W gamma|.
  rowstat_kernel   (hiptsdbg_rowstat)  against the float64 finish of the same float32 pairs: rstd to (blocks + 12) 2^-24 kappa relative,
                   kappa = (s2 / D) / (var + eps); rstd mean to (blocks + 12) 2^-24 (kappa |rstd mean| + rstd sum_b |s1_b| / D - |rstd mean|):
                   the same relative bound wherever the tiles' sums share a sign, and the magnitude of the mean's own sum where a
                   mean ~ 0 cancels across tiles (a bound relative to the cancelled mean is one no summation meets: measured 12 x
                   over it on the device, rstd at 0.17 of its bound).  Rows whose pairs give s2 / D == mean^2 exactly: 1 / sqrt(eps) to 2 ulp.
  the chain        per wiring of ln_fold_ref.WIRINGS (read off vit_run_images, eva_run_images, ccip_run_images): call 1, the producer
                   (hiptsdbg_gemm_epilogue), returns x, the 16-bit copy and stat_part; call 2, the consumer, receives that copy as its A
                   operand and that stat_part as stat_in (stride and blocks as the forward passes them: stride M) with col_u and bias from
                   hiptsdbg_fold_ln; where the forward can finish the pairs with rowstat_kernel (eva.hip) also through hiptsdbg_rowstat.
                   Reference: float64 Linear(LayerNorm(x)) of the x call 1 returned, through the consumer's activation and layout
                   (gemm_epi_ref.reference); bound: gemm_epi_ref.fold_bound plus the output type's term.  M = 272, every row regime in
                   every launch, grid and generic inputs.
  EVA02's inner norm: EPI_SWIGLU does not return its float32 rows, so the generic chain is three launches (RESID_XG -> SWIGLU at the
                   model's 2 x 2752 columns -> fc2).  Launch 2 is held to its own bound; the rows fc2's LayerNorm sees are read back from
                   the copy launch 2 wrote (x^ = copy / gamma, within e16 |x^| of the float32 rows: ln_fold_ref.rows_of_copy), the 22
                   pairs it returned are held to those rows' sums (ln_fold_ref.pair_bound), and fc2's reference is float64
                   Linear(LayerNorm(x^)) with that e16 |x^| carried through the LayerNorm's derivative (ln_fold_ref.perturbation_bound)
                   on top of fold_bound.  Its hidden rows cannot be dealt per regime (they follow a LayerNorm: mean ~ 0.4, sigma ~ 0.7),
                   so the grid kind hands fc2 the exact copy and the exact pairs of 2730-wide grid rows -- exact in any order, so what
                   any correct producer writes.
  controls         on grid inputs each of: ln_dim the padded width, the pairs' rows shifted by one, one tile's pair dropped -- must miss
                   the bound.
  the record       per (wiring, operand type, regime) max |err| / rms(want) of the folded chain and of the separate path on the same x
                   (hiptsdbg_row_ln into a 16-bit operand, the consumer without the fold), printed; DESIGN.md holds the table."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_epi_ref as R  # noqa: E402
import ln_fold_ref as L  # noqa: E402
import test_gpu_gemm_epi as E  # noqa: E402  (the GEMM debug entry's structs)
import test_gpu_rows as TR  # noqa: E402  (hiptsdbg_row_ln)

pytestmark = pytest.mark.gpu

F32 = np.float32
FILL = 0xFF
FILL32, FILL16 = 0xFFFFFFFF, 0xFFFF
M, EPS = L.M, L.EPS
TOKENS, TOKENS_PAD, ROPE_TOKENS = 136, 192, 130             # two images of 136 rows
WIRING = {w[0]: w for w in L.WIRINGS}
LOG2E = 1.4426950408889634


@functools.lru_cache(maxsize=None)
def _lib():
    from hiptagsearch import _lib as lib
    h = lib.load()
    I, U64, P, FL = ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_float
    h.hiptsdbg_rowstat.argtypes = [P, U64, I, I, I, I, FL, I, P, U64]
    h.hiptsdbg_fold_ln.argtypes = [P, I, P, P, P, I, I, I, P, P, U64]
    return h


def _ok(st, who):
    if st != 0:         # the arguments are valid by construction: a refusal or a HIP error ends the session (nothing more is launched after a fault)
        from hiptagsearch import _lib as lib
        pytest.exit("%s failed (%d): %s" % (who, st, lib.last_error()), returncode=3)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def fold_ln(wbits, f16, gamma, beta, bias, N, K, guard=16):
    """(u, c) float32, each N elements and `guard` more that must come back holding the fill"""
    wbits, gamma = np.ascontiguousarray(wbits, np.uint16), np.ascontiguousarray(gamma, F32)
    beta = None if beta is None else np.ascontiguousarray(beta, F32)
    bias = None if bias is None else np.ascontiguousarray(bias, F32)
    assert wbits.size == N * K and gamma.size == K and (beta is None or beta.size == K) and (bias is None or bias.size == N)
    u, c = np.zeros(N + guard, F32), np.zeros(N + guard, F32)
    _ok(_lib().hiptsdbg_fold_ln(_ptr(wbits), f16, _ptr(gamma), _ptr(beta), _ptr(bias), N, K, FILL, _ptr(u), _ptr(c), u.nbytes), "hiptsdbg_fold_ln")
    return u, c


def rowstat(part, m, stride, blocks, D, eps, guard=8):
    """[m + guard][2] float32 from part, float32 [blocks][stride][2] or the raw buffer a producer launch returned"""
    part = np.ascontiguousarray(part, F32)
    assert part.size >= 2 * blocks * stride and stride >= m
    out = np.zeros((m + guard, 2), F32)
    _ok(_lib().hiptsdbg_rowstat(_ptr(part), part.nbytes, m, stride, blocks, D, eps, FILL, _ptr(out), out.nbytes), "hiptsdbg_rowstat")
    return out


# ---- fold_ln_kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["beta+bias", "none"])
@pytest.mark.parametrize("f16", [1, 0], ids=["f16", "bf16"])
@pytest.mark.parametrize("NK", [(5, 64), (130, 192), (257, 72)], ids=lambda s: "%dx%d" % s)
def test_fold_ln_kernel(NK, f16, form):
    n, k = NK
    _, wbits, w64 = L.weight(n, k, f16, 7 * n + k)
    gamma, beta, b = L.vectors("generic", k, n, 3, form == "beta+bias")
    u, c = fold_ln(wbits, f16, gamma, beta, b, n, k)
    u64, c64, mu, mc = L.fold_vectors64(w64, gamma, beta, b)
    ru, rc = L.ratio(u[:n], u64, L.fold_vector_bound(u64, mu, k)), L.ratio(c[:n], c64, L.fold_vector_bound(c64, mc, k))
    print("error / bound: u %.3f  c %.3f" % (ru.max(), rc.max()))
    assert ru.max() <= 1.0 and rc.max() <= 1.0
    if form == "none":
        assert (c[:n].view(np.uint32) == 0).all(), "without beta and bias c must be +0"
    assert (u[n:].view(np.uint32) == FILL32).all() and (c[n:].view(np.uint32) == FILL32).all(), "elements past N were written"


# ---- rowstat_kernel -----------------------------------------------------------------------------------------------------------------
ROWSTAT_REGIMES = [0, 4, 16, 64, "exact"]


def _rowstat_pairs(m, blocks, D, seed):
    """float32 pairs [blocks][m + 8][2] of rows dealt over ROWSTAT_REGIMES: sigma 1 rows of the given |mean| / sigma, and rows of 2.0
    (s2 / D == mean^2 exactly).  Tile b covers columns [b t, b t + t), t = ceil(D / blocks / 64) * 64 -- 128 for 2730 over 22."""
    rng = np.random.default_rng(seed)
    t = (D + blocks * 64 - 1) // (blocks * 64) * 64
    x = np.zeros((m, blocks * t))
    for r in range(m):
        reg = ROWSTAT_REGIMES[r % len(ROWSTAT_REGIMES)]
        x[r, :D] = 2.0 if reg == "exact" else reg + rng.standard_normal(D)
    xt = x.reshape(m, blocks, t)
    part = np.full((blocks, m + 8, 2), 1e30, F32)                   # rows past m of the stride: never to be read
    part[:, :m, 0], part[:, :m, 1] = xt.sum(2).T, (xt * xt).sum(2).T
    return part


@pytest.mark.parametrize("blocks,D", [(1, 256), (3, 768), (4, 1024), (5, 1280), (22, 5632), (22, 2730)], ids=lambda v: str(v))
@pytest.mark.parametrize("m", [1, 63, 65, 200])
def test_rowstat_kernel(m, blocks, D):
    part = _rowstat_pairs(m, blocks, D, 100 * m + blocks + D)
    out = rowstat(part, m, m + 8, blocks, D, EPS)
    assert (out[m:].view(np.uint32) == FILL32).all(), "rows past M were written"
    p = part.astype(np.float64)
    s1, s2 = p[:, :m, 0].sum(0), p[:, :m, 1].sum(0)
    mean = s1 / D
    var = np.maximum(s2 / D - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + EPS)
    kappa = (s2 / D) / (var + EPS)
    rel = (blocks + 12) * R.U * kappa
    reg = np.arange(m) % len(ROWSTAT_REGIMES)
    exact = reg == ROWSTAT_REGIMES.index("exact")
    # rstd mean inherits rstd's error, (blocks + 12) 2^-24 (kappa - 1) of it, and adds the mean's own: (blocks + 12) 2^-24 of the magnitude
    # of its sum, sum_b |s1_b| / D.  Where the pairs share a sign that magnitude is |mean| and the two add up to (blocks + 12) 2^-24 kappa
    # relative, the bound as stated for rstd; only a row of mean ~ 0 that cancels across its tiles gets more, and no more than its sum's
    magn = rstd * np.abs(p[:, :m, 0]).sum(0) / D
    assert (magn >= np.abs(rstd * mean) * (1.0 - 1e-12)).all()
    brm = (blocks + 12) * R.U * ((kappa - 1.0) * np.abs(rstd * mean) + magn)
    r0, r1 = L.ratio(out[:m, 0], rstd, rel * rstd), L.ratio(out[:m, 1], rstd * mean, brm)
    print("error / bound: rstd %.3f  rstd mean %.3f" % (r0[~exact].max(initial=0.0), r1[~exact].max(initial=0.0)))
    assert r0[~exact].max(initial=0.0) <= 1.0 and r1[~exact].max(initial=0.0) <= 1.0
    if exact.any():         # s2 / D == mean^2 in float32: var is 0, the answer 1 / sqrt(eps) and mean / sqrt(eps)
        want = np.array([1.0 / np.sqrt(np.float64(F32(EPS))), 2.0 / np.sqrt(np.float64(F32(EPS)))])
        ulp = np.spacing(want.astype(F32)).astype(np.float64)
        assert (np.abs(out[:m][exact].astype(np.float64) - want[None, :]) <= 2.0 * ulp[None, :]).all(), out[:m][exact][:2]


# ---- one hiptsdbg_gemm_epilogue call ----------------------------------------------------------------------------------------------------
def gemm_call(fields, arrays, outs):
    """fields: the scalar members of hiptsdbg_gemm_case_t; arrays: its host arrays; outs: {x | rowmajor | stat | o0..o2: (dtype, elements)}
    -> {name: the whole buffer as copied back}"""
    c, o, keep, raw = E.CaseT(), E.OutT(), [], {}
    for k, val in fields.items():
        setattr(c, k, val)
    c.fill = FILL
    for k, a in arrays.items():
        if a is None:
            continue
        a = np.ascontiguousarray(a)
        assert a.dtype == (np.uint16 if k in ("a", "w") else F32), k
        keep.append(a)
        setattr(c, k, a.ctypes.data)
        if k == "x_init":
            c.x_init_bytes = a.nbytes
    for name, (dtype, elems) in outs.items():
        raw[name] = np.zeros(elems, dtype)
        field = {"x": "x", "rowmajor": "rowmajor", "stat": "stat_part"}.get(name)
        if field:
            setattr(o, field, raw[name].ctypes.data)
            setattr(o, field + "_bytes", raw[name].nbytes)
        else:
            o.out16[int(name[1])] = raw[name].ctypes.data
            o.out16_bytes[int(name[1])] = raw[name].nbytes
    _ok(E._entry()(ctypes.byref(c), ctypes.byref(o)), "hiptsdbg_gemm_epilogue")
    return raw


def _stream(x0, N, xb, guard):
    """(elements, index, initial contents) of the float32 stream buffer holding x0 [M][N] row-major or in 16 x 16 blocks, fill around it"""
    rows = (M + 15) // 16 * 16 if xb else M
    index = R.x_index(M, N, N, xb)
    init = np.full(rows * N + guard, np.frombuffer(bytes([FILL] * 4), F32)[0], F32)
    init[index] = x0
    return rows * N + guard, index, init


def _guards_hold(raw, name, index, fill):
    outside = np.ones(raw[name].size, bool)
    outside[index.ravel()] = False
    bits = raw[name].view(np.uint32) if raw[name].dtype == F32 else raw[name]
    assert (bits[outside] == fill).all(), "%s: elements outside the launch's extent were written" % name


def _seed(geom, f16, kind):
    return 10000 + 1000 * sorted(L.GEOMETRY).index(geom) + 10 * f16 + (kind == "grid")


# ---- call 1: the producers ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def produced(geom, f16, kind, epi):
    """what one RESID_XG / RESID_XGI launch of a model's stream wrote: x [M][D] float32, the 16-bit copy's patterns [M][D], the stat_part
    buffer as copied back; with the norm's gamma / beta the copy was made for"""
    g = L.GEOMETRY[geom]
    D, seed = g["D"], _seed(geom, f16, kind)
    feat, xb = next((w[2][1], w[2][2]) for w in L.WIRINGS if w[1] == geom and w[2][0] == epi)
    rng = np.random.default_rng(seed + 5)
    target, scale = L.rows(kind, D, f16, seed, g["m_max"])
    gamma, beta, _ = L.vectors(kind, D, 1, seed + 1, g["beta"])
    _, wbits, _ = L.weight(D, 128, f16, seed + 2)
    const = np.array([L.regimes(kind)[i][5] is not None for i in L.regime_of_row(kind)])
    a32 = np.zeros((M, 128), F32) if kind == "grid" else (rng.standard_normal((M, 128)) * (scale * ~const)[:, None]).astype(F32)
    x0 = target
    arrays = dict(a=L.to16(a32, f16)[0], w=wbits, ln_gamma=gamma)
    if feat & R.RES_SCALE:      # x = x0 rs + acc: the rows the LayerNorm is to see are x0 rs
        rs = np.ones(D, F32) if kind == "grid" else rng.uniform(0.8, 1.2, D).astype(F32)
        x0 = (target / rs[None, :]).astype(F32)
        arrays["res_scale"] = rs
    fields = dict(epi=epi, M=M, N=D, K=128, f16=f16, shared_chip=0, x_blocked=xb, sk_ws=int(bool(feat & R.SK_WS)), stat_stride=M, ln_eps=EPS, qscale=1.0, hd_log2=6)
    if epi == R.RESID_XGI:      # its own folded input: EVA02-L's fc2 reads 22 pairs over 2730 columns.  grid: u = 0, c = 0 and A = 0, so x = x0
        part = np.zeros((22, M, 2), F32)
        part[:, :, 0], part[:, :, 1] = 2730 / 22 * 0.2, 2730 / 22 * 1.04
        arrays.update(stat_in=part, col_u=np.zeros(D, F32) if kind == "grid" else (rng.standard_normal(D) * 0.3).astype(F32),
                      bias=np.zeros(D, F32) if kind == "grid" else (rng.standard_normal(D) * 0.1).astype(F32))
        fields.update(stat_in_blocks=22, stat_in_stride=M, ln_dim=2730)
    tiles = D // 256
    elems, xi, arrays["x_init"] = _stream(x0, D, xb, 2 * D + 64)
    ci, si = R.x_index(M, D, D, 0), R.stat_index(M, tiles, M)
    raw = gemm_call(fields, arrays, {"x": (F32, elems), "o0": (np.uint16, M * D + 2 * D + 64), "stat": (F32, 2 * tiles * M + 64)})
    for name, index, fill in (("x", xi, FILL32), ("o0", ci, FILL16), ("stat", si, FILL32)):
        _guards_hold(raw, name, index, fill)
    x, copy = raw["x"][xi], raw["o0"][ci]
    assert np.isfinite(x).all()
    if kind == "grid":          # what the grid bound assumes, of the rows the launch returned
        assert np.array_equal(x, target), "A = 0 and bias 0: the producer must return x_init"
        assert L.grid_preconditions(x, scale, gamma, f16) == (True, True)
        assert np.array_equal(L.from16(copy, f16), x.astype(np.float64) * gamma.astype(np.float64)[None, :]), "the 16-bit copy is not gamma x"
        xt = x.astype(np.float64).reshape(M, tiles, 256)
        sums = np.stack([xt.sum(2), (xt * xt).sum(2)], -1).reshape(M, -1)
        assert np.array_equal(raw["stat"][si].astype(np.float64), sums), "sums that are exact in any order differ from the rows' sums"
    return dict(x=x, copy=copy, stat=raw["stat"], gamma=gamma, beta=beta, dx=None)


def _swiglu_weight(f16, seed, D=1024, live=2730, HK=2752):
    """EVA02-L's fc1: [gate 32 | value 32] rows per 32 hidden units, the units past `live` zero rows with zero bias"""
    rng = np.random.default_rng(seed)
    w32 = (rng.standard_normal((2 * HK, D)) * 0.02).astype(F32)
    unit = (np.arange(2 * HK) // 64) * 32 + np.arange(2 * HK) % 32
    gate = (np.arange(2 * HK) % 64) < 32
    b = (rng.standard_normal(2 * HK) * 0.1 + np.where(gate, 1.0, 0.5)).astype(F32)         # hidden rows of mean ~ 0.4, sigma ~ 0.6
    w32[unit >= live], b[unit >= live] = 0.0, 0.0
    return w32, b


def _layout(geom, epi, N, f16, seed):
    """the consumer's own arguments: (fields, arrays, output spec {name: (dtype, elements, index)}, what gemm_epi_ref.reference reads)"""
    rng = np.random.default_rng(seed)
    fields, arrays, spec, v = {}, {}, {}, dict(gelu_tanh=0, star_kind=0, star_scale=0.9, star_bias=-0.45, qscale=1.0, tokens=0)
    guard = 2 * N + 64
    if epi in (R.QK, R.QK_ROPE, R.VT):
        hd = 32 if geom == "ccip" else 64
        dim = N if epi == R.VT else (N // 2 if geom == "ccip" else N // 3)
        qs = (0.17677669529663687 if hd == 32 else 0.125) * LOG2E if epi != R.VT else 1.0
        fields.update(tokens=TOKENS, tokens_pad=TOKENS_PAD, dim=dim, heads=dim // hd, hd_log2=5 if hd == 32 else 6, qscale=qs)
        v.update(tokens=TOKENS, dim=dim, qscale=qs)
        index = R.vt_index if epi == R.VT else R.qk_index
        for i in range(N // dim):
            spec["o%d" % i] = (np.uint16, 2 * TOKENS_PAD * dim + 4096, index(M, dim, TOKENS, TOKENS_PAD, dim // hd, hd))
        if epi == R.QK_ROPE:
            ang = rng.uniform(-np.pi, np.pi, (ROPE_TOKENS, 32))
            arrays["rope"] = np.stack([np.sin(ang), np.cos(ang)], -1).astype(F32)
            fields["rope_tokens"] = ROPE_TOKENS
            v.update(rope=arrays["rope"], rope_tokens=ROPE_TOKENS)
    elif epi in (R.GELU, R.STAR):
        spec["o0"] = (np.uint16, M * N + guard, R.x_index(M, N, N, 0))
        fields["gelu_tanh"] = v["gelu_tanh"] = 1              # the ViT's fc1
        fields.update(star_kind=0, star_scale=0.9, star_bias=-0.45)
    elif epi == R.SWIGLU:
        cols, tiles = N // 2, (N + 255) // 256
        arrays["ln_gamma"] = rng.uniform(0.5, 1.5, cols).astype(F32)
        fields.update(ld_out=cols, stat_stride=M)
        spec["o0"] = (np.uint16, M * cols + guard, R.x_index(M, cols, cols, 0))
        spec["stat"] = (F32, 2 * tiles * M + 64, R.stat_index(M, tiles, M))
        v.update(ln_gamma=arrays["ln_gamma"], want_stat=True)
    else:                       # EPI_RESID_ROWSTAT (the forward's last residual launch: rows left row-major) / EPI_RESID_XGI
        v["x0"] = rng.standard_normal((M, N)).astype(F32)
        elems, xi, arrays["x_init"] = _stream(v["x0"], N, 1, guard)
        spec["x"] = (F32, elems, xi)
        if epi == R.RESID_ROWSTAT:
            spec["rowmajor"] = (F32, M * N + guard, R.x_index(M, N, N, 0))
        else:
            tiles = (N + 255) // 256
            arrays["ln_gamma"] = rng.uniform(0.5, 1.5, N).astype(F32)
            fields["stat_stride"] = M
            spec["o0"] = (np.uint16, M * N + guard, R.x_index(M, N, N, 0))
            spec["stat"] = (F32, 2 * tiles * M + 64, R.stat_index(M, tiles, M))
    return fields, arrays, spec, v


@functools.lru_cache(maxsize=None)
def _consumer_operands(wid, f16, kind, N=None, swiglu_full=False):
    """(W patterns, W float64, b, u, c): the consumer's weight and what hiptsdbg_fold_ln makes of it for the producer's norm"""
    _, geom, (pepi, _, _), (epi, _, _, n), _ = WIRING[wid]
    g = L.GEOMETRY[geom]
    N = N or n
    src = hidden(f16, kind) if geom == "eva_fc2" else produced(geom, f16, kind, pepi)
    seed = _seed(geom, f16, kind) + 100 * (1 + [w[0] for w in L.WIRINGS].index(wid))
    if swiglu_full:
        w32, b = _swiglu_weight(f16, seed)
    else:
        w32 = L.weight(N, g["D"], f16, seed)[0]
        w32[:, g["ln_dim"]:] = 0.0                                            # the pad columns of EVA02's fc2 are zero
        b = L.vectors(kind, g["ln_dim"], N, seed + 1, g["beta"])[2]
    wbits, w64 = L.to16(w32, f16)
    u, c = fold_ln(wbits, f16, src["gamma"], src["beta"], b, N, g["D"])
    assert (u[N:].view(np.uint32) == FILL32).all() and (c[N:].view(np.uint32) == FILL32).all()
    if not g["beta"]:
        assert b is None and (c[:N] == 0).all()
    return wbits, w64, b, u[:N].copy(), c[:N].copy()


@functools.lru_cache(maxsize=None)
def hidden(f16, kind):
    """the rows EVA02's inner LayerNorm normalises, as fc2 receives them: the 16-bit copy [M][2752] and the 22 pairs.
    generic: launch 2 of the three-launch chain (EPI_SWIGLU on what RESID_XG wrote); x: the rows read back from its copy, dx: e16 |x|.
    grid: the exact copy and the exact pairs of 2730-wide grid rows."""
    g = L.GEOMETRY["eva_fc2"]
    D, live, seed = g["D"], g["ln_dim"], _seed("eva_fc2", f16, kind)
    gamma, beta = np.zeros(D, F32), np.zeros(D, F32)
    gamma[:live], beta[:live], _ = L.vectors(kind, live, 1, seed + 1)
    if kind == "grid":
        x = np.zeros((M, D), F32)
        x[:, :live], scale = L.rows("grid", live, f16, seed, g["m_max"])
        assert L.grid_preconditions(x, scale, gamma, f16) == (True, True)
        part = L.tile_sums32(x, g["tile"])                                   # [22][M][2]
        xt = np.pad(x.astype(np.float64), ((0, 0), (0, 22 * g["tile"] - D))).reshape(M, 22, g["tile"])
        assert np.array_equal(part.astype(np.float64), np.stack([xt.sum(2), (xt * xt).sum(2)], -1).transpose(1, 0, 2))
        return dict(x=x.astype(np.float64), copy=L.to16(x * gamma[None, :], f16)[0], stat=part.ravel(), gamma=gamma, beta=beta, dx=None)
    wid = "eva-xg-swiglu"
    src = produced("eva", f16, kind, R.RESID_XG)
    wbits, w64, b, u, c = _consumer_operands(wid, f16, kind, 2 * D, True)
    fields, arrays, spec, v = _layout("eva", R.SWIGLU, 2 * D, f16, seed + 7)
    arrays["ln_gamma"] = v["ln_gamma"] = gamma
    fields.update(epi=R.SWIGLU, M=M, N=2 * D, K=1024, f16=f16, shared_chip=0, ln_eps=EPS, qscale=1.0, hd_log2=6, stat_in_blocks=4, stat_in_stride=M, ln_dim=1024)
    arrays.update(a=src["copy"], w=wbits, bias=c, col_u=u, stat_in=src["stat"])
    raw = gemm_call(fields, arrays, {k: s[:2] for k, s in spec.items()})
    for name, (dtype, elems, index) in spec.items():
        _guards_hold(raw, name, index, FILL32 if dtype == F32 else FILL16)
    zq, _ = L.reference_z(src["x"], L.from16(src["copy"], f16), w64, src["gamma"], src["beta"], b, kind, 4, f16)
    pq = R.reference(R.SWIGLU, None, None, dict(v, M=M, N=2 * D, K=1024, z=zq, want_stat=False))["o0"]
    copy = raw["o0"][spec["o0"][2]]
    assert (pq.val[:, live:] == 0).all() and (L.from16(copy, f16)[:, live:] == 0).all(), "hidden units past 2730 must be 0"
    r2 = L.ratio(L.from16(copy, f16), pq.val, pq.bound(1024, "f16" if f16 else "bf16"))
    # the rows fc2's LayerNorm is to see are the ones the device wrote: read back from the copy, held to dx = e16 |x| (rows_of_copy), and
    # the 22 pairs launch 2 returned are those rows' sums over 128 hidden units each, the 22 zero pad units of the last tile included
    x, dx = L.rows_of_copy(copy, gamma, f16, live)
    sums, sb = L.pair_bound(x, dx, g["tile"])
    pairs = raw["stat"][R.stat_index(M, 22, M)].astype(np.float64).reshape(M, 22, 2).transpose(1, 0, 2)
    rs = L.ratio(pairs, sums, sb)
    print("launch 2: copy error / bound %.3f, pairs against the sums of the rows it wrote: error / bound %.3f" % (r2.max(), rs.max()))
    assert r2.max() <= 1.0, "launch 2 (EPI_SWIGLU at 2 x 2752 columns) misses its own bound"
    assert rs.max() <= 1.0, "the 22 pairs are not the sums of the rows the copy holds"
    return dict(x=x, copy=copy, stat=raw["stat"], gamma=gamma, beta=beta, dx=dx)


# ---- call 2: the consumers -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def consumed(wid, f16, kind, tamper=None, fold=True):
    """One consumer launch on what the producer wrote and its float64 reference: {output name: (got float64 [M][cols], Q)}.
    tamper: a negative control -- 'ln_dim' (the padded width), 'shift' (the pairs' rows moved by one), 'drop' (one tile's pair less).
    fold = False: the separate path -- hiptsdbg_row_ln writes the 16-bit operand from the same x, the consumer runs without the fold."""
    _, geom, (pepi, _, _), (epi, feat, xb, N), how = WIRING[wid]
    g = L.GEOMETRY[geom]
    D, ln_dim, blocks = g["D"], g["ln_dim"], L.blocks_of(geom)
    src = hidden(f16, kind) if geom == "eva_fc2" else produced(geom, f16, kind, pepi)
    wbits, w64, b, u, c = _consumer_operands(wid, f16, kind)
    fields, arrays, spec, v = _layout(geom, epi, N, f16, _seed(geom, f16, kind) + 7)
    fields.update(epi=epi, M=M, N=N, K=D, f16=f16, shared_chip=0, ln_eps=EPS, x_blocked=xb, sk_ws=int(bool(feat & R.SK_WS)))
    fields.setdefault("qscale", 1.0)
    fields.setdefault("hd_log2", 6)
    x64 = src["x"].astype(np.float64)
    fmt = "f16" if f16 else "bf16"
    if fold:
        stat = np.array(src["stat"], F32)                                    # the buffer as copied back, guard elements included
        if tamper == "shift":
            pairs = stat[:2 * blocks * M].reshape(blocks, M, 2)
            pairs[:] = np.roll(pairs, 1, axis=1)
        nb = blocks - 1 if tamper == "drop" else blocks
        width = blocks * g["tile"] if tamper == "ln_dim" else ln_dim
        arrays.update(a=src["copy"], w=wbits, bias=c, col_u=u)
        if how == "stat_in":
            arrays["stat_in"] = stat
            fields.update(stat_in_blocks=nb, stat_in_stride=M, ln_dim=width)
        else:               # eva.hip: launch_rowstat(stat_p, rowstat_p, M, M, sblocks, mlp_hidden, eps)
            rs = rowstat(stat, M, M, nb, width, EPS)
            assert (rs[M:].view(np.uint32) == FILL32).all()
            arrays["rowstat"] = rs[:M].copy()
        zq, st = L.reference_z(x64, L.from16(src["copy"], f16), w64, src["gamma"], src["beta"], b, kind, blocks, f16, ln_dim=ln_dim)
        if src["dx"] is not None:
            zq.extra = zq.extra + L.perturbation_bound(src["dx"], x64, zq.val, L.fold_vectors64(w64, src["gamma"], src["beta"], b)[1][None, :], w64,
                                                       src["gamma"], st, ln_dim)
    else:
        beta = src["beta"]
        st_, _, xn = TR.launch_row_ln(TR.variant("opt16_beta" if beta is not None else "opt16_nobeta"), f16, src["x"], src["gamma"], beta, EPS)
        _ok(st_, "hiptsdbg_row_ln")
        xn = xn[:M * D].reshape(M, D)
        arrays.update(a=xn, w=wbits, bias=b)
        # its own bound: the row kernel's float32 LayerNorm and 16-bit rounding per element, carried through |W|, and the MFMA sum
        lnq = R.layernorm_of_stored(src["x"], src["gamma"], beta, EPS)
        zv = lnq.val @ w64.T + (b.astype(np.float64)[None, :] if b is not None else 0.0)
        zq = R.Q(zv, np.abs(zv), 2, (D + 16) * R.U * (np.abs(L.from16(xn, f16)) @ np.abs(w64).T) + lnq.bound(0, fmt) @ np.abs(w64).T)
    raw = gemm_call(fields, arrays, {k: s[:2] for k, s in spec.items()})
    for name, (dtype, elems, index) in spec.items():
        if name == "x" and "rowmajor" in spec:
            assert np.array_equal(raw["x"].view(np.uint32), arrays["x_init"].view(np.uint32)), "the blocked stream changed although rows go row-major"
            continue
        _guards_hold(raw, name, index, FILL32 if dtype == F32 else FILL16)
    want = R.reference(epi, None, None, dict(v, M=M, N=N, K=D, z=zq))
    out = {}
    for name, q in want.items():
        got = raw["rowmajor" if name == "x" and "rowmajor" in spec else name][spec["rowmajor" if name == "x" and "rowmajor" in spec else name][2]]
        is16 = got.dtype == np.uint16
        out[name] = (L.from16(got, f16).reshape(got.shape) if is16 else got.astype(np.float64), q, q.bound(D, fmt if is16 else None))
    return out


def _worst(out, kind):
    """(largest error / bound over every output, the same per regime, every output finite)"""
    reg = L.regime_of_row(kind)
    names = [r[0] for r in L.regimes(kind)]
    per = dict.fromkeys(names, 0.0)
    finite = True
    for name, (got, q, bound) in out.items():
        finite = finite and bool(np.isfinite(got).all())
        r = L.ratio(got, q.val, bound)
        for i, n in enumerate(names):
            per[n] = max(per[n], float(r[reg == i].max()))
    return max(per.values()), per, finite


CHAIN = [pytest.param(w[0], f16, kind, id="%s-%s-%s" % (w[0], "f16" if f16 else "bf16", kind)) for w in L.WIRINGS for f16 in (1, 0) for kind in ("grid", "generic")]


@pytest.mark.parametrize("wid,f16,kind", CHAIN)
def test_chain(wid, f16, kind):
    E._default_environment()
    worst, per, finite = _worst(consumed(wid, f16, kind), kind)
    print("error / bound per regime:", {k: round(x, 4) for k, x in per.items()})
    assert finite, "a consumer output is not finite"
    assert worst <= 1.0, per


CONTROLS = [pytest.param(wid, f16, id="%s-%s" % (wid, "f16" if f16 else "bf16")) for wid in ("vit-xg-gelu", "eva-swiglu-rowstat", "eva-swiglu-xgi-kernel", "ccip-xg-star")
            for f16 in (1, 0)]


@pytest.mark.parametrize("wid,f16", CONTROLS)
def test_chain_negative_controls(wid, f16):
    """the bound notices a consumer that reads the producer's statistics wrongly: each control misses it on at least one element"""
    geom = WIRING[wid][1]
    g = L.GEOMETRY[geom]
    assert _worst(consumed(wid, f16, "grid"), "grid")[0] <= 1.0
    tampers = ["shift", "drop"] + (["ln_dim"] if L.blocks_of(geom) * g["tile"] != g["ln_dim"] else [])
    seen = {t: _worst(consumed(wid, f16, "grid", t), "grid")[0] for t in tampers}
    print("worst error / bound of the controls:", {k: round(x, 1) for k, x in seen.items()})
    assert all(x > 1.0 for x in seen.values()), seen
    assert geom != "eva_fc2" or "ln_dim" in seen


# every wiring whose rows a launch returns in float32 and row_ln_kernel takes (at most 1024 columns): all but fc2's, whose 2730-wide hidden
# rows exist only as the 16-bit copy
RECORDED = ["vit-xg-qkv", "vit-xg-gelu", "eva-xg-qkrope", "eva-xgi-qkrope", "eva-xg-swiglu", "ccip-xg-star", "ccip-xg-qk", "ccip-xg-vt"]


@pytest.mark.parametrize("f16", [1, 0], ids=["f16", "bf16"])
def test_record_folded_against_separate(f16):
    """The table of DESIGN.md ("The folded LayerNorm: what it computes, how accurate it is, and where"): max |err| / rms(want) per regime on the generic inputs, the folded
    chain beside the separate path on the same x.  No threshold on the folded figures -- they are the record; the separate path is held to
    its own bound."""
    reg = L.regime_of_row("generic")
    names = [r[0] for r in L.regimes("generic")]
    print("\n%-16s %-5s %-13s %-11s %-11s" % ("wiring", "type", "regime", "folded", "separate"))
    for wid in RECORDED:
        fo, se = consumed(wid, f16, "generic"), consumed(wid, f16, "generic", None, False)
        assert _worst(se, "generic")[0] <= 1.0, (wid, _worst(se, "generic")[1])
        keys = [k for k in fo if k != "stat"]
        want = np.hstack([fo[k][1].val for k in keys])
        got_f, got_s = np.hstack([fo[k][0] for k in keys]), np.hstack([se[k][0] for k in keys])
        for i, n in enumerate(names):
            rms = np.sqrt((want[reg == i] ** 2).mean()) or 1.0                # want == 0 (a zero row without beta): the absolute error
            ef, es = np.abs(got_f - want)[reg == i].max(), np.abs(got_s - want)[reg == i].max()
            print("%-16s %-5s %-13s %-11.2e %-11.2e" % (wid, "f16" if f16 else "bf16", n, ef / rms, es / rms))
