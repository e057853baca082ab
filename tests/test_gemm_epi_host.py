"""CPU: the tables of tests/gemm_epi_ref.py.  Every GEMM arm -- (epilogue, main loop, tile height, interior, operand type, ragged M, ragged
N, persistent grid, blocked stream, features) -- that a launch_gemm call of the five forwards reaches at any batch from 1 to the model's
largest reference batch (256 CUs, default environment) has a case in CASES, every case's plan is the arm it claims, and the float64
references agree with definitions that do not come from the kernel's header: torch's activations, float64 LayerNorm -> Linear,
oracle/eva.py's rotation, numpy reshapes of the layouts."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gemm_epi_ref as R  # noqa: E402


@pytest.mark.parametrize("model", sorted(R.MODELS))
def test_reachable_arms_are_covered(model):
    switches = [k for k in os.environ if k.startswith(("HIPTS_GEMM", "HIPTS_EPI_", "HIPTS_RESID_GENERAL")) and k != "HIPTS_GEMM_Q4"]
    assert switches == [], "the tables are for the default environment"
    covered = {R.case_key(c) for c in R.CASES}
    reach = R.reachable(model)
    missing = {k: b for k, b in reach.items() if k not in covered}
    print("%s: %d reachable arms" % (model, len(reach)))
    assert not missing, "\n".join("%s reached at batches %s" % (R.key_name(k), b) for k, b in sorted(missing.items()))


def test_each_case_reaches_the_arm_it_claims():
    keys = [R.case_key(c) for c in R.CASES]
    assert len(set(keys)) == len(keys), "one row per arm"
    for case in R.CASES:
        epi, f16, M, N, shared, feat, xb, _ = case
        for K in R.case_ks(case):
            p = R.plan(epi, M, N, K, f16, shared, feat, 0, R.case_dim(epi, N))
            assert R.arm_key(epi, f16, M, N, feat, xb, p) == R.case_key(case), (case, R.key_name(R.arm_key(epi, f16, M, N, feat, xb, p)))
    for case in R.k64_cases():
        epi, f16, M, N, shared, feat, xb, _ = case
        assert R.arm_key(epi, f16, M, N, feat, xb, R.plan(epi, M, N, 64, f16, shared, feat, 0, R.case_dim(epi, N))) == R.case_key(case)
    assert sorted({c[7][0] for c in R.k64_cases()}) == sorted({c[7][0] for c in R.CASES})


def test_bf16_general_and_ragged_arm_per_epilogue():
    for epi in range(16):
        mine = [R.case_key(c) for c in R.CASES if c[0] == epi and c[1] == 0]
        assert any(k[1:4] == (R.PP, 8, 0) and k[7] == 1 for k in mine), R.EPI_NAMES[epi]      # general 256-row persistent arm
        assert any(k[5] == 1 and k[6] == 1 for k in mine), R.EPI_NAMES[epi]                     # ragged rows and columns


def test_launch_table_names_every_call_site():
    """The number of launch_gemm( / gemm( call expressions inside each forward's kernel sequence equals the length of CALL_SITES for it;
    every listed site has rows in LAUNCHES, and every row belongs to a listed site."""
    import re
    csrc = os.path.join(ROOT, "anime-illust-image-searcher_amd", "csrc")
    ends = {"vit_run_images": "int vit_forward_impl(", "eva_run_images": "int eva_forward_impl(", "ccip_run_images": "int ccip_forward_impl(",
            "cnx_run_images": "int cnx_forward_impl(", "sw_run_images": "int sw_forward_impl("}
    for where, sites in R.CALL_SITES.items():
        f, fn = where.split(":")
        text = open(os.path.join(csrc, f)).read()
        body = re.sub(r"//[^\n]*", "", text[text.index("int %s(" % fn):text.index(ends[fn])])
        calls = re.findall(r"(?<![A-Za-z_])(?:launch_gemm|gemm)\(", body)
        assert len(calls) == len(sites), "%s has %d launch calls, CALL_SITES lists %d" % (where, len(calls), len(sites))
        labels = {row[1][len(where) + 1:] for row in R.LAUNCHES if row[1].startswith(where + " ")}
        starts = [w for s in sites if s for w in s.split(";")]
        for w in starts:
            assert any(l.startswith(w) for l in labels), "%s: no LAUNCHES row for call site %r" % (where, w)
        for l in labels:
            assert any(l.startswith(w) for w in starts), "%s: row %r belongs to no listed call site" % (where, l)
    assert {row[1].split(" ")[0] for row in R.LAUNCHES} == set(R.CALL_SITES)


# ---- the references against independent definitions --------------------------------------------------------------------------
def _inputs(M, N, K, seed=0):
    rng = np.random.default_rng(seed)
    a, w = rng.standard_normal((M, K)), rng.standard_normal((N, K)) * 0.05
    return rng, a, w


def _v(M, N, K, **kw):
    v = dict(M=M, N=N, K=K, bias=np.zeros(N, np.float32), qscale=1.0, ln_eps=1e-6, gelu_tanh=0, star_kind=0, star_scale=1.0, star_bias=0.0)
    v.update(kw)
    return v


@pytest.mark.parametrize("stats", ["rowstat", "stat_in"])
def test_folded_forms_equal_layernorm_then_linear(stats):
    """rstd (W (gamma x)) - rstd mean (W gamma) + (W beta + b) == W LN(x) + b in float64, for every epilogue that takes the fold"""
    M, N, D = 37, 192, 96
    rng = np.random.default_rng(1)
    x = rng.standard_normal((M, D)) * 1.7 + 0.4
    gamma, beta, b = rng.uniform(0.5, 1.5, D), rng.standard_normal(D) * 0.1, rng.standard_normal(N) * 0.1
    W = rng.standard_normal((N, D)) * 0.05
    eps = 1e-6
    mean, var = x.mean(1, keepdims=True), x.var(1, keepdims=True)
    want = ((x - mean) / np.sqrt(var + eps) * gamma + beta) @ W.T + b
    acc = (x * gamma) @ W.T
    v = _v(M, N, D, bias=(W @ beta + b), col_u=W @ gamma, ln_eps=eps, ln_dim=D)
    if stats == "rowstat":
        rstd = 1.0 / np.sqrt(var + eps)
        v["rowstat"] = np.concatenate([rstd, rstd * mean], 1)
    else:       # three partial (sum, sum of squares) pairs per row
        parts = np.zeros((3, M + 5, 2))
        for i in range(3):
            blk = x[:, 32 * i:32 * i + 32]
            parts[i, :M, 0], parts[i, :M, 1] = blk.sum(1), (blk * blk).sum(1)
        v["stat_in"] = parts
    z = R.linear(R.Q(acc, np.abs(acc), D), v)
    np.testing.assert_allclose(z.val, want, rtol=0, atol=1e-10)
    np.testing.assert_allclose(R.reference(R.VT, acc, np.abs(acc), v)["o0"].val, want, rtol=0, atol=1e-10)
    x0 = rng.standard_normal((M, N))
    for epi in (R.RESID_ROWSTAT, R.RESID_XGI):
        np.testing.assert_allclose(R.reference(epi, acc, np.abs(acc), dict(v, x0=x0))["x"].val, x0 + want, rtol=0, atol=1e-10)
    import torch
    got = R.reference(R.GELU, acc, np.abs(acc), dict(v, gelu_tanh=1))["o0"].val
    np.testing.assert_allclose(got, torch.nn.functional.gelu(torch.from_numpy(want), approximate="tanh").numpy(), rtol=0, atol=1e-10)


def test_activations_equal_torch():
    import torch
    import torch.nn.functional as F
    M, N, K = 23, 128, 64
    rng, a, w = _inputs(M, N, K)
    acc = (a @ w.T) * 6.0
    bias = rng.standard_normal(N) * 0.3
    z = torch.from_numpy(acc + bias)
    mag = np.abs(acc)
    for tanh_form in (0, 1):
        got = R.reference(R.GELU, acc, mag, _v(M, N, K, bias=bias, gelu_tanh=tanh_form))["o0"].val
        np.testing.assert_allclose(got, F.gelu(z, approximate="tanh" if tanh_form else "none").numpy(), rtol=0, atol=1e-12)
    got = R.reference(R.STAR, acc, mag, _v(M, N, K, bias=bias, star_scale=0.9, star_bias=-0.45))["o0"].val
    np.testing.assert_allclose(got, (0.9 * torch.relu(z) ** 2 - 0.45).numpy(), rtol=0, atol=1e-12)          # MetaFormer's StarReLU
    got = R.reference(R.STAR, acc, mag, _v(M, N, K, bias=bias, star_kind=1))["o0"].val
    np.testing.assert_allclose(got, F.silu(z).numpy(), rtol=0, atol=1e-12)
    head = R.reference(R.HEAD, acc, mag, _v(M, N, K, bias=bias))
    np.testing.assert_allclose(head["x"].val, z.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(head["probs"].val, torch.sigmoid(z).numpy(), rtol=0, atol=1e-12)
    # SwiGLU: W rows interleaved per 32 hidden units [gate 0..31 | value 0..31]
    units = N // 2
    gate_w, val_w = rng.standard_normal((units, K)) * 0.3, rng.standard_normal((units, K)) * 0.3
    gb, vb, gamma = rng.standard_normal(units) * 0.1, rng.standard_normal(units) * 0.1, rng.uniform(0.5, 1.5, units)
    wi, bi = np.zeros((N, K)), np.zeros(N)
    for u in range(units):
        wi[(u // 32) * 64 + u % 32], wi[(u // 32) * 64 + 32 + u % 32] = gate_w[u], val_w[u]
        bi[(u // 32) * 64 + u % 32], bi[(u // 32) * 64 + 32 + u % 32] = gb[u], vb[u]
    acc2 = a @ wi.T
    ref = R.reference(R.SWIGLU, acc2, np.abs(acc2), _v(M, N, K, bias=bi, ln_gamma=gamma, want_stat=True))
    p = F.silu(torch.from_numpy(a @ gate_w.T + gb)).numpy() * (a @ val_w.T + vb)
    np.testing.assert_allclose(ref["o0"].val, p * gamma, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref["stat"].val, np.stack([p.sum(1), (p * p).sum(1)], -1), rtol=0, atol=1e-10)        # one 256-column tile


def test_residual_forms():
    M, N, K = 19, 64, 64
    rng, a, w = _inputs(M, N, K, 3)
    acc, mag = a @ w.T, np.abs(a) @ np.abs(w).T
    bias, rs, x0 = rng.standard_normal(N), rng.uniform(0.8, 1.2, N), rng.standard_normal((M, N))
    pos = rng.standard_normal((5, N))
    lin = acc + bias
    v = _v(M, N, K, bias=bias, x0=x0)
    np.testing.assert_allclose(R.reference(R.RESID, acc, mag, v)["x"].val, x0 + lin, atol=1e-12)
    np.testing.assert_allclose(R.reference(R.BIAS, acc, mag, v)["x"].val, lin, atol=1e-12)
    np.testing.assert_allclose(R.reference(R.RESID_XG, acc, mag, v)["x"].val, x0 + lin, atol=1e-12)
    vs = dict(v, res_scale=rs)
    for epi in (R.RESCALE, R.RESID_LN, R.RESID_XG):
        np.testing.assert_allclose(R.reference(epi, acc, mag, vs)["x"].val, x0 * rs + lin, atol=1e-12)
    np.testing.assert_allclose(R.reference(R.RESID_LS, acc, mag, vs)["x"].val, x0 + rs * lin, atol=1e-12)
    vp = dict(v, pos=pos, tokens=5, qscale=0.25)
    want = acc * 0.25 + bias + pos[np.arange(M) % 5]
    np.testing.assert_allclose(R.reference(R.PATCH, acc, mag, vp)["x"].val, want, atol=1e-12)
    np.testing.assert_allclose(R.reference(R.RESID_XG, acc, mag, vp)["x"].val, want, atol=1e-12)
    # the bound is the formula on magnitudes: it dominates the value and grows with every term
    q = R.reference(R.RESCALE, acc, mag, vs)["x"]
    assert (q.mag >= np.abs(q.val) - 1e-12).all() and (q.bound(K) > 0).all()
    np.testing.assert_allclose(q.mag, np.abs(x0) * rs + mag + np.abs(bias), atol=1e-12)
    # LayerNorm of the stored rows
    import torch
    xs = (x0 * 1.3 + 0.2).astype(np.float32)
    g = rng.uniform(0.5, 1.5, N).astype(np.float32)
    want = torch.nn.functional.layer_norm(torch.from_numpy(xs.astype(np.float64)), (N,), torch.from_numpy(g.astype(np.float64)), None, 1e-6).numpy()
    np.testing.assert_allclose(R.layernorm_of_stored(xs, g, None, 1e-6).val, want, atol=1e-12)


def test_rope_equals_the_oracle_rotation():
    import torch
    from oracle import eva
    grid, heads, hd = 3, 2, 64
    npatch, dim = grid * grid, heads * hd
    TS = 16                                                     # class token + 9 patch tokens, rows padded to 16 per image
    M, N, K = 2 * TS, 3 * dim, 64
    rng, a, w = _inputs(M, N, K, 5)
    acc = a @ w.T
    bias = rng.standard_normal(N) * 0.1
    sin, cos = eva.rope_tables(grid, hd)                        # [tokens][64], each band twice
    table = np.stack([sin.numpy()[:, ::2], cos.numpy()[:, ::2]], -1).astype(np.float32)        # rope[t - 1][i] = (sin, cos) of column pair i
    ref = R.reference(R.QK_ROPE, acc, np.abs(acc), _v(M, N, K, bias=bias, dim=dim, tokens=TS, rope=table, rope_tokens=npatch, qscale=0.5))
    z = torch.from_numpy(acc + bias).reshape(2, TS, 3, heads, hd)
    for i, (name, scale) in enumerate((("o0", 0.5), ("o1", 1.0), ("o2", 1.0))):
        t = z[:, :, i].transpose(1, 2)                          # [image][head][token][d] as oracle/eva.py holds q and k
        if i < 2:
            body = t[:, :, 1:1 + npatch]
            t = torch.cat([t[:, :, :1], body * cos.double() + eva._rot(body) * sin.double(), t[:, :, 1 + npatch:]], dim=2)
        want = (t * scale).transpose(1, 2).reshape(M, dim).numpy()
        np.testing.assert_allclose(ref[name].val, want, rtol=0, atol=1e-6)       # the table is float32


def test_layout_indices_equal_reshapes():
    images, tokens, tokens_pad, heads, hd = 3, 10, 16, 4, 32
    M, dim = images * tokens, heads * hd
    z = np.arange(M * dim, dtype=np.int64).reshape(M, dim)
    buf = np.full(images * heads * tokens_pad * hd, -1, np.int64)
    buf[R.qk_index(M, dim, tokens, tokens_pad, heads, hd)] = z
    want = np.full((images, heads, tokens_pad, hd), -1, np.int64)
    want[:, :, :tokens] = z.reshape(images, tokens, heads, hd).transpose(0, 2, 1, 3)       # the attention tests' [image][head][token][d]
    assert np.array_equal(buf.reshape(want.shape), want)
    buf[:] = -1
    buf[R.vt_index(M, dim, tokens, tokens_pad, heads, hd)] = z
    want = np.full((images, heads, hd, tokens_pad), -1, np.int64)
    want[:, :, :, :tokens] = z.reshape(images, tokens, heads, hd).transpose(0, 2, 3, 1)
    assert np.array_equal(buf.reshape(want.shape), want)
    Mb, ld = 48, 64
    zb = np.arange(Mb * ld, dtype=np.int64).reshape(Mb, ld)
    buf = np.zeros(Mb * ld, np.int64)
    buf[R.x_index(Mb, ld, ld, 1)] = zb
    assert np.array_equal(buf.reshape(Mb // 16, ld // 16, 16, 16), zb.reshape(Mb // 16, 16, ld // 16, 16).transpose(0, 2, 1, 3))
    assert np.array_equal(R.x_index(5, 7, 9, 0), np.arange(5)[:, None] * 9 + np.arange(7)[None, :])
