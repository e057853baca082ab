"""CPU: the restatements of tests/tokens_ref.py against independent definitions -- swinv2_ref's patch merging, torch's conv2d, the oracle
EVA02 and ViT graphs -- in float64, the properties that make the exact-answer inputs of tests/test_gpu_tokens.py exact, and the mutants:
for every pooling case the GPU test runs, a pool that drops, doubles or misplaces ONE token, reads a row it must not read, leaves an empty
split's partial row unwritten or leaves the lo half out moves at least one element of the expected buffers by more than that case's bound
(zero for the bit-for-bit cases, the E32 bound for the float64 ones).  That is the evidence that the GPU cases can see such a kernel."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rows_ref as R  # noqa: E402
import swinv2_ref  # noqa: E402
import tokens_ref as T  # noqa: E402
from oracle import eva as oracle_eva  # noqa: E402
from oracle import vit as oracle_vit  # noqa: E402

F32 = np.float32
CSRC = os.path.join(ROOT, "anime-illust-image-searcher_amd", "csrc")


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


# ---- copies and gathers ------------------------------------------------------------------------------------------------------------------------
def test_merge_then_product_is_swinv2_refs_patch_merging():
    """swinv2_ref.features with no blocks: the stream after stage 1 is LN(reduction(merged stage-0 stream)).  merge_rows of the stage-0
    stream, the product and the LayerNorm reproduce it; the (dy, dx) column order does not."""
    rng = np.random.default_rng(1)
    cfg = dict(image_size=16, patch=4, window=2, dims=[8, 16, 32, 64], heads=[1, 1, 1, 1], depths=[0, 0, 0, 0], ln_eps=1e-5)
    w = {"patch_embed.proj.weight": rng.standard_normal((8, 3, 4, 4)), "patch_embed.proj.bias": rng.standard_normal(8),
         "patch_embed.norm.weight": rng.standard_normal(8), "patch_embed.norm.bias": rng.standard_normal(8),
         "layers.1.downsample.reduction.weight": rng.standard_normal((16, 32)), "layers.1.downsample.norm.weight": rng.standard_normal(16),
         "layers.1.downsample.norm.bias": rng.standard_normal(16)}
    w = {k: t64(v) for k, v in w.items()}
    img = t64(rng.standard_normal((2, 3, 16, 16)))
    x0 = swinv2_ref.features(w, img, cfg, stop_stage=0).numpy()                   # [2][4 * 4][8]
    want = swinv2_ref.features(w, img, cfg, stop_stage=1).numpy().reshape(8, 16)
    red, g, b = (w["layers.1.downsample." + k].numpy() for k in ("reduction.weight", "norm.weight", "norm.bias"))
    got = R.layernorm64(T.merge_rows(x0.reshape(2, 4, 4, 8)) @ red.T, g, b, 1e-5)
    assert np.max(np.abs(got - want)) < 1e-12
    swapped = R.layernorm64(T.merge_rows(x0.reshape(2, 4, 4, 8), swap=True) @ red.T, g, b, 1e-5)
    assert np.max(np.abs(swapped - want)) > 0.1


@pytest.mark.parametrize("batch,H,C", T.MERGE_SHAPES)
def test_merge_cases_see_a_dy_dx_swap(batch, H, C):
    x = T.distinct_f32(batch * H * H * C, H + C).reshape(batch, H, H, C)
    for f16 in (0, 1):
        want, mutant = T.merge_expected(x, f16), T.merge_expected(x, f16, swap=True)
        rows = want[:-T.GUARD // 2].reshape(-1, 8 * C)
        assert np.any(rows[:, :4 * C] != mutant[:-T.GUARD // 2].reshape(-1, 8 * C)[:, :4 * C])
        assert np.all(R.from_op(rows[:, 4 * C:], f16) != 0) and np.unique(rows[:, :4 * C].astype(np.uint32) << 16 | rows[:, 4 * C:]).size == x.size


@pytest.mark.parametrize("batch,H,C", T.IM2COL_SHAPES + [(2, 8, 8)])
def test_im2col_then_product_is_conv2d(batch, H, C):
    rng = np.random.default_rng(H * C)
    x = rng.standard_normal((batch, H, H, C))
    wt = rng.standard_normal((5, C, 3, 3))
    want = F.conv2d(t64(x.transpose(0, 3, 1, 2)), t64(wt), stride=2, padding=1).numpy().transpose(0, 2, 3, 1).reshape(-1, 5)
    cols = T.im2col_rows(x)
    got = cols @ wt.transpose(0, 2, 3, 1).reshape(5, 9 * C).T                        # W2d[n][(3 ky + kx) C + c] = W[n][c][ky][kx]
    assert np.max(np.abs(got - want)) < 1e-12
    # an even H: the windows never reach the padding below and to the right
    assert np.array_equal(cols, T.im2col_rows(x, pad_bottom_right=False))


@pytest.mark.parametrize("batch,H,C", T.IM2COL_SHAPES)
def test_im2col_cases_zero_exactly_the_top_and_left_taps(batch, H, C):
    xn = T.distinct_u16(batch * H * H * C, H + C).reshape(batch, H, H, C)
    Ho = H // 2
    col = T.im2col_rows(xn).reshape(batch, Ho, Ho, 3, 3, C)
    outside = np.zeros(col.shape, bool)
    outside[:, 0, :, 0] = True                  # first output row, ky = 0
    outside[:, :, 0, :, 0] = True               # first output column, kx = 0
    assert np.array_equal(col == 0, outside)
    assert np.unique(col[~outside]).size <= xn.size and set(np.unique(col[~outside])) == set(xn.ravel())      # every input element is somewhere


def test_assemble_is_the_oracles_token_assembly():
    """oracle/eva.py: t = cat([cls, patch rows], 1) + pos_embed, in float32.  The forward adds pos[1 + k] to patch row k in the patch
    GEMM's epilogue, so what the assemble step receives is tmp = row + pos[1 + k]; with the convolution's rows zero that sum is pos itself
    and the oracle's line is the whole arithmetic."""
    rng = np.random.default_rng(2)
    B, n, TS, D = 3, 9, 13, 16
    cls = rng.standard_normal((1, 1, D)).astype(F32)
    pos = rng.standard_normal((1, 1 + n, D)).astype(F32)
    conv = np.zeros((B, n, D), F32)
    want = (torch.cat([torch.from_numpy(cls).expand(B, -1, -1), torch.from_numpy(conv)], dim=1) + torch.from_numpy(pos)).numpy()
    tmp = conv + pos[:, 1:]
    x = T.assemble_rows(tmp, cls[0, 0], pos[0, 0], TS)
    assert x.shape == (B, TS, D) and np.array_equal(x[:, :1 + n].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(x[:, 1 + n:].view(np.uint32), np.zeros((B, TS - 1 - n, D), np.uint32))              # +0
    # the blocked copy holds the same rows at gemm_epi.h::x_off, and nothing else
    row_major, blk = T.assemble_expected(tmp, cls[0, 0], pos[0, 0], TS, 1)
    M = B * TS
    body = blk[:-T.GUARD // 4].reshape((M + 15) // 16, D // 16, 16, 16)
    for m in (0, 1, 15, 16, M - 1):
        assert np.array_equal(body[m // 16, :, m % 16, :].ravel(), row_major[m * D:(m + 1) * D])
    assert np.all(body[M // 16, :, M % 16:, :] == T.FILL32) and M % 16 != 0


def _zero_block(D, hidden, eva):
    """one transformer block that adds nothing to the stream: its two output projections are zero"""
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)          # noqa: E731
    one = torch.ones(D, dtype=torch.float64)
    w = {"norm1.weight": one, "norm1.bias": z(D), "norm2.weight": one, "norm2.bias": z(D), "attn.proj.weight": z(D, D), "attn.proj.bias": z(D),
         "mlp.fc2.weight": z(D, hidden), "mlp.fc2.bias": z(D)}
    if eva:
        w.update({"attn.q_proj.weight": z(D, D), "attn.q_proj.bias": z(D), "attn.k_proj.weight": z(D, D), "attn.v_proj.weight": z(D, D), "attn.v_proj.bias": z(D),
                  "mlp.fc1_g.weight": z(hidden, D), "mlp.fc1_g.bias": z(hidden), "mlp.fc1_x.weight": z(hidden, D), "mlp.fc1_x.bias": z(hidden),
                  "mlp.norm.weight": torch.ones(hidden, dtype=torch.float64), "mlp.norm.bias": z(hidden)})
    else:
        w.update({"attn.qkv.weight": z(3 * D, D), "attn.qkv.bias": z(3 * D), "mlp.fc1.weight": z(hidden, D), "mlp.fc1.bias": z(hidden)})
    return {"blocks.0." + k: v for k, v in w.items()}


def test_eva_colsum_and_pool_are_the_oracles_head():
    """oracle/eva.py with one block that adds nothing, a zero convolution and an identity head: its logits are fc_norm(mean over the patch
    tokens) of cat([cls, 0]) + pos_embed, with a pos_embed per image standing for arbitrary tokens.  The assembled rows, eva_colsum64 and
    rows_ref.pool_ln64 with count = np give the same."""
    rng = np.random.default_rng(3)
    B, grid, D = 2, 3, 16
    n, TS = grid * grid, grid * grid + 4
    cls = rng.standard_normal(D).astype(F32)
    pos = rng.standard_normal((B, 1 + n, D)).astype(F32)
    pos[:, 0] = pos[0, 0]
    g, b = R.stat_affine(D, 4)
    w = _zero_block(D, 8, True)
    w.update({"patch_embed.proj.weight": torch.zeros(D, 3, 1, 1, dtype=torch.float64), "patch_embed.proj.bias": torch.zeros(D, dtype=torch.float64),
              "cls_token": t64(cls).reshape(1, 1, D), "pos_embed": t64(pos), "fc_norm.weight": t64(g), "fc_norm.bias": t64(b),
              "head.weight": torch.eye(D, dtype=torch.float64), "head.bias": torch.zeros(D, dtype=torch.float64)})
    want = oracle_eva.eva_forward(w, t64(rng.standard_normal((B, 3, grid, grid))), patch=1, heads=1, eps=1e-6).numpy()
    x = T.assemble_rows(pos[:, 1:], cls, pos[0, 0], TS)
    x[:, 1 + n:] = 1e30                                         # the pad rows are not pooled, whatever they hold
    got = R.pool_ln64(T.eva_colsum64(x, n), g, b, 1e-6, n)
    assert np.max(np.abs(got - want)) < 1e-12


@pytest.mark.parametrize("pool_then_norm", [0, 1])
def test_vit_pool_forms_are_the_oracles_head(pool_then_norm):
    rng = np.random.default_rng(5)
    B, grid, D = 3, 4, 16
    tokens = rng.standard_normal((B, grid * grid, D)).astype(F32)
    g, b = R.stat_affine(D, 6)
    w = _zero_block(D, 8, False)
    w.update({"patch_embed.proj.weight": torch.zeros(D, 3, 1, 1, dtype=torch.float64), "patch_embed.proj.bias": torch.zeros(D, dtype=torch.float64),
              "pos_embed": t64(tokens), "norm.weight": t64(g), "norm.bias": t64(b), "head.weight": torch.eye(D, dtype=torch.float64),
              "head.bias": torch.zeros(D, dtype=torch.float64)})
    want = oracle_vit.vit_forward(w, t64(rng.standard_normal((B, 3, grid, grid))), patch=1, heads=1, eps=1e-6, pool_then_norm=bool(pool_then_norm)).numpy()
    for splits in (1, 3, 8, 32):                                 # the answer does not depend on the splits
        part, feat = T.vit_pool64(tokens, g, b, 1e-6, pool_then_norm, splits)
        assert part.shape == (B, splits, D) and np.max(np.abs(feat - want)) < 1e-12
        feat32 = T.vit_pool32(tokens, g, b, 1e-6, pool_then_norm, splits)[1]
        assert feat32.dtype == F32 and np.max(np.abs(feat32 - want)) < 1e-4


def test_forward_splits_is_the_forwards_formula_and_its_values_are_cases():
    src = open(os.path.join(CSRC, "vit.hip")).read()
    assert "h->pool_splits = h->tokens >= 64 ? std::min(32, std::max(8, h->tokens / 28)) : 1;" in src
    assert [T.forward_splits(t) for t in (1, 63, 64, 70, 196, 784, 1024)] == [1, 1, 8, 8, 8, 28, 32]
    for tokens in {t for t, _ in T.VIT_POOL_TS}:
        assert (tokens, T.forward_splits(tokens)) in T.VIT_POOL_TS
    assert T.empty_splits(70, 32) == list(range(24, 32)) and all(T.empty_splits(t, s) == [] for t, s in T.VIT_POOL_TS if (t, s) != (70, 32))
    assert re.search(r"constexpr int POOL_SPLITS = %d;" % T.EVA_SPLITS, open(os.path.join(CSRC, "eva.hip")).read())


def test_cast_values_hold_the_edges_of_both_types():
    v = T.cast_values(255)
    assert v.size == 1020 and not np.any(np.isnan(v))
    for f16, mant, emin, emax in ((1, 10, -14, 15), (0, 7, -126, 127)):
        out = R.from_op(R.to_op(v, f16), f16).astype(np.float64)
        assert np.any(np.isposinf(out) & np.isfinite(v)) and np.any(np.isneginf(out))                            # rounds to infinity
        assert np.any((out != 0) & (np.abs(out) < 2.0 ** emin))                                               # rounds to a subnormal
        assert np.any((out == 0) & (v != 0)) and np.any(out == (2 - 2.0 ** -mant) * 2.0 ** emax)               # to zero; the largest finite value
        assert np.any(out == 1 + 2.0 ** (1 - mant)) and np.any(out == 1) and np.any(out == 1 + 2.0 ** -mant)       # ties went both ways
    bits = v.view(np.uint32)
    assert np.any(bits == 0) and np.any(bits == 0x80000000)


# ---- exactness of the exact-answer inputs ------------------------------------------------------------------------------------------------------
VIT_EXACT = [(t, s, D, p) for t, s in T.VIT_POOL_TS for D in T.VIT_POOL_D for p in (0, 1)]


def _is_f32(a):
    return np.array_equal(np.asarray(a, np.float64).astype(F32).astype(np.float64), a)


@pytest.mark.parametrize("tokens,splits,D,ptn", VIT_EXACT)
def test_vit_exact_inputs_are_exact(tokens, splits, D, ptn):
    x, g, b, eps = T.vit_exact_case(tokens, splits, D, ptn)
    part, feat = T.vit_pool64(x, g, b, eps, ptn, splits)
    assert np.array_equal(part, np.round(part)) and np.abs(part).max() < 2 ** 24                  # integers: exact in any order of summation
    part32, feat32 = T.vit_pool32(x, g, b, eps, ptn, splits)
    assert np.array_equal(part32.astype(np.float64), part)
    # the contribution of every token, as float32 computes it, is the exact one
    assert np.array_equal(T.vit_contrib32(x, eps, ptn).astype(np.float64), T.vit_contrib64(x, eps, ptn))
    total = part.sum(1)
    if ptn:                     # the pooled row is m +- s: mean, variance and rstd are exact, the feature is fl(fl(+-g) + b)
        a = total / tokens
        m = a.mean(1, keepdims=True)
        assert np.array_equal(m, np.round(m)) and np.all(np.log2(np.abs(a - m)) % 1 == 0) and np.all(np.abs(a - m) == np.abs(a - m)[:, :1])
        assert np.array_equal(feat32.view(np.uint32), R.exact_answer(np.sign(a - m), g, b).view(np.uint32))
    else:                       # S / T, * g, + b: three single float32 operations on exact inputs, the same in any order of summation
        assert _is_f32(total) and np.max(np.abs(feat32 - feat)) <= 2.0 ** -20 * np.max(np.abs(feat))
    if tokens > 1 and not ptn:  # images have different token totals: |sum_t r_bt| = |total| in every column
        assert np.unique(np.abs(total[:, 0])).size == T.POOL_BATCH and np.all(np.abs(total) == np.abs(total[:, :1]))
    assert np.unique(total, axis=0).shape[0] == T.POOL_BATCH
    for f16 in (0, 1):          # the lo half carries something
        assert np.any(R.from_op(R.split_hilo(feat32, f16)[1], f16) != 0)


@pytest.mark.parametrize("n", T.COLSUM_NP)
@pytest.mark.parametrize("D", T.COLSUM_D)
def test_eva_exact_inputs_are_exact(n, D):
    for pad in T.COLSUM_PAD:
        x = T.eva_exact_case(n, pad, D)
        part = T.eva_colsum64(x, n)
        assert np.array_equal(part, np.round(part)) and np.array_equal(T.eva_colsum32(x, n).astype(np.float64), part)
        assert np.all(x[:, 0] == F32(1e30)) and np.all(x[:, 1 + n:] == F32(1e30)) and np.abs(x[:, 1:1 + n]).max() <= 50
        empty = T.empty_splits(n, T.EVA_SPLITS)
        assert (len(empty) > 0) == (n in (1, 10, 37)) and np.all(part[:, empty] == 0)               # 37: 13 splits of 3, three of none


@pytest.mark.parametrize("tokens", T.SW_MEAN_T)
@pytest.mark.parametrize("C", T.SW_MEAN_C)
def test_sw_mean_exact_inputs_are_exact(tokens, C):
    y = T.sw_exact_case(tokens, C)
    want = T.sw_mean64(y)
    assert _is_f32(want) and np.array_equal(T.sw_mean32(y).astype(np.float64), want)
    prefix = np.cumsum(y.astype(np.float64), 1)                       # the kernel adds the tokens in order: every prefix is exact
    assert _is_f32(prefix)
    for f16 in (0, 1):
        assert np.any(R.from_op(R.split_hilo(want.astype(F32), f16)[1], f16) != 0)


# ---- mutants --------------------------------------------------------------------------------------------------------------------------------
def _moved(a, b, bound):
    """some element differs by more than the bound (a NaN on one side counts: the GPU test compares bits, or asserts <= bound)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        return bool(np.any(~(np.abs(a - b) <= bound)))


def _pool_mutants(A, batch, count):
    out = {"drop the last token of a split": T.mutant_drop_last(A), "double a token": T.mutant_double(A, count // 2)}
    if batch > 1:
        out["first token of image 1 to image 0"] = T.mutant_move_first_of_image1(A, batch)
    return out


def _hi_only(feat32, f16):
    return R.from_op(R.split_hilo(feat32, f16)[0], f16)


@pytest.mark.parametrize("tokens,splits,D,ptn", VIT_EXACT)
def test_mutants_vit_exact(tokens, splits, D, ptn):
    """bound zero: a mutant must change a word of the partial buffer, which the GPU test compares whole, and for norm-then-pool a word of
    the feature too.  (Pool-then-norm with eps = 0 does not see a scaling of the pooled row, so doubling the only token, or dropping the
    one token whose z is zero, leaves that feature alone: the partials are what catches those.)"""
    x, g, b, eps = T.vit_exact_case(tokens, splits, D, ptn)
    part, feat = T.vit_pool64(x, g, b, eps, ptn, splits)
    A = T.assign(T.POOL_BATCH, tokens, 0, tokens, splits)
    for name, Am in _pool_mutants(A, T.POOL_BATCH, tokens).items():
        with np.errstate(invalid="ignore", divide="ignore"):            # one token, dropped: the LayerNorm of a zero row with eps = 0
            pm, fm = T.vit_pool64(x, g, b, eps, ptn, splits, Am)
        assert _moved(pm, part, 0), name
        assert ptn or _moved(fm.astype(F32), feat.astype(F32), 0), name
    for s in T.empty_splits(tokens, splits):                                    # an unwritten partial row holds the fill, a NaN
        pm = part.copy()
        pm[:, s] = np.nan
        assert _moved(pm, part, 0) and _moved(T.vit_finalize64(pm, g, b, eps, tokens, ptn), feat, 0)
    feat32 = T.vit_pool32(x, g, b, eps, ptn, splits)[1]
    for f16 in (0, 1):                                                          # the lo half left out: unwritten (fill) or zero
        lo = R.split_hilo(feat32, f16)[1]
        assert np.any(lo != T.FILL16) and np.any(lo != 0)


@pytest.mark.parametrize("kind", T.STAT_INPUT_KINDS)
@pytest.mark.parametrize("tokens,splits,D", T.VIT_STAT)
@pytest.mark.parametrize("ptn", [0, 1])
def test_mutants_vit_statistics(tokens, splits, D, ptn, kind):
    x, g, b, eps = T.vit_stat_case(kind, tokens, D)
    part, feat = T.vit_pool64(x, g, b, eps, ptn, splits)
    part32, feat32 = T.vit_pool32(x, g, b, eps, ptn, splits)
    e32p, e32 = R.e32_of(part32, part), R.e32_of(feat32, feat)
    A = T.assign(T.POOL_BATCH, tokens, 0, tokens, splits)
    for f16 in (0, 1):
        bound = R.hilo_bounds(feat, e32, f16)[1]
        for name, Am in _pool_mutants(A, T.POOL_BATCH, tokens).items():
            pm, fm = T.vit_pool64(x, g, b, eps, ptn, splits, Am)
            assert _moved(pm, part, e32p) and _moved(fm, feat, bound), name
        assert _moved(_hi_only(feat32, f16), feat, bound), "drop the lo half"


def _eva_mutants(x, n):
    batch, TS, _ = x.shape
    A = T.assign(batch, TS, 1, n, T.EVA_SPLITS)
    out = _pool_mutants(A, batch, n)
    out["include row 0"] = T.mutant_include(A, batch, T.EVA_SPLITS, TS, 0, 0)
    if TS > n + 1:
        last = (n - 1) // (-(-n // T.EVA_SPLITS))
        out["include a pad row"] = T.mutant_include(A, batch, T.EVA_SPLITS, TS, n + 1, last)
    return out


@pytest.mark.parametrize("n", T.COLSUM_NP)
@pytest.mark.parametrize("D", T.COLSUM_D)
def test_mutants_eva_colsum_exact(n, D):
    for pad in T.COLSUM_PAD:
        x = T.eva_exact_case(n, pad, D)
        part = T.eva_colsum64(x, n)
        names = _eva_mutants(x, n)
        assert ("include a pad row" in names) == (pad > 1)
        for name, Am in names.items():
            assert _moved(T.eva_colsum64(x, n, Am), part, 0), name
        for s in T.empty_splits(n, T.EVA_SPLITS):
            assert not np.array_equal(T.words(part[:, s]), np.full(part[:, s].size, T.FILL32, np.uint32))


@pytest.mark.parametrize("kind", T.STAT_INPUT_KINDS)
@pytest.mark.parametrize("n,TS,D", T.EVA_STAT)
def test_mutants_eva_chain_statistics(n, TS, D, kind):
    x, g, b, eps = T.eva_stat_case(kind, n, TS, D)
    part = T.eva_colsum64(x, n)
    feat = R.pool_ln64(part, g, b, eps, n)
    part32 = T.eva_colsum32(x, n)
    feat32 = R.pool_ln32(part32, g, b, eps, n)
    e32p, e32 = R.e32_of(part32, part), R.e32_of(feat32, feat)
    for f16 in (0, 1):
        bound = R.hilo_bounds(feat, e32, f16)[1]
        for name, Am in _eva_mutants(x, n).items():
            pm = T.eva_colsum64(x, n, Am)
            assert _moved(pm, part, e32p) and _moved(R.pool_ln64(pm, g, b, eps, n), feat, bound), name
        assert _moved(_hi_only(feat32, f16), feat, bound), "drop the lo half"


@pytest.mark.parametrize("tokens", T.SW_MEAN_T)
@pytest.mark.parametrize("C", T.SW_MEAN_C)
def test_mutants_sw_mean_exact(tokens, C):
    y = T.sw_exact_case(tokens, C)
    want = T.sw_mean64(y)
    for name, Am in _pool_mutants(T.assign(T.POOL_BATCH, tokens, 0, tokens, 1), T.POOL_BATCH, tokens).items():
        assert _moved(T.sw_mean64(y, Am).astype(F32), want.astype(F32), 0), name
    for f16 in (0, 1):
        lo = R.split_hilo(want.astype(F32), f16)[1]
        assert np.any(lo != T.FILL16) and np.any(lo != 0)


@pytest.mark.parametrize("kind", T.STAT_INPUT_KINDS)
@pytest.mark.parametrize("tokens,C", T.SW_STAT)
def test_mutants_sw_mean_statistics(tokens, C, kind):
    y = T.sw_stat_case(kind, tokens, C)
    want, rest = T.sw_mean64(y), T.sw_mean32(y)
    e32 = R.e32_of(rest, want)
    for f16 in (0, 1):
        bound = R.hilo_bounds(want, e32, f16)[1]
        for name, Am in _pool_mutants(T.assign(T.POOL_BATCH, tokens, 0, tokens, 1), T.POOL_BATCH, tokens).items():
            assert _moved(T.sw_mean64(y, Am), want, bound), name
        assert _moved(_hi_only(rest, f16), want, bound), "drop the lo half"
