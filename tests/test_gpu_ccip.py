"""GPU parity: CCIP feature encoder (CAFormer forward, bf16 MFMA, fp32 accumulate) vs the float32 torch-CPU
oracle (oracle/ccip.py; parity unpinned -- the reference's ONNX graph is not available, see its header).

Tolerance: north_star states none for this path (1e-3 is for the ViT logits).  The output is a LayerNorm-ed
feature (unit scale per component) that downstream code only uses through cosine similarity
(webui.py:303-335 via the feature index).  Measured on the synthetic checkpoints (unit-variance activations
through every StarReLU block, which squares and so doubles relative rounding errors): bf16 operands
max |df| 3.5e-2 (tiny) / 6.9e-2 (B36), cosine 0.99988; IEEE-half operands 4e-3 / 9e-3, cosine 0.999998 --
an 8x ratio, i.e. operand rounding only.  Bounds: bf16 max |df| <= 1e-1 and cosine >= 0.9995; half
max |df| <= 2e-2 and cosine >= 0.99999.

operand_f16 = 2 (e4m3 operands) is refused since round 4: test_ccip_e4m3_mode_is_withdrawn.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = {0: (1e-1, 0.9995), 1: (2e-2, 0.99999)}       # operand_f16 -> (max |df|, min cosine)


def _oracle(cfg, w, images_u8):
    from oracle import ccip as oc
    x = oc.preprocess_u8_nhwc(images_u8)
    f = oc.metaformer_forward(oc.to_torch(w), x, dims=cfg["dims"], depths=cfg["depths"], head_dim=cfg["head_dim"], eps=cfg["ln_eps"])
    return f.numpy(), x.numpy()


def _check(got, want, f16=0):
    err = np.abs(got - want).max()
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    print("CCIP (operand_f16=%d) max |df| = %.3e, min cosine = %.6f" % (f16, err, cos.min()))
    assert err <= TOL[f16][0], err
    assert cos.min() >= TOL[f16][1], cos.min()


@pytest.mark.parametrize("f16", [0, 1])
def test_ccip_tiny_matches_oracle(f16):
    from hiptagsearch import synth
    from hiptagsearch.cfeatures import CCIPEncoder
    cfg = dict(synth.CCIP_TINY, operand_f16=f16)
    w = synth.ccip_weights(cfg, seed=3)
    imgs = synth.images_u8(5, cfg["image_size"], seed=47)
    want, x = _oracle(cfg, w, imgs)
    enc = CCIPEncoder(cfg, w, max_batch=8)
    got = enc.forward_u8(imgs)
    _check(got, want, f16)
    # float32 NCHW entry point: the `input` array of gen_cfeatures.py:158, and the onnxruntime call shape
    got2 = enc.run(["output"], {"input": x})[0]
    _check(got2, want, f16)
    np.testing.assert_allclose(got2, got, atol=TOL[f16][0] / 4)
    # device in / out, and a batch larger than max_batch is chunked
    import torch
    d = torch.empty((5, cfg["dims"][3]), dtype=torch.float32, device="cuda")
    enc.forward_u8(torch.from_numpy(imgs).cuda(), out=d)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d.cpu().numpy(), got)
    imgs12 = synth.images_u8(12, cfg["image_size"], seed=48)
    np.testing.assert_array_equal(enc.forward_u8(imgs12)[:8], enc.forward_u8(imgs12[:8]))


@pytest.mark.parametrize("f16", [0, 1])
def test_ccip_tiny_float32_entry(f16):
    """The float32 NCHW entry (hipts_ccip_forward_f32: the one-thread-per-kernel-row gather with the 7 x 7 stride 4 pad 2 window and the
    unflipped float32 planes) on its own: a 64-pixel image gives a 16 x 16 stem grid, and the window crosses all four borders.  The
    normalised pixels the oracle's preprocess produces are the values the uint8 entry reads from its table, so the two entries build the
    same patch matrix and their features are equal bit for bit (measured: max difference exactly 0 in both operand modes)."""
    from hiptagsearch import synth
    from hiptagsearch.cfeatures import CCIPEncoder
    cfg = dict(synth.CCIP_TINY, operand_f16=f16)
    w = synth.ccip_weights(cfg, seed=3)
    imgs = synth.images_u8(3, cfg["image_size"], seed=51)
    want, x = _oracle(cfg, w, imgs)
    enc = CCIPEncoder(cfg, w, max_batch=4)
    got = enc(x)
    _check(got, want, f16)
    got_u8 = enc.forward_u8(imgs)
    print("CCIP (operand_f16=%d) float32 entry against forward_u8: max |df| = %.3e" % (f16, np.abs(got - got_u8).max()))
    np.testing.assert_array_equal(got, got_u8)


def test_ccip_without_res_scale_and_missing_tensor():
    from hiptagsearch import synth, _lib
    from hiptagsearch.cfeatures import CCIPEncoder
    cfg = dict(synth.CCIP_TINY)
    w = {k: v for k, v in synth.ccip_weights(cfg, seed=5).items() if "res_scale" not in k}      # res_scale tensors are optional
    imgs = synth.images_u8(2, cfg["image_size"], seed=49)
    want, _ = _oracle(cfg, w, imgs)
    _check(CCIPEncoder(cfg, w, max_batch=2).forward_u8(imgs), want)
    w.pop("stages.1.blocks.0.mlp.fc2.weight")
    with pytest.raises(_lib.HipTagSearchError, match="not set"):
        CCIPEncoder(cfg, w, max_batch=2).forward_u8(imgs)


@pytest.mark.parametrize("f16", [0, 1])
def test_ccip_b36_384_matches_oracle(f16):
    """config[4] geometry: CAFormer-B36 widths at 384 px (9216 / 2304 / 576 / 144 tokens), 2 images."""
    from hiptagsearch import synth
    from hiptagsearch.cfeatures import CCIPEncoder
    cfg = dict(synth.CCIP_B36_384, operand_f16=f16)
    w = synth.ccip_weights(cfg, seed=46)
    imgs = synth.images_u8(2, 384, seed=47)
    want, _ = _oracle(cfg, w, imgs)
    enc = CCIPEncoder(cfg, w, max_batch=2)
    got = enc.forward_u8(imgs)
    _check(got, want, f16)
    # run to run identical (no atomics, fixed schedules)
    np.testing.assert_array_equal(enc.forward_u8(imgs), got)
    print("CCIP B36@384: %.2f GFLOP / image" % (enc.flops_per_image() / 1e9))


def test_ccip_b36_384_batch_64_folded_layernorms():
    """Batch 64 (two sub-batch streams of 32 images): stage 2's residual launches have more tiles than half the CUs, so its LayerNorms are
    FOLDED (round 5: EPI_RESID_XG with res_scale writes gamma * x and the row sums, q | k, v and fc1 apply rstd / mean in their epilogues;
    csrc/ccip.hip) -- a path the 2-image test never takes.  Rows 0, 31, 32 and 63 against the float32 oracle of those images (the oracle
    does not depend on the batch), every row finite, and run to run identical."""
    from hiptagsearch import synth
    from hiptagsearch.cfeatures import CCIPEncoder
    cfg = dict(synth.CCIP_B36_384, operand_f16=1)
    w = synth.ccip_weights(cfg, seed=46)
    imgs = synth.images_u8(64, 384, seed=48)
    enc = CCIPEncoder(cfg, w, max_batch=64)
    got = enc.forward_u8(imgs)
    assert got.shape == (64, 768) and np.isfinite(got).all()
    pick = [0, 31, 32, 63]
    want, _ = _oracle(cfg, w, imgs[pick])
    _check(got[pick], want, 1)
    np.testing.assert_array_equal(enc.forward_u8(imgs), got)
    # a sub-batch of the same images without the fold (batch 8: stage 2 is 36 tiles, the two-workgroups-per-CU kernels): the two forms of
    # the LayerNorm round differently (gamma * x before the statistics are applied), nothing more
    small = CCIPEncoder(cfg, w, max_batch=8).forward_u8(imgs[:8])
    cos = (small * got[:8]).sum(1) / (np.linalg.norm(small, axis=1) * np.linalg.norm(got[:8], axis=1))
    assert np.abs(small - got[:8]).max() <= 2e-2 and cos.min() >= 0.99999, (np.abs(small - got[:8]).max(), cos.min())


def test_ccip_e4m3_mode_is_withdrawn():
    """operand_f16 = 2 (e4m3 operands for pwconv2 / fc1 / fc2, BASELINE.json configs[4]'s fp8 leg) was built in round 1 and withdrawn in
    round 4: cosine 0.968 against the float32 oracle on B36 @384, 1 % slower than half operands, and a CPU emulation of every scaling
    scheme the scaled MFMA offers (per-tensor, per-32-element E8M0 blocks, later stages only, activations only:
    tools/ccip_fp8_emulation.py) stays at 0.985 .. 0.995 -- three mantissa bits do not survive 36 blocks.  The library refuses it."""
    import hiptagsearch
    from hiptagsearch import synth
    from hiptagsearch.cfeatures import CCIPEncoder
    cfg = dict(synth.CCIP_TINY, operand_f16=2)
    with pytest.raises(hiptagsearch.HipTagSearchError):
        CCIPEncoder(cfg, synth.ccip_weights(cfg, seed=3), max_batch=2)


def test_ccip_two_sub_batch_streams_match_single_stream():
    """batch >= 32 runs as two sub-batches on two internal streams; rows must equal the single-stream results."""
    from hiptagsearch import synth
    from hiptagsearch.cfeatures import CCIPEncoder
    cfg = dict(synth.CCIP_TINY)
    w = synth.ccip_weights(cfg, seed=6)
    imgs = synth.images_u8(37, cfg["image_size"], seed=50)
    enc = CCIPEncoder(cfg, w, max_batch=40)
    got = enc.forward_u8(imgs)
    np.testing.assert_array_equal(enc.forward_u8(imgs), got)
    small = CCIPEncoder(cfg, w, max_batch=8)                      # batches of 8: one stream
    np.testing.assert_array_equal(small.forward_u8(imgs), got)


def _dwconv7_f64(x_f16, w, half_weights):
    """out[b][y][x][c] = sum_{ky,kx} in[b][y+ky-3][x+kx-3][c] * w[c][ky*7+kx] in float64 (the timm SepConv's depthwise conv,
    MetaFormer `SepConv.dwconv`: padding 3, no bias); half_weights: the weights as the matrix-core kernel holds them."""
    x = x_f16.astype(np.float64)
    wk = (w.astype(np.float16) if half_weights else w).astype(np.float64)
    B, H, _, C = x.shape
    xp = np.zeros((B, H + 6, H + 6, C))
    xp[:, 3:H + 3, 3:H + 3] = x
    out = np.zeros_like(x)
    for ky in range(7):
        for kx in range(7):
            out += xp[:, ky:ky + H, kx:kx + H] * wk[:, ky * 7 + kx]
    return out


@pytest.mark.parametrize("H,C,mode", [(16, 64, 1), (24, 128, 2), (48, 64, 3), (50, 64, 2), (50, 64, 3), (96, 64, 1), (33, 64, 1), (9, 64, 0), (24, 128, 0)])
def test_dwconv7_kernels_against_float64(H, C, mode):
    """The depthwise 7x7 on its own (hiptsdbg_dwconv7): the float32-FMA kernel (mode 0) and the matrix-core kernel (Toeplitz operands,
    32- and 48-column tiles; sides that are not multiples of the tile, borders inside the first and last tile) against a float64
    convolution of the same half inputs -- with the weights rounded to half for the matrix-core kernel, which is its only deviation.
    The half outputs may differ from the rounded float64 sums by one unit in the last place (float32 accumulation order)."""
    import ctypes, os, sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(ROOT, "anime-illust-image-searcher_amd"))
    from hiptagsearch import _lib
    lib = _lib.load()
    f = lib.hiptsdbg_dwconv7
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    rng = np.random.default_rng(H * 1000 + C + mode)
    B = 3
    x = rng.standard_normal((B, H, H, C)).astype(np.float16)
    x[0, 0, 0, :] = 7.0                                  # corners: a wrong halo shows here first
    x[1, H - 1, H - 1, :] = -5.0
    w = (rng.standard_normal((C, 49)) * 0.2).astype(np.float32)
    out = np.empty_like(x)
    st = f(x.ctypes.data, w.ctypes.data, out.ctypes.data, B, H, C, mode, 0, None)
    assert st == 0, _lib.last_error()
    want = _dwconv7_f64(x, w, half_weights=mode != 0)
    ulp = np.spacing(np.abs(want).astype(np.float16)).astype(np.float64)
    err = np.abs(out.astype(np.float64) - want)
    assert np.isfinite(out).all()
    assert (err <= 0.5 * ulp + 2e-6 * np.abs(want) + 1e-6).all(), (err.max(), np.unravel_index(err.argmax(), err.shape))
    if mode != 0:      # and the two kernels agree to the weight rounding: |dw| <= 2^-12 |w| per tap
        ref = np.empty_like(x)
        assert f(x.ctypes.data, w.ctypes.data, ref.ctypes.data, B, H, C, 0, 0, None) == 0
        assert np.abs(out.astype(np.float64) - ref.astype(np.float64)).max() <= 2e-2


@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("M,C,with_rs,with_ln", [(300, 128, True, True), (512, 256, True, True), (37, 256, False, True), (256, 128, False, False), (1000, 256, True, False)])
def test_mlp_fused_against_float64(M, C, with_rs, with_ln, waves):
    """The fused MLP kernel alone (csrc/mlp.hip through hiptsdbg_mlp_fused; the MetaFormer `Mlp` + scaled residual + next LayerNorm):
    x = rs * x + StarReLU(xn W1^T) W2^T against float64 with the kernel's roundings (half weights, hidden activations rounded to half),
    row counts that are no multiple of a wave's 32 or a workgroup's 128 / 256 rows, both workgroup sizes."""
    import ctypes, os, sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(ROOT, "anime-illust-image-searcher_amd"))
    from hiptagsearch import _lib
    lib = _lib.load()
    f = lib.hiptsdbg_mlp_fused
    f.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    rng = np.random.default_rng(M + C)
    xn = rng.standard_normal((M, C)).astype(np.float16)
    w1 = (rng.standard_normal((4 * C, C)) / np.sqrt(C)).astype(np.float32)
    w2 = (rng.standard_normal((C, 4 * C)) / np.sqrt(4 * C)).astype(np.float32)
    x = rng.standard_normal((M, C)).astype(np.float32) * 2
    rs = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32)
    g = (1 + 0.2 * rng.standard_normal(C)).astype(np.float32)
    s, b, eps = 0.8944, -0.4472, 1e-6
    S = (xn.astype(np.float64) @ w1.astype(np.float16).astype(np.float64).T).astype(np.float32)
    r = np.maximum(S, np.float32(0))
    P = (r * r * np.float32(s) + np.float32(b)).astype(np.float16)
    O = P.astype(np.float64) @ w2.astype(np.float16).astype(np.float64).T
    want = (x.astype(np.float64) * rs if with_rs else x.astype(np.float64)) + O
    got = x.copy()
    xo = np.zeros((M, C), dtype=np.float16)
    st = f(xn.ctypes.data, w1.ctypes.data, w2.ctypes.data, got.ctypes.data, rs.ctypes.data if with_rs else None, g.ctypes.data if with_ln else None,
           xo.ctypes.data, M, C, s, b, eps, 0, None, waves)
    assert st == 0, _lib.last_error()
    # a hidden value that lands on a rounding boundary of half may round the other way under another summation order: 2^-11 relative on one
    # of 4C terms -- far below the bound
    err = np.abs(got - want).max()
    print("fused MLP M=%d C=%d: max |dx| = %.3e (|x| ~ %.2f)" % (M, C, err, np.abs(want).mean()))
    assert err <= 2e-3, err
    if with_ln:
        mu = want.mean(1, keepdims=True)
        ln = (want - mu) / np.sqrt(((want - mu) ** 2).mean(1, keepdims=True) + eps) * g
        e2 = np.abs(xo.astype(np.float64) - ln).max()
        assert e2 <= 4e-3, e2
