"""GPU parity of the SwinV2 tagger forward (csrc/swinv2.hip, csrc/swin_attn.hip) against the float64 CPU restatement tests/swinv2_ref.py
(itself pinned to transformers' Swinv2ForImageClassification by tests/test_swinv2_host.py).

Tolerances: bound = the first GPU run's measured value x 1.25 (values in the comments below).  Conditions that are not tolerances: the
labels selected on the trained-like checkpoint equal the oracle's on every image, u8 and f32 inputs give the same bits, batches give
the same bits as single images, and the window attention is further from a -inf-masked oracle than its bound.

The two exact-answer window tests (test_window_attention_counts_its_group, test_window_attention_places_every_token) are not measured:
their inputs (tests/attention_exact.py) have a closed-form answer and their bounds follow from the 16-bit output type."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "anime-illust-image-searcher_amd")
sys.path.insert(0, HERE)

import swinv2_ref  # noqa: E402

pytestmark = pytest.mark.gpu

# Bounds = measured x 1.25, first GPU run of this forward (MI355X, the code as it stands here):
#   window attention alone (|v| ~ 1, both input kinds): bf16 operands max |d| 1.74e-2, half 3.34e-3; against a -inf mask 2.6-4.2
#   tiny, 4 noise + 6 structured images: bf16 max |dlogit| 2.67e-3, half 3.44e-4 (logit rms 0.33); u8 and f32 inputs bit-identical
#   B @448 half, seed-0 weights, 3 noise + 6 structured: max |dlogit| 8.43e-4 (the flat picture; noise images <= 1.8e-4) -- x 1.25 would
#   exceed the 1e-3 bar of the other taggers, which stays the bound
#   B @448 trained-like (logit rms 10.3): max |dlogit| 3.37e-3, 28-32 labels per image, all equal to the oracle's
#   B @448 trained-like residual stream after stages 0 / 1 / 2 / 3: max |d| / max |x| 1.90e-4 / 3.93e-4 / 9.51e-4 / 9.90e-4
ATT_MAX = {0: 2.2e-2, 1: 4.2e-3}          # window attention alone, max |d| against float64, by operand_f16
TINY_MAX = {0: 3.3e-3, 1: 4.3e-4}         # max |dlogit|, tiny config, by operand_f16
B_MAX = 1.0e-3                            # SwinV2-B @448, half operands, seed-0 weights: max |dlogit|
B_TRAINED_MAX = 4.2e-3                    # trained-like checkpoint: max |dlogit| (labels must be equal regardless)
STREAM_REL = {0: 2.4e-4, 1: 4.9e-4, 2: 1.19e-3, 3: 1.24e-3}     # residual stream after each stage: max |d| / max |x|
SWINV2_B_GFLOP = 130.74


def _lib():
    return ctypes.CDLL(os.path.join(PKG, "libhip_tagsearch.so"))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _oracle(cfg, w, x_f32):
    with torch.no_grad():
        lg, _ = swinv2_ref.forward(swinv2_ref.to_torch(w), torch.from_numpy(np.asarray(x_f32)).double(), cfg)
    return lg.numpy()


def _errors(got, want):
    d = got.astype(np.float64) - want
    mx = np.abs(d).max(1)
    rms = np.sqrt((d ** 2).mean(1))
    return mx, rms, rms / np.sqrt((want ** 2).mean(1))


def _inputs(cfg, n_noise, structured=True):
    from hiptagsearch import synth
    imgs = synth.images_u8(n_noise, cfg["image_size"], seed=21)
    if structured:
        imgs = np.concatenate([imgs, synth.structured_images_u8(cfg["image_size"], seed=77)])
    return imgs, swinv2_ref.preprocess_u8(imgs, cfg["norm_mean"], cfg["norm_std"]).numpy()


def _window_attention_gpu(q, k, v, ls, cpb, side, window, shift, f16):
    B, N, C = q.shape
    f = [np.ascontiguousarray(t.numpy() if torch.is_tensor(t) else t, dtype=np.float32) for t in (q, k, v, ls, cpb)]
    out = np.empty((B, N, C), dtype=np.float32)
    st = _lib().hiptsdbg_swinv2_window_attention(_p(f[0]), _p(f[1]), _p(f[2]), _p(f[3]), _p(f[4]), B, C // 32, side, window, shift, f16,
                                                 _p(out))
    assert st == 0
    return out, f


@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("window,shift", [(7, 0), (7, 3), (14, 0), (14, 7)])
def test_window_attention_matches_float64(window, shift, f16):
    """The kernel alone against the float64 restatement: logit scales at ln 10, at the clamp and above it (ln 150), a spread position
    bias, noise inputs and a region layout where the -100 mask decides the output.  Negative control (shifted windows): the same
    output against an oracle with -inf in place of -100 must miss the bound."""
    side, nh = 2 * window, 4
    g = torch.Generator().manual_seed(window * 10 + shift)
    ls = torch.tensor([np.log(10.0), np.log(100.0), np.log(150.0), np.log(30.0)], dtype=torch.float64)
    cpb = 16 * torch.sigmoid(torch.randn(nh, (2 * window - 1) ** 2, generator=g, dtype=torch.float64))
    qn, kn, vn = (torch.randn(2, side * side, 32 * nh, generator=g, dtype=torch.float64) for _ in range(3))
    qm, km, vm = swinv2_ref.masked_keys_win_qkv(2, side, window, shift, nh, seed=window + shift)
    q, k, v = torch.cat([qn, qm]), torch.cat([kn, km]), torch.cat([vn, vm])
    got, f = _window_attention_gpu(q, k, v, ls, cpb, side, window, shift, f16)
    qf, kf, vf, lf, cf = (torch.from_numpy(t).double() for t in f)                # the float32 inputs the kernel saw
    want = swinv2_ref.window_attention(qf, kf, vf, lf, cf, side, window, shift).numpy()
    err = np.abs(got - want).max()
    print("window %d shift %d operand_f16 %d: max |d| %.3e (noise %.3e, masked layout %.3e)" % (
        window, shift, f16, err, np.abs(got - want)[:2].max(), np.abs(got - want)[2:].max()))
    assert np.isfinite(got).all()
    assert err <= ATT_MAX[f16], err
    if shift:
        want_inf = swinv2_ref.window_attention(qf, kf, vf, lf, cf, side, window, shift, mask_value=-float("inf")).numpy()
        err_inf = np.abs(got - want_inf).max()
        print("   against a -inf mask: %.3e" % err_inf)
        assert err_inf > ATT_MAX[f16]


# Three windows per axis: interior windows and, shifted, all nine roll regions; 1, 2, 2, 7 and 8 key chunks of 32 (16: the launcher's limit)
EXACT_WINDOWS = [(4, 12, 0), (4, 12, 2), (7, 21, 0), (7, 21, 3), (8, 24, 4), (14, 42, 7), (16, 48, 0), (16, 48, 8)]


@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("window,side,shift", EXACT_WINDOWS)
def test_window_attention_counts_its_group(window, side, shift, f16):
    """Every cosine 1, no position bias: a token's output is the float64 mean of v over the tokens of its window that share its roll
    region (tests/attention_exact.py, by roll, partition and region; checked against swinv2_ref.window_attention on the host).  Bound
    ulp16(want) + 2^-16 max |v| from the output type: equal numerators, at most 256 float32 terms; a key across regions weighs e^-100."""
    import attention_exact as ax
    regions = swinv2_ref.raster_regions(side, window, shift).numpy()
    q, k, v, ls, cpb, want = ax.window_counting(2, 2, side, window, shift, regions, f16)
    got, _ = _window_attention_gpu(q, k, v, ls, cpb, side, window, shift, f16)
    bad = ax.window_counting_bad(got, want, f16, float(np.abs(v).max()))
    print("window %d side %d shift %d operand_f16 %d: max |d| %.3e" % (window, side, shift, f16, np.abs(got - want).max()))
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[0], np.abs(got - want).max())


@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("window,side,shift", EXACT_WINDOWS)
def test_window_attention_places_every_token(window, side, shift, f16):
    """k[j] = the window-local index of j as two one-hot digits, q[i] = the code of the next token of i's (window, region) group: scores
    100, 50 or 0, so o[i] = v[next(i)] within one spacing of the output type -- every query row and every key of every window placed."""
    import attention_exact as ax
    regions = swinv2_ref.raster_regions(side, window, shift).numpy()
    q, k, v, ls, cpb, want = ax.window_placement(2, 2, side, window, shift, regions, f16)
    got, _ = _window_attention_gpu(q, k, v, ls, cpb, side, window, shift, f16)
    bad = ax.window_placement_bad(got, want, f16)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[0], np.abs(got - want).max())


def test_tiny_both_operand_modes_u8_and_f32():
    from hiptagsearch import synth
    from hiptagsearch.tagger import SwinV2Tagger
    cfg = dict(synth.SWINV2_TINY)
    w = synth.swinv2_weights(cfg, seed=3)
    imgs, x = _inputs(cfg, 4)
    want = _oracle(cfg, w, x)
    worst = {}
    for f16 in (0, 1):
        m = SwinV2Tagger(dict(cfg, operand_f16=f16), w, max_batch=16)
        lg_u8, pr_u8 = m.forward_u8(imgs)
        lg_f, _ = m.forward(x)
        m.close()
        assert np.isfinite(lg_u8).all()
        np.testing.assert_array_equal(lg_u8, lg_f)
        np.testing.assert_allclose(pr_u8, 1.0 / (1.0 + np.exp(-lg_u8.astype(np.float64))), rtol=0, atol=2e-6)
        mx, _, rel = _errors(lg_u8, want)
        worst[f16] = mx.max()
        print("tiny operand_f16=%d: max |dlogit| %.3e  rms-relative %.3e  (logit rms %.3f)" % (f16, mx.max(), rel.max(),
                                                                                              np.sqrt((want ** 2).mean())))
        assert worst[f16] <= TINY_MAX[f16], (f16, worst[f16])


def test_b448_half_operands_matches_oracle():
    from hiptagsearch import synth
    from hiptagsearch.tagger import SwinV2Tagger
    cfg = dict(synth.SWINV2_B_448)
    w = synth.swinv2_weights(cfg, seed=0)
    imgs, x = _inputs(cfg, 3)
    want = _oracle(cfg, w, x)
    m = SwinV2Tagger(cfg, w, max_batch=16)
    assert abs(m.flops_per_image() - SWINV2_B_GFLOP * 1e9) <= 1e-3 * SWINV2_B_GFLOP * 1e9
    lg, _ = m.forward_u8(imgs)
    m.close()
    assert np.isfinite(lg).all()
    mx, rms, rel = _errors(lg, want)
    for i in range(len(imgs)):
        print("B@448 image %d: max |dlogit| %.3e  rms %.3e  rms-relative %.3e" % (i, mx[i], rms[i], rel[i]))
    assert mx.max() <= B_MAX, mx


def test_b448_residual_stream_per_stage():
    from hiptagsearch import synth
    from hiptagsearch.tagger import SwinV2Tagger
    cfg = dict(synth.SWINV2_B_448)
    w = synth.swinv2_weights(cfg, seed=0, trained_like=True)
    _, x = _inputs(cfg, 1, structured=False)
    x0 = np.ascontiguousarray(x[:1], dtype=np.float32)
    m = SwinV2Tagger(cfg, w, max_batch=1)
    lib = _lib()
    for stage, (H, _, C, _) in enumerate(swinv2_ref.stage_geometry(cfg)):
        out = np.empty((1, H * H * C), dtype=np.float32)
        assert lib.hiptsdbg_swinv2_stream(m._h, _p(x0), 1, stage, _p(out)) == 0
        with torch.no_grad():
            ref = swinv2_ref.features(swinv2_ref.to_torch(w), torch.from_numpy(x0).double(), cfg, stop_stage=stage).reshape(1, -1).numpy()
        err = np.abs(out - ref).max() / np.abs(ref).max()
        print("B@448 trained-like stream after stage %d: max |d| / max |x| %.3e" % (stage, err))
        assert err <= STREAM_REL[stage], (stage, err)
    m.close()


def test_b448_trained_like_selects_the_oracles_labels():
    from hiptagsearch import synth
    from hiptagsearch.tagger import SwinV2Tagger, TagSelector
    from oracle import tags as otags
    cfg = dict(synth.SWINV2_B_448)
    w = synth.swinv2_weights(cfg, seed=0, trained_like=True)
    imgs, x = _inputs(cfg, 2)
    want = _oracle(cfg, w, x)
    m = SwinV2Tagger(cfg, w, max_batch=16)
    lg, probs = m.forward_u8(imgs)
    mx, _, rel = _errors(lg, want)
    print("B@448 trained-like: logit rms %.2f  max |dlogit| %.3e  rms-relative %.3e" % (np.sqrt((want ** 2).mean()), mx.max(), rel.max()))
    names, cat = synth.label_table(cfg["num_classes"])
    sel = TagSelector(cat, max_batch=16)
    counts, ids, _ = sel.run(probs, 0.3, True, 0.3, True)
    want_probs = otags.sigmoid_f32(want.astype(np.float32))
    gi, ci = list(np.where(cat == 0)[0]), list(np.where(cat == 4)[0])
    n_sel = []
    for i in range(len(imgs)):
        g, c, _, _ = otags.select_indices(want_probs[i], gi, ci, 0.3, True, 0.3, True)
        got = list(ids[i, :counts[i, 0] + counts[i, 1]])
        n_sel.append(len(got))
        assert sorted(got) == sorted(list(g) + list(c)), (i, got, list(g), list(c))
    print("  labels selected per image:", n_sel)
    assert min(n_sel) >= 5
    assert mx.max() <= B_TRAINED_MAX, mx
    sel.close()
    m.close()


def test_b448_batch_invariance_bit_for_bit():
    """A batch of 64 (two sub-batch streams) equals the same images one at a time and inside an odd batch of 33."""
    from hiptagsearch import synth
    from hiptagsearch.tagger import SwinV2Tagger
    cfg = dict(synth.SWINV2_B_448)
    m = SwinV2Tagger(cfg, synth.swinv2_weights(cfg, seed=1), max_batch=64)
    imgs = synth.images_u8(64, 448, seed=99)
    full, _ = m.forward_u8(imgs)
    odd, _ = m.forward_u8(imgs[7:40])
    np.testing.assert_array_equal(odd, full[7:40])
    for i in (0, 1, 31, 32, 33, 63):
        one, _ = m.forward_u8(imgs[i:i + 1])
        np.testing.assert_array_equal(one[0], full[i])
    m.close()


def test_errors_missing_tensor_and_bad_config():
    from hiptagsearch import _lib as L, synth
    from hiptagsearch.tagger import SwinV2Tagger
    cfg = dict(synth.SWINV2_TINY)
    w = synth.swinv2_weights(cfg, seed=3)
    del w["layers.2.blocks.1.attn.cpb_mlp.2.weight"]
    m = SwinV2Tagger(cfg, w, max_batch=2)
    with pytest.raises(L.HipTagSearchError) as e:
        m.forward_u8(synth.images_u8(1, 224))
    assert e.value.status == -5 and "layers.2.blocks.1.attn.cpb_mlp.2.weight" in str(e.value)
    m.close()
    for bad in (dict(cfg, window=6),                         # 6 does not divide the side 56
                dict(cfg, heads=(4, 4, 8, 16)),              # head_dim 16 in stage 0
                dict(cfg, window=20, image_size=640)):       # 400-token windows
        with pytest.raises(L.HipTagSearchError) as e:
            SwinV2Tagger(bad, {}, max_batch=2)
        assert e.value.status == -1


def test_cli_swinv2_tiny_writes_the_oracles_tags(tmp_path):
    from PIL import Image
    from hiptagsearch import synth
    from oracle import tags as otags
    cfg = dict(synth.SWINV2_TINY)
    os.makedirs(tmp_path / "imgs")
    imgs = synth.images_u8(5, 224, seed=4321)
    for i, im in enumerate(imgs):
        Image.fromarray(im).save(tmp_path / "imgs" / ("%02d.png" % i))
    r = subprocess.run([sys.executable, os.path.join(PKG, "tagging.py"), "--dir", "imgs", "--model", "swinv2-tiny"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(tmp_path / "tags-wd-tagger.txt", encoding="utf-8").read().splitlines()
    by_path = {l.split(",")[0]: l for l in lines}
    assert len(lines) == 5
    w = synth.swinv2_weights(cfg, seed=0, trained_like=True)          # the CLI's stand-in checkpoint (Predictor.load_model)
    want_probs = otags.sigmoid_f32(_oracle(cfg, w, swinv2_ref.preprocess_u8(imgs).numpy()).astype(np.float32))
    names, cat = synth.label_table(cfg["num_classes"])
    want = otags.predict_lines(want_probs, names, cat)
    for i in range(5):
        p = os.path.join("imgs", "%02d.png" % i)
        assert by_path[p] == p + "," + want[i], "image %d" % i
