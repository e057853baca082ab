"""GPU parity of the ConvNeXt tagger forward (csrc/convnext.hip) against the float64 CPU restatement tests/convnext_ref.py
(itself pinned to transformers' ConvNextForImageClassification by tests/test_convnext_host.py).

Tolerances: bound = the first GPU run's measured value x 1.25 (values and run in the comments below).  Two conditions are not
tolerances: the labels selected on the trained-like checkpoint equal the oracle's on every image, and half operands are not less
accurate than bf16."""
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

import convnext_ref  # noqa: E402

pytestmark = pytest.mark.gpu

# Bounds = measured x 1.25, first GPU run of this forward (MI355X, tests as they stand here, u8 and f32 inputs identical):
#   tiny, 4 noise + 6 structured images: bf16 operands max |dlogit| 5.84e-3, half 8.91e-4 (logit rms 0.63)
#   B @448 half, seed-0 plain weights, 3 noise + 6 structured: max |dlogit| 6.93e-4, rms-relative 2.41e-4; every layer scale 1e-6:
#   8.77e-4 / 3.32e-4 (one bound for both: the larger); residual stream after stage 0: max |d| / max |x| 3.95e-5
#   B @448 trained-like (logit rms 10.4): max |dlogit| 2.76e-3, rms-relative 6.3e-5, 27-34 labels per image, all equal to the oracle's
TINY_MAX = {0: 7.3e-3, 1: 1.12e-3}       # max |dlogit|, tiny config, by operand_f16
B_MAX, B_REL = 1.1e-3, 4.2e-4            # ConvNeXt-B @448, half operands: max |dlogit|, rms-relative
STREAM0_REL = 5e-5
# branches at gamma = 1e-6 in the stage-0 stream (test_b448_layer_scale_1e6_branches_survive): relative error 4.16e-2 on the first GPU
# run -- the fp32 stream's own rounding of x + 1e-6 y (a float32 CPU run of the restatement gives 4.2e-2) -- and 0.41 with gamma folded
# into half fc2
BRANCH_REL = 5.2e-2


def _oracle(cfg, w, x_f32):
    lg, _ = convnext_ref.forward(convnext_ref.to_torch(w), torch.from_numpy(np.asarray(x_f32)).double(), cfg["depths"], cfg["ln_eps"])
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
    return imgs, convnext_ref.preprocess_u8(imgs, cfg["norm_mean"], cfg["norm_std"]).numpy()


def test_tiny_both_operand_modes_u8_and_f32():
    from hiptagsearch import synth
    from hiptagsearch.tagger import ConvNeXtTagger
    cfg = dict(synth.CONVNEXT_TINY)
    w = synth.convnext_weights(cfg, seed=3)
    imgs, x = _inputs(cfg, 4)
    want = _oracle(cfg, w, x)
    worst = {}
    for f16 in (0, 1):
        m = ConvNeXtTagger(dict(cfg, operand_f16=f16), w, max_batch=16)
        lg_u8, pr_u8 = m.forward_u8(imgs)
        lg_f, _ = m.forward(x)
        m.close()
        assert np.isfinite(lg_u8).all() and np.isfinite(lg_f).all()
        np.testing.assert_allclose(pr_u8, 1.0 / (1.0 + np.exp(-lg_u8.astype(np.float64))), rtol=0, atol=2e-6)
        for name, lg in (("u8", lg_u8), ("f32", lg_f)):
            mx, _, rel = _errors(lg, want)
            print("tiny operand_f16=%d %s: max |dlogit| %.3e  rms-relative %.3e  (logit rms %.3f)" % (f16, name, mx.max(), rel.max(),
                                                                                                   np.sqrt((want ** 2).mean())))
            worst[f16] = max(worst.get(f16, 0.0), mx.max())
        assert worst[f16] <= TINY_MAX[f16], (f16, worst[f16])
    assert worst[1] <= worst[0]          # half operands are not less accurate than bf16


def test_b448_half_operands_matches_oracle():
    from hiptagsearch import synth
    from hiptagsearch.tagger import ConvNeXtTagger
    cfg = dict(synth.CONVNEXT_B_448)
    w = synth.convnext_weights(cfg, seed=0)
    imgs, x = _inputs(cfg, 3)
    want = _oracle(cfg, w, x)
    m = ConvNeXtTagger(cfg, w, max_batch=16)
    assert abs(m.flops_per_image() - 122.85e9) <= 1e-3 * 122.85e9
    lg, _ = m.forward_u8(imgs)
    assert np.isfinite(lg).all()
    mx, rms, rel = _errors(lg, want)
    for i in range(len(imgs)):
        print("B@448 image %d: max |dlogit| %.3e  rms %.3e  rms-relative %.3e" % (i, mx[i], rms[i], rel[i]))
    assert mx.max() <= B_MAX and rel.max() <= B_REL, (mx, rel)
    # every layer scale at timm's initial 1e-6: the logits still match the oracle to the same bound.  (This alone cannot see whether the
    # branches survive -- at 1e-6 they move the logits by ~4e-5, far below the bound: test_b448_layer_scale_1e6_branches_survive does.)
    w6 = dict(w)
    for k in w6:
        if k.endswith(".gamma"):
            w6[k] = np.full_like(w6[k], 1e-6)
    want6 = _oracle(cfg, w6, x[:4])
    m6 = ConvNeXtTagger(cfg, w6, max_batch=16)
    lg6, _ = m6.forward_u8(imgs[:4])
    mx6, _, rel6 = _errors(lg6, want6)
    print("B@448 layer scales 1e-6: max |dlogit| %.3e  rms-relative %.3e" % (mx6.max(), rel6.max()))
    assert mx6.max() <= B_MAX and rel6.max() <= B_REL, (mx6, rel6)
    # the stream after stage 0 (debug entry) against the oracle's: a blocks-only check that places a failure
    lib = ctypes.CDLL(os.path.join(PKG, "libhip_tagsearch.so"))
    n = 112 * 112 * 128
    out = np.empty((1, n), dtype=np.float32)
    x0 = np.ascontiguousarray(x[:1], dtype=np.float32)
    assert lib.hiptsdbg_convnext_stream(m._h, x0.ctypes.data_as(ctypes.c_void_p), 1, 0, out.ctypes.data_as(ctypes.c_void_p)) == 0
    ref0 = convnext_ref.features(convnext_ref.to_torch(w), torch.from_numpy(x0).double(), cfg["depths"], stop_stage=0)
    ref0 = ref0.permute(0, 2, 3, 1).reshape(1, n).numpy()
    err0 = np.abs(out - ref0).max() / np.abs(ref0).max()
    print("B@448 stream after stage 0: max |d| / max |x| %.3e" % err0)
    assert err0 <= STREAM0_REL
    m.close()
    m6.close()


def test_b448_trained_like_selects_the_oracles_labels():
    from hiptagsearch import synth
    from hiptagsearch.tagger import ConvNeXtTagger, TagSelector
    from oracle import tags as otags
    cfg = dict(synth.CONVNEXT_B_448)
    w = synth.convnext_weights(cfg, seed=0, trained_like=True)
    imgs, x = _inputs(cfg, 2)
    want = _oracle(cfg, w, x)
    m = ConvNeXtTagger(cfg, w, max_batch=16)
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
    sel.close()
    m.close()


def test_b448_batch_invariance_bit_for_bit():
    """A batch of 64 (two sub-batch streams) equals the same images one at a time and inside an odd batch of 33."""
    from hiptagsearch import synth
    from hiptagsearch.tagger import ConvNeXtTagger
    cfg = dict(synth.CONVNEXT_B_448)
    m = ConvNeXtTagger(cfg, synth.convnext_weights(cfg, seed=1), max_batch=64)
    imgs = synth.images_u8(64, 448, seed=99)
    full, _ = m.forward_u8(imgs)
    odd, _ = m.forward_u8(imgs[7:40])
    np.testing.assert_array_equal(odd, full[7:40])
    for i in (0, 1, 31, 32, 33, 63):
        one, _ = m.forward_u8(imgs[i:i + 1])
        np.testing.assert_array_equal(one[0], full[i])
    m.close()


def test_errors_missing_tensor_and_bad_config():
    from hiptagsearch import _lib, synth
    from hiptagsearch.tagger import ConvNeXtTagger
    cfg = dict(synth.CONVNEXT_TINY)
    w = synth.convnext_weights(cfg, seed=3)
    del w["stages.2.blocks.1.mlp.fc2.bias"]
    m = ConvNeXtTagger(cfg, w, max_batch=2)
    with pytest.raises(_lib.HipTagSearchError) as e:
        m.forward_u8(synth.images_u8(1, 64))
    assert e.value.status == -5 and "stages.2.blocks.1.mlp.fc2.bias" in str(e.value)
    m.close()
    for bad in (dict(cfg, image_size=48), dict(cfg, dims=(128, 256, 520, 1024)), dict(cfg, dims=(128, 256, 512, 2048))):
        with pytest.raises(_lib.HipTagSearchError) as e:
            ConvNeXtTagger(bad, {}, max_batch=2)
        assert e.value.status == -1


def test_cli_convnext_tiny_writes_the_oracles_tags(tmp_path):
    from PIL import Image
    from hiptagsearch import synth
    from oracle import tags as otags
    cfg = dict(synth.CONVNEXT_TINY)
    os.makedirs(tmp_path / "imgs")
    imgs = synth.images_u8(5, 64, seed=4321)
    for i, im in enumerate(imgs):
        Image.fromarray(im).save(tmp_path / "imgs" / ("%02d.png" % i))
    r = subprocess.run([sys.executable, os.path.join(PKG, "tagging.py"), "--dir", "imgs", "--model", "convnext-tiny"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(tmp_path / "tags-wd-tagger.txt", encoding="utf-8").read().splitlines()
    by_path = {l.split(",")[0]: l for l in lines}
    assert len(lines) == 5
    w = synth.convnext_weights(cfg, seed=0, trained_like=True)          # the CLI's stand-in checkpoint (Predictor.load_model)
    want_probs = otags.sigmoid_f32(_oracle(cfg, w, convnext_ref.preprocess_u8(imgs).numpy()).astype(np.float32))
    names, cat = synth.label_table(cfg["num_classes"])
    want = otags.predict_lines(want_probs, names, cat)
    for i in range(5):
        p = os.path.join("imgs", "%02d.png" % i)
        assert by_path[p] == p + "," + want[i], "image %d" % i


def _stream0(model, x0):
    """The fp32 residual stream after stage 0 (hiptsdbg_convnext_stream), [1, H*H*C]."""
    lib = ctypes.CDLL(os.path.join(PKG, "libhip_tagsearch.so"))
    out = np.empty((1, 112 * 112 * 128), dtype=np.float32)
    assert lib.hiptsdbg_convnext_stream(model._h, x0.ctypes.data_as(ctypes.c_void_p), 1, 0, out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out.astype(np.float64)


def test_b448_layer_scale_1e6_branches_survive():
    """timm initialises the layer scale at 1e-6.  gamma folded into W2 and rounded to half would put gamma W2 in the subnormal range,
    which the MFMA reads as zero: the blocks' branches would vanish while the logits still matched the oracle to ~1e-3 (the branches
    move them by ~4e-5 at this scale).  So the branch contribution is measured itself, in the fp32 stream after stage 0: (stream with
    every gamma = 1e-6) - (stream with gamma = 0), against the float64 oracle's same difference.  A negative control hands the library a
    checkpoint with gamma folded into fc2 (weights and bias times gamma, gamma = 1), the defect this guards against, and must fail the
    bound.  Measured on the first GPU run: see BRANCH_REL."""
    from hiptagsearch import synth
    from hiptagsearch.tagger import ConvNeXtTagger
    cfg = dict(synth.CONVNEXT_B_448)
    w = synth.convnext_weights(cfg, seed=0)

    def with_gamma(g):
        return {k: (np.full_like(v, g) if k.endswith(".gamma") else v) for k, v in w.items()}
    w_on, w_off = with_gamma(1e-6), with_gamma(0.0)
    w_fold = dict(w_on)
    for k in w:
        if k.endswith(".gamma"):
            p = k[:-len("gamma")]
            w_fold[p + "mlp.fc2.weight"] = w[p + "mlp.fc2.weight"] * np.float32(1e-6)
            w_fold[p + "mlp.fc2.bias"] = w[p + "mlp.fc2.bias"] * np.float32(1e-6)
            w_fold[k] = np.ones_like(w[k])
    _, x = _inputs(cfg, 1, structured=False)
    x0 = np.ascontiguousarray(x[:1], dtype=np.float32)

    def ref_stream(ww):
        r = convnext_ref.features(convnext_ref.to_torch(ww), torch.from_numpy(x0).double(), cfg["depths"], stop_stage=0)
        return r.permute(0, 2, 3, 1).reshape(1, -1).numpy()
    d_ref = ref_stream(w_on) - ref_stream(w_off)
    assert np.sqrt((d_ref ** 2).mean()) > 1e-7          # the branches are there to be measured
    streams = {}
    for name, ww in (("on", w_on), ("off", w_off), ("fold", w_fold)):
        m = ConvNeXtTagger(cfg, ww, max_batch=1)
        streams[name] = _stream0(m, x0)
        m.close()
    rel = np.linalg.norm((streams["on"] - streams["off"]) - d_ref) / np.linalg.norm(d_ref)
    rel_fold = np.linalg.norm((streams["fold"] - streams["off"]) - d_ref) / np.linalg.norm(d_ref)
    print("B@448 stage-0 branches at gamma 1e-6: relative error %.3e (gamma folded into half fc2: %.3e)" % (rel, rel_fold))
    assert rel <= BRANCH_REL, rel
    assert rel_fold > BRANCH_REL, rel_fold              # the check sees the defect it is there for
