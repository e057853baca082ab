"""SwinV2 tagger, the parts that need no GPU: the float64 restatement (tests/swinv2_ref.py) against transformers'
Swinv2ForImageClassification, the synthetic checkpoint's key layout, the exported ABI and configuration structure, and the Predictor's
model dispatch."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "anime-illust-image-searcher_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import swinv2_ref  # noqa: E402

# a second geometry: window 8 on sides 32 / 16 / 8 / 4 -- two shifted stages, one whose side equals the window, one smaller than it
SMALL_W8 = dict(image_size=128, patch=4, window=8, dims=(64, 128, 256, 512), depths=(2, 2, 2, 1), heads=(2, 4, 8, 16), mlp_ratio=4,
                num_classes=50, ln_eps=1e-5, gelu_tanh=0, cpb_pretrained_window=0, norm_mean=(0.5, 0.5, 0.5), norm_std=(0.5, 0.5, 0.5),
                operand_f16=1)


# timm swinv2_base_window8_256 (img_size 448, window_size 14), num_classes = 10861: every key and shape of its state_dict (>= 0.9 layout,
# persistent entries only)
def _timm_swinv2_base_shapes(num_classes=10861):
    dims, depths, heads = (128, 256, 512, 1024), (2, 2, 18, 2), (4, 8, 16, 32)
    s = {"patch_embed.proj.weight": (128, 3, 4, 4), "patch_embed.proj.bias": (128,), "patch_embed.norm.weight": (128,),
         "patch_embed.norm.bias": (128,)}
    for i in range(4):
        d = dims[i]
        if i:
            s["layers.%d.downsample.reduction.weight" % i] = (d, 4 * dims[i - 1])
            s["layers.%d.downsample.norm.weight" % i] = s["layers.%d.downsample.norm.bias" % i] = (d,)
        for j in range(depths[i]):
            p = "layers.%d.blocks.%d." % (i, j)
            s.update({p + "attn.logit_scale": (heads[i], 1, 1), p + "attn.q_bias": (d,), p + "attn.v_bias": (d,),
                      p + "attn.cpb_mlp.0.weight": (512, 2), p + "attn.cpb_mlp.0.bias": (512,), p + "attn.cpb_mlp.2.weight": (heads[i], 512),
                      p + "attn.qkv.weight": (3 * d, d), p + "attn.proj.weight": (d, d), p + "attn.proj.bias": (d,),
                      p + "norm1.weight": (d,), p + "norm1.bias": (d,), p + "mlp.fc1.weight": (4 * d, d), p + "mlp.fc1.bias": (4 * d,),
                      p + "mlp.fc2.weight": (d, 4 * d), p + "mlp.fc2.bias": (d,), p + "norm2.weight": (d,), p + "norm2.bias": (d,)})
    s.update({"norm.weight": (1024,), "norm.bias": (1024,), "head.fc.weight": (num_classes, 1024), "head.fc.bias": (num_classes,)})
    return s


@pytest.mark.parametrize("geometry", ["tiny", "w8"])
def test_restatement_matches_transformers(geometry):
    """The restatement and transformers' Swinv2 (loaded through the key mapping of swinv2_ref.hf_state_dict) agree to float32 rounding."""
    transformers = pytest.importorskip("transformers")
    from hiptagsearch import synth
    cfg = dict(synth.SWINV2_TINY) if geometry == "tiny" else dict(SMALL_W8)
    w = synth.swinv2_weights(cfg, seed=5, trained_like=True)
    hf = transformers.Swinv2ForImageClassification(transformers.Swinv2Config(
        image_size=cfg["image_size"], patch_size=cfg["patch"], num_channels=3, embed_dim=cfg["dims"][0], depths=list(cfg["depths"]),
        num_heads=list(cfg["heads"]), window_size=cfg["window"], pretrained_window_sizes=[0, 0, 0, 0], mlp_ratio=float(cfg["mlp_ratio"]),
        qkv_bias=True, hidden_act="gelu", layer_norm_eps=cfg["ln_eps"], drop_path_rate=0.0, hidden_dropout_prob=0.0,
        attention_probs_dropout_prob=0.0, use_absolute_embeddings=False, num_labels=cfg["num_classes"])).eval()
    hf.load_state_dict(swinv2_ref.hf_state_dict(swinv2_ref.to_torch(w, torch.float32), cfg["depths"]), strict=True)
    x = swinv2_ref.preprocess_u8(synth.images_u8(2, cfg["image_size"], seed=11))
    with torch.no_grad():
        got = hf(pixel_values=x).logits.double()
        ref, _ = swinv2_ref.forward(swinv2_ref.to_torch(w), x.double(), cfg)
    scale = ref.abs().max().item()
    assert scale > 1.0
    assert (got - ref).abs().max().item() <= 2e-5 * scale


def test_restatement_mask_and_clamp_matter():
    """The -100 mask and the logit-scale clamp are not inert in the restatement: on masked_keys_win_qkv, -inf in place of -100 changes
    the attention output (the GPU tests' negative control relies on it), and so does dropping the clamp at ln 100."""
    side, w, nh = 14, 7, 2
    q, k, v = swinv2_ref.masked_keys_win_qkv(1, side, w, w // 2, nh, seed=3)
    ls = torch.tensor([np.log(100.0), np.log(150.0)], dtype=torch.float64)
    cpb = 16 * torch.sigmoid(torch.randn(nh, (2 * w - 1) ** 2, generator=torch.Generator().manual_seed(4), dtype=torch.float64))
    a = swinv2_ref.window_attention(q, k, v, ls, cpb, side, w, w // 2)
    b = swinv2_ref.window_attention(q, k, v, ls, cpb, side, w, w // 2, mask_value=-float("inf"))
    assert (a - b).abs().max().item() > 0.1
    assert swinv2_ref.raster_regions(side, w, w // 2).unique().numel() == 9
    # the clamp: head 1 (ln 150) equals head 1 at exactly ln 100; head 0 at ln 150 without the clamp would differ
    c = swinv2_ref.window_attention(q, k, v, torch.full_like(ls, np.log(100.0)), cpb, side, w, w // 2)
    assert (a - c).abs().max().item() < 1e-12
    d = swinv2_ref.window_attention(q, k, v, ls, cpb, side, w, 0)
    assert (a - d).abs().max().item() > 0.1                 # the shift matters


def test_synthetic_checkpoint_has_timm_swinv2_base_layout():
    from hiptagsearch import synth
    w = synth.swinv2_weights(synth.SWINV2_B_448)
    want = _timm_swinv2_base_shapes()
    assert set(w) == set(want)
    assert all(tuple(w[k].shape) == v for k, v in want.items())
    assert all(v.dtype == np.float32 for v in w.values())


def test_trained_like_logit_scales_and_position_bias():
    from hiptagsearch import synth
    cfg = synth.SWINV2_B_448
    w = synth.swinv2_weights(cfg, trained_like=True)
    ls = np.concatenate([v.reshape(-1) for k, v in w.items() if k.endswith("logit_scale")])
    assert ls.min() >= np.log(10.0) - 1e-6 and ls.max() > np.log(100.0)
    assert (ls > np.log(100.0)).sum() >= sum(cfg["depths"])                   # some heads of every block above the clamp
    p = "layers.2.blocks.1.attn."
    t = swinv2_ref.cpb_table(*(torch.from_numpy(w[p + k]).double() for k in ("cpb_mlp.0.weight", "cpb_mlp.0.bias", "cpb_mlp.2.weight")), 14)
    assert t.shape == (16, 27 * 27)
    assert t.std().item() > 1.0 and t.min().item() > 0.05 and t.max().item() < 15.95          # spread, not saturated


def test_library_exports_swinv2_entry_points():
    from hiptagsearch import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in ("create", "destroy", "set_tensor", "forward_u8", "forward_f32", "flops_per_image"):
        assert "hipts_swinv2_" + name in exported
        assert "hipts_swinv2_" + name in _lib.EXPORTED_SYMBOLS
    assert "hiptsdbg_swinv2_stream" in exported and "hiptsdbg_swinv2_window_attention" in exported


def _header_fields(name):
    text = open(os.path.join(ROOT, "include", "hip_tagsearch.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\}" % name, text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(t, f, int(n) if n else 1) for t, f, n in re.findall(r"(int32_t|float)\s+(\w+)(?:\[(\d+)\])?;", body)]


def test_swinv2_config_layout_matches_header_library_and_docs():
    """hipts_sizeof_config(4) = the ctypes structure = the INTEGRATION.md stub = the header, field by field."""
    from hiptagsearch import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.hipts_sizeof_config.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]
    cmap = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    ns = {"ctypes": ctypes}
    m = re.search(r"^class SwinCfg\(ctypes\.Structure\):.*?\n(?=\S)", doc, flags=re.S | re.M)
    assert m
    exec(m.group(0), ns)
    fields = _header_fields("hipts_swinv2_config")
    assert [f for _, f, _ in fields] == ["image_size", "patch", "window", "dims", "depths", "heads", "mlp_ratio", "num_classes", "ln_eps",
                                         "gelu_tanh", "cpb_pretrained_window", "norm_mean", "norm_std", "max_batch", "operand_f16"]
    want = [(f, cmap[t] if n == 1 else cmap[t] * n) for t, f, n in fields]
    for st in (_lib.Swinv2Config, ns["SwinCfg"]):
        got = list(st._fields_)
        assert [f for f, _ in got] == [f for f, _ in want]
        assert all(ctypes.sizeof(a) == ctypes.sizeof(b) and a._type_ == b._type_ for (_, a), (_, b) in zip(got, want))
    n = ctypes.c_size_t(0)
    assert lib.hipts_sizeof_config(4, ctypes.byref(n)) == 0
    assert n.value == ctypes.sizeof(_lib.Swinv2Config) == ctypes.sizeof(ns["SwinCfg"]) == sum(4 * k for _, _, k in fields)
    assert lib.hipts_sizeof_config(7, ctypes.byref(n)) != 0


def test_predictor_dispatch():
    from hiptagsearch import synth, tagger
    assert tagger.model_class(synth.SWINV2_B_448) is tagger.SwinV2Tagger
    assert tagger.model_class(synth.SWINV2_TINY) is tagger.SwinV2Tagger
    assert tagger.model_class(synth.CONVNEXT_B_448) is tagger.ConvNeXtTagger
    assert tagger.model_class(synth.VIT_B16_448) is tagger.ViTTagger
    assert tagger.model_class(synth.EVA02_L14_448) is tagger.EvaTagger


def test_precise_is_refused_for_swinv2():
    from hiptagsearch import synth, tagger
    p = tagger.Predictor(precise=True)
    with pytest.raises(ValueError, match="attention"):
        p.load_model(cfg=synth.SWINV2_TINY)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "anime-illust-image-searcher_amd", "tagging.py"), "--dir", ROOT, "--model",
                        "swinv2-tiny", "--precise"], capture_output=True, text=True)
    assert r.returncode == 2 and "attention" in r.stderr

