"""ConvNeXt tagger, the parts that need no GPU: the float64 restatement (tests/convnext_ref.py) against transformers'
ConvNextForImageClassification, the synthetic checkpoint's key layout, the exported ABI and configuration structure, and the
Predictor's model dispatch."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "anime-illust-image-searcher_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import convnext_ref  # noqa: E402

# timm convnext_base (conv_mlp = False), num_classes = 10861: every key and shape of its state_dict
def _timm_convnext_base_shapes(num_classes=10861):
    dims, depths = (128, 256, 512, 1024), (3, 3, 27, 3)
    s = {"stem.0.weight": (128, 3, 4, 4), "stem.0.bias": (128,), "stem.1.weight": (128,), "stem.1.bias": (128,)}
    for i in range(4):
        if i:
            s["stages.%d.downsample.0.weight" % i] = s["stages.%d.downsample.0.bias" % i] = (dims[i - 1],)
            s["stages.%d.downsample.1.weight" % i] = (dims[i], dims[i - 1], 2, 2)
            s["stages.%d.downsample.1.bias" % i] = (dims[i],)
        for j in range(depths[i]):
            p, d = "stages.%d.blocks.%d." % (i, j), dims[i]
            s.update({p + "gamma": (d,), p + "conv_dw.weight": (d, 1, 7, 7), p + "conv_dw.bias": (d,), p + "norm.weight": (d,),
                      p + "norm.bias": (d,), p + "mlp.fc1.weight": (4 * d, d), p + "mlp.fc1.bias": (4 * d,), p + "mlp.fc2.weight": (d, 4 * d),
                      p + "mlp.fc2.bias": (d,)})
    s.update({"head.norm.weight": (1024,), "head.norm.bias": (1024,), "head.fc.weight": (num_classes, 1024), "head.fc.bias": (num_classes,)})
    return s


@pytest.mark.parametrize("depths", [None, (3, 3, 3, 3)])
def test_restatement_matches_transformers(depths):
    """The restatement and transformers' ConvNeXt (loaded through the one-to-one key mapping) agree to float32 rounding."""
    transformers = pytest.importorskip("transformers")
    from hiptagsearch import synth
    cfg = dict(synth.CONVNEXT_TINY)
    if depths:
        cfg["depths"] = depths
    w = synth.convnext_weights(cfg, seed=5, trained_like=True)
    hf = transformers.ConvNextForImageClassification(transformers.ConvNextConfig(
        num_channels=3, patch_size=4, num_stages=4, hidden_sizes=list(cfg["dims"]), depths=list(cfg["depths"]), hidden_act="gelu",
        layer_norm_eps=cfg["ln_eps"], drop_path_rate=0.0, num_labels=cfg["num_classes"], image_size=cfg["image_size"])).eval()
    hf.load_state_dict(convnext_ref.hf_state_dict(convnext_ref.to_torch(w, torch.float32), cfg["depths"]), strict=True)
    x = convnext_ref.preprocess_u8(synth.images_u8(3, cfg["image_size"], seed=11))
    with torch.no_grad():
        got = hf(pixel_values=x).logits.double()
    ref, _ = convnext_ref.forward(convnext_ref.to_torch(w), x.double(), cfg["depths"], cfg["ln_eps"])
    scale = ref.abs().max().item()
    assert scale > 1.0
    assert (got - ref).abs().max().item() <= 2e-5 * scale


def test_synthetic_checkpoint_has_timm_convnext_base_layout():
    from hiptagsearch import synth
    w = synth.convnext_weights(synth.CONVNEXT_B_448)
    want = _timm_convnext_base_shapes()
    assert set(w) == set(want)
    assert all(tuple(w[k].shape) == v for k, v in want.items())
    assert all(v.dtype == np.float32 for v in w.values())


def test_trained_like_layer_scales():
    from hiptagsearch import synth
    w = synth.convnext_weights(synth.CONVNEXT_B_448, trained_like=True)
    g = np.concatenate([v for k, v in w.items() if k.endswith(".gamma")])
    assert g.min() >= 1e-6 * 0.999 and g.max() <= 1.0
    assert np.all(w["stages.2.blocks.0.gamma"] == np.float32(1e-6))          # a block left at timm's initial value
    assert np.log10(g[g > 1e-5]).std() > 0.8                                  # spread over orders of magnitude


def test_library_exports_convnext_entry_points():
    import subprocess
    from hiptagsearch import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in ("create", "destroy", "set_tensor", "forward_u8", "forward_f32", "flops_per_image"):
        assert "hipts_convnext_" + name in exported
        assert "hipts_convnext_" + name in _lib.EXPORTED_SYMBOLS
    assert "hiptsdbg_convnext_stream" in exported


def _header_fields(name):
    text = open(os.path.join(ROOT, "include", "hip_tagsearch.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\}" % name, text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for t, f, n in re.findall(r"(int32_t|float)\s+(\w+)(?:\[(\d+)\])?;", body):
        out.append((t, f, int(n) if n else 1))
    return out


def test_convnext_config_layout_matches_header_library_and_docs():
    """hipts_sizeof_config(3) = the ctypes structure = the INTEGRATION.md stub = the header, field by field."""
    from hiptagsearch import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.hipts_sizeof_config.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]
    cmap = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    ns = {"ctypes": ctypes}
    m = re.search(r"^class ConvnextCfg\(ctypes\.Structure\):.*?\n(?=\S)", doc, flags=re.S | re.M)
    assert m
    exec(m.group(0), ns)
    fields = _header_fields("hipts_convnext_config")
    assert [f for _, f, _ in fields] == ["image_size", "dims", "depths", "num_classes", "ln_eps", "norm_mean", "norm_std", "max_batch",
                                         "operand_f16"]
    want = [(f, cmap[t] if n == 1 else cmap[t] * n) for t, f, n in fields]
    for st in (_lib.ConvnextConfig, ns["ConvnextCfg"]):
        got = list(st._fields_)
        assert [f for f, _ in got] == [f for f, _ in want]
        assert all(ctypes.sizeof(a) == ctypes.sizeof(b) and a._type_ == b._type_ for (_, a), (_, b) in zip(got, want))
    n = ctypes.c_size_t(0)
    assert lib.hipts_sizeof_config(3, ctypes.byref(n)) == 0
    assert n.value == ctypes.sizeof(_lib.ConvnextConfig) == ctypes.sizeof(ns["ConvnextCfg"]) == sum(4 * k for _, _, k in fields)
    assert lib.hipts_sizeof_config(7, ctypes.byref(n)) != 0


def test_predictor_dispatch():
    from hiptagsearch import synth, tagger
    assert tagger.model_class(synth.CONVNEXT_B_448) is tagger.ConvNeXtTagger
    assert tagger.model_class(synth.CONVNEXT_TINY) is tagger.ConvNeXtTagger
    assert tagger.model_class(synth.VIT_B16_448) is tagger.ViTTagger
    assert tagger.model_class(synth.VIT_TINY) is tagger.ViTTagger
    assert tagger.model_class(synth.EVA02_L14_448) is tagger.EvaTagger
    assert tagger.model_class(synth.EVA02_TINY) is tagger.EvaTagger


def test_precise_is_refused_for_convnext():
    from hiptagsearch import synth, tagger
    p = tagger.Predictor(precise=True)
    with pytest.raises(ValueError, match="attention"):
        p.load_model(cfg=synth.CONVNEXT_TINY)
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "anime-illust-image-searcher_amd", "tagging.py"), "--dir", ROOT, "--model",
                        "convnext-tiny", "--precise"], capture_output=True, text=True)
    assert r.returncode == 2 and "attention" in r.stderr
