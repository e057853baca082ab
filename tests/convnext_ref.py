"""Float64 CPU restatement of timm's ConvNeXt (convnext_base, conv_mlp = False) from a timm-layout state dict: the oracle of the
ConvNeXt tagger tests.  oracle/ holds no ConvNeXt; tests/test_convnext_host.py pins this restatement to HuggingFace transformers'
independent ConvNextForImageClassification."""
import numpy as np
import torch
import torch.nn.functional as F


def to_torch(w, dtype=torch.float64):
    return {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in w.items()}


def _ln_cl(x, w, b, eps):          # channels-last LayerNorm of an NCHW tensor
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), w, b, eps).permute(0, 3, 1, 2)


def features(w, x, depths, eps=1e-6, stop_stage=None):
    """x: [B, 3, S, S] normalised BGR (the model's input).  Returns the pooled, normalised features [B, dims[3]], or with stop_stage
    the NCHW residual stream after that stage."""
    x = F.conv2d(x, w["stem.0.weight"], w["stem.0.bias"], stride=4)
    x = _ln_cl(x, w["stem.1.weight"], w["stem.1.bias"], eps)
    for i, depth in enumerate(depths):
        if i > 0:
            p = "stages.%d.downsample." % i
            x = F.conv2d(_ln_cl(x, w[p + "0.weight"], w[p + "0.bias"], eps), w[p + "1.weight"], w[p + "1.bias"], stride=2)
        for j in range(depth):
            p = "stages.%d.blocks.%d." % (i, j)
            y = F.conv2d(x, w[p + "conv_dw.weight"], w[p + "conv_dw.bias"], padding=3, groups=x.shape[1])
            y = y.permute(0, 2, 3, 1)
            y = F.layer_norm(y, (y.shape[-1],), w[p + "norm.weight"], w[p + "norm.bias"], eps)
            y = F.gelu(F.linear(y, w[p + "mlp.fc1.weight"], w[p + "mlp.fc1.bias"]))          # exact erf GELU
            y = F.linear(y, w[p + "mlp.fc2.weight"], w[p + "mlp.fc2.bias"]) * w[p + "gamma"]
            x = x + y.permute(0, 3, 1, 2)
        if stop_stage == i:
            return x
    f = x.mean((2, 3))
    return F.layer_norm(f, (f.shape[-1],), w["head.norm.weight"], w["head.norm.bias"], eps)


def forward(w, x, depths, eps=1e-6):
    """(logits, probs) float64 [B, num_classes]."""
    logits = F.linear(features(w, x, depths, eps), w["head.fc.weight"], w["head.fc.bias"])
    return logits, torch.sigmoid(logits)


def preprocess_u8(images_u8, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
    """uint8 [B, S, S, 3] RGB -> float32 [B, 3, S, S] normalised BGR: ToTensor and Normalize in float32, then the channel flip."""
    x = torch.from_numpy(np.ascontiguousarray(images_u8)).permute(0, 3, 1, 2).to(torch.float32) / 255.0
    x = (x - torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)) / torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1)
    return x.flip(1).contiguous()


def hf_state_dict(w, depths):
    """The timm-layout dict in transformers' ConvNextForImageClassification naming (one-to-one)."""
    sd = {"convnext.embeddings.patch_embeddings.weight": w["stem.0.weight"], "convnext.embeddings.patch_embeddings.bias": w["stem.0.bias"],
          "convnext.embeddings.layernorm.weight": w["stem.1.weight"], "convnext.embeddings.layernorm.bias": w["stem.1.bias"],
          "convnext.layernorm.weight": w["head.norm.weight"], "convnext.layernorm.bias": w["head.norm.bias"],
          "classifier.weight": w["head.fc.weight"], "classifier.bias": w["head.fc.bias"]}
    for i, depth in enumerate(depths):
        q = "convnext.encoder.stages.%d." % i
        if i > 0:
            for k in ("0", "1"):
                for t in ("weight", "bias"):
                    sd[q + "downsampling_layer.%s.%s" % (k, t)] = w["stages.%d.downsample.%s.%s" % (i, k, t)]
        for j in range(depth):
            p, r = "stages.%d.blocks.%d." % (i, j), q + "layers.%d." % j
            for a, b in (("conv_dw", "dwconv"), ("norm", "layernorm"), ("mlp.fc1", "pwconv1"), ("mlp.fc2", "pwconv2")):
                for t in ("weight", "bias"):
                    sd[r + "%s.%s" % (b, t)] = w[p + "%s.%s" % (a, t)]
            sd[r + "layer_scale_parameter"] = w[p + "gamma"]
    return sd
