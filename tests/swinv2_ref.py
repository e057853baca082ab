"""Float64 CPU restatement of timm's SwinTransformerV2 (swin_transformer_v2.py, >= 0.9 key layout) from a timm-layout state dict: the
oracle of the SwinV2 tagger tests.  oracle/ holds no SwinV2; tests/test_swinv2_host.py pins this restatement to HuggingFace
transformers' independent Swinv2ForImageClassification."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from convnext_ref import preprocess_u8, to_torch  # noqa: F401  (same transform and dtype helper as the ConvNeXt tagger)


def stage_geometry(cfg):
    """[(side, window, dims, heads)] per stage: a stage whose side is <= window attends over the whole map, unshifted."""
    out, H = [], cfg["image_size"] // cfg.get("patch", 4)
    for i in range(4):
        if i:
            H //= 2
        out.append((H, min(H, cfg["window"]), cfg["dims"][i], cfg["heads"][i]))
    return out


def block_shift(cfg, stage, j):
    H, w, _, _ = stage_geometry(cfg)[stage]
    return 0 if (j % 2 == 0 or H <= cfg["window"]) else cfg["window"] // 2


def cpb_table(w1, b1, w2, window, pretrained_window=0):
    """16 sigmoid(cpb_mlp(table)) as [heads, (2w-1)^2], rows of the table in (dy, dx) order, dy and dx = query minus key offsets."""
    r = torch.arange(-(window - 1), window, dtype=torch.float64)
    t = torch.stack(torch.meshgrid(r, r, indexing="ij"), dim=-1)                 # [2w-1, 2w-1, 2]
    t = t / ((pretrained_window if pretrained_window > 0 else window) - 1) * 8.0
    t = torch.sign(t) * torch.log2(t.abs() + 1.0) / math.log2(8)
    hid = F.relu(F.linear(t.reshape(-1, 2), w1, b1))
    return (16.0 * torch.sigmoid(F.linear(hid, w2))).t().contiguous()


def window_attention(q, k, v, logit_scale, cpb, side, window, shift, mask_value=-100.0):
    """q, k, v: [B, side*side, heads*32] raster order (q, k before F.normalize), logit_scale [heads] (before the clamp), cpb
    [heads, (2w-1)^2].  Returns [B, side*side, heads*32]: roll by -shift, window partition, attention, reverse.  mask_value: what is
    added between tokens of different roll regions (timm: -100)."""
    B, N, C = q.shape
    nh = C // 32
    w, H = window, side

    def part(x):                    # [B, H*H, C] -> [B*nW, heads, w*w, 32]
        x = x.reshape(B, H, H, C)
        if shift:
            x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
        x = x.reshape(B, H // w, w, H // w, w, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, w * w, nh, 32)
        return x.permute(0, 2, 1, 3)
    qw, kw, vw = part(q), part(k), part(v)
    attn = F.normalize(qw, dim=-1) @ F.normalize(kw, dim=-1).transpose(-2, -1)
    attn = attn * torch.clamp(logit_scale.reshape(nh, 1, 1), max=math.log(1.0 / 0.01)).exp()
    coords = torch.stack(torch.meshgrid(torch.arange(w), torch.arange(w), indexing="ij")).flatten(1)   # [2, T]
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0) + (w - 1)
    idx = rel[..., 0] * (2 * w - 1) + rel[..., 1]
    attn = attn + cpb[:, idx].unsqueeze(0)
    if shift:
        img = torch.zeros(H, H)
        cnt = 0
        for hs in ((0, -w), (-w, -shift), (-shift, None)):
            for ws in ((0, -w), (-w, -shift), (-shift, None)):
                img[slice(*hs), slice(*ws)] = cnt
                cnt += 1
        mw = img.reshape(H // w, w, H // w, w).permute(0, 2, 1, 3).reshape(-1, w * w)
        diff = (mw.unsqueeze(1) - mw.unsqueeze(2)) != 0                            # [nW, T, T]
        mask = torch.zeros(diff.shape, dtype=attn.dtype).masked_fill(diff, mask_value)
        nW = mask.shape[0]
        attn = (attn.reshape(B, nW, nh, w * w, w * w) + mask.unsqueeze(1).unsqueeze(0)).reshape(-1, nh, w * w, w * w)
    o = torch.softmax(attn, dim=-1) @ vw                                           # [B*nW, heads, T, 32]
    o = o.permute(0, 2, 1, 3).reshape(B, H // w, H // w, w, w, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, H, C)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o.reshape(B, N, C)


def raster_regions(side, window, shift):
    """The roll region (0..8, timm's attn_mask slices of the rolled image) of every raster token, [side*side]."""
    img = torch.zeros(side, side, dtype=torch.int64)
    cnt = 0
    for hs in ((0, -window), (-window, -shift), (-shift, None)):
        for ws in ((0, -window), (-window, -shift), (-shift, None)):
            img[slice(*hs), slice(*ws)] = cnt
            cnt += 1
    return torch.roll(img, shifts=(shift, shift), dims=(0, 1)).reshape(-1)


def masked_keys_win_qkv(batch, side, window, shift, heads, seed=0):
    """q, k, v [batch, side*side, heads*32] float64 for which the -100 mask decides the output: every query q = +-u (the sign by the
    parity of its roll region) and its key k = -q, plus a little noise.  Inside a region the cosine is -1; a key of a region of the other
    parity has cosine +1 and, at a logit scale of 100, still outscores the region's own keys by ~100 after the -100 mask -- with -inf in
    its place it would get no weight at all."""
    g = torch.Generator().manual_seed(seed)
    C = 32 * heads
    u = torch.randn(C, generator=g, dtype=torch.float64)
    sgn = (1.0 - 2.0 * (raster_regions(side, window, shift) % 2).to(torch.float64)).reshape(1, -1, 1)
    q = sgn * u + 0.05 * torch.randn(batch, side * side, C, generator=g, dtype=torch.float64)
    k = -sgn * u + 0.05 * torch.randn(batch, side * side, C, generator=g, dtype=torch.float64)
    v = torch.randn(batch, side * side, C, generator=g, dtype=torch.float64)
    return q, k, v


def features(w, x, cfg, stop_stage=None):
    """x: [B, 3, S, S] normalised BGR (the model's input).  Returns the pooled features [B, dims[3]] (LayerNorm per token, then the
    mean), or with stop_stage the residual stream [B, H*H, C] after that stage."""
    eps = cfg["ln_eps"]
    gelu = (lambda t: F.gelu(t, approximate="tanh")) if cfg.get("gelu_tanh", 0) else F.gelu
    x = F.conv2d(x, w["patch_embed.proj.weight"], w["patch_embed.proj.bias"], stride=cfg.get("patch", 4))
    B = x.shape[0]
    x = x.permute(0, 2, 3, 1)
    x = F.layer_norm(x, (x.shape[-1],), w["patch_embed.norm.weight"], w["patch_embed.norm.bias"], eps).reshape(B, -1, x.shape[-1])
    for i, (H, win, C, nh) in enumerate(stage_geometry(cfg)):
        if i > 0:
            p = "layers.%d.downsample." % i
            xs = x.reshape(B, H, 2, H, 2, -1).permute(0, 1, 3, 4, 2, 5).reshape(B, H * H, -1)      # timm's (dx, dy, c) order
            x = F.layer_norm(F.linear(xs, w[p + "reduction.weight"]), (C,), w[p + "norm.weight"], w[p + "norm.bias"], eps)
        for j in range(cfg["depths"][i]):
            p = "layers.%d.blocks.%d." % (i, j)
            qkv_b = torch.cat([w[p + "attn.q_bias"], torch.zeros_like(w[p + "attn.q_bias"]), w[p + "attn.v_bias"]])
            qkv = F.linear(x, w[p + "attn.qkv.weight"], qkv_b)
            cpb = cpb_table(w[p + "attn.cpb_mlp.0.weight"], w[p + "attn.cpb_mlp.0.bias"], w[p + "attn.cpb_mlp.2.weight"], win,
                            cfg.get("cpb_pretrained_window", 0))
            a = window_attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], w[p + "attn.logit_scale"].reshape(-1), cpb, H, win,
                                 block_shift(cfg, i, j))
            a = F.linear(a, w[p + "attn.proj.weight"], w[p + "attn.proj.bias"])
            x = x + F.layer_norm(a, (C,), w[p + "norm1.weight"], w[p + "norm1.bias"], eps)
            y = F.linear(gelu(F.linear(x, w[p + "mlp.fc1.weight"], w[p + "mlp.fc1.bias"])), w[p + "mlp.fc2.weight"], w[p + "mlp.fc2.bias"])
            x = x + F.layer_norm(y, (C,), w[p + "norm2.weight"], w[p + "norm2.bias"], eps)
        if stop_stage == i:
            return x
    x = F.layer_norm(x, (x.shape[-1],), w["norm.weight"], w["norm.bias"], eps)
    return x.mean(1)


def forward(w, x, cfg):
    """(logits, probs) float64 [B, num_classes]."""
    logits = F.linear(features(w, x, cfg), w["head.fc.weight"], w["head.fc.bias"])
    return logits, torch.sigmoid(logits)


def hf_state_dict(w, depths):
    """The timm-layout dict in transformers' Swinv2ForImageClassification naming: qkv split into query / key / value (key without
    bias), q_bias / v_bias as the query / value biases, cpb_mlp as continuous_position_bias_mlp, norm1 / norm2 as layernorm_before /
    layernorm_after, and timm's layers.{i}.downsample (start of stage i) as HF's encoder.layers.{i-1}.downsample (end of stage i-1)."""
    sd = {"swinv2.embeddings.patch_embeddings.projection.weight": w["patch_embed.proj.weight"],
          "swinv2.embeddings.patch_embeddings.projection.bias": w["patch_embed.proj.bias"],
          "swinv2.embeddings.norm.weight": w["patch_embed.norm.weight"], "swinv2.embeddings.norm.bias": w["patch_embed.norm.bias"],
          "swinv2.layernorm.weight": w["norm.weight"], "swinv2.layernorm.bias": w["norm.bias"],
          "classifier.weight": w["head.fc.weight"], "classifier.bias": w["head.fc.bias"]}
    for i, depth in enumerate(depths):
        if i > 0:
            q = "swinv2.encoder.layers.%d.downsample." % (i - 1)
            sd[q + "reduction.weight"] = w["layers.%d.downsample.reduction.weight" % i]
            sd[q + "norm.weight"] = w["layers.%d.downsample.norm.weight" % i]
            sd[q + "norm.bias"] = w["layers.%d.downsample.norm.bias" % i]
        for j in range(depth):
            p, r = "layers.%d.blocks.%d." % (i, j), "swinv2.encoder.layers.%d.blocks.%d." % (i, j)
            qkv = w[p + "attn.qkv.weight"]
            C = qkv.shape[1]
            a = r + "attention.self."
            sd[a + "query.weight"], sd[a + "key.weight"], sd[a + "value.weight"] = qkv[:C], qkv[C:2 * C], qkv[2 * C:]
            sd[a + "query.bias"], sd[a + "value.bias"] = w[p + "attn.q_bias"], w[p + "attn.v_bias"]
            sd[a + "logit_scale"] = w[p + "attn.logit_scale"]
            for t in ("0.weight", "0.bias", "2.weight"):
                sd[a + "continuous_position_bias_mlp." + t] = w[p + "attn.cpb_mlp." + t]
            sd[r + "attention.output.dense.weight"] = w[p + "attn.proj.weight"]
            sd[r + "attention.output.dense.bias"] = w[p + "attn.proj.bias"]
            for a_, b_ in (("norm1", "layernorm_before"), ("norm2", "layernorm_after"), ("mlp.fc1", "intermediate.dense"),
                           ("mlp.fc2", "output.dense")):
                for t in ("weight", "bias"):
                    sd[r + "%s.%s" % (b_, t)] = w[p + "%s.%s" % (a_, t)]
    return sd
