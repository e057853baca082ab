#!/usr/bin/env python3
"""Development aid: SwinV2-B @448 tagger (window 14) images/s and TFLOP/s at batch 10 / 32 / 64 (device input, device output; GPU only)."""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "anime-illust-image-searcher_amd"))
import numpy as np, torch
from hiptagsearch import synth
from hiptagsearch.tagger import SwinV2Tagger
cfg = dict(synth.SWINV2_B_448)
w = synth.swinv2_weights(cfg, seed=0)
PEAK = 2.5e15          # MI355X dense 16-bit MFMA peak, FLOP/s
for B in (10, 32, 64):
    m = SwinV2Tagger(cfg, w, max_batch=B)
    imgs = torch.randint(0, 256, (B, 448, 448, 3), dtype=torch.uint8, device="cuda")
    probs = torch.empty((B, cfg["num_classes"]), dtype=torch.float32, device="cuda")
    for _ in range(3): m.forward_u8(imgs, probs=probs, want="probs")
    torch.cuda.synchronize(); t0 = time.perf_counter()
    n = 12
    for _ in range(n): m.forward_u8(imgs, probs=probs, want="probs")
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / n
    fl = m.flops_per_image()
    print("batch %d: %.2f ms  %.0f images/s  %.1f TFLOP/s = %.3f of peak (%.2f GFLOP/img)" % (B, dt * 1e3, B / dt, B * fl / dt / 1e12,
                                                                                         B * fl / dt / PEAK, fl / 1e9))
    m.close()
