#!/usr/bin/env python3
"""Where a checkpoint sits in the folded LayerNorm's accuracy table ("The folded LayerNorm"): one image through the
trained-like ViT-B/16 (12 layers) and its 1-, 2-, 4- and 8-layer prefixes, and per run the largest |mean| / sigma and max |gamma x| over the rows of
the residual stream (hiptsdbg_vit_dump "x": the blocked stream after the last layer's attention residual, un-blocked with x_index)."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "anime-illust-image-searcher_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gemm_epi_ref as R  # noqa: E402
from hiptagsearch import _lib, synth  # noqa: E402
from hiptagsearch.tagger import ViTTagger  # noqa: E402


def main():
    lib = _lib.load()
    dump = lib.hiptsdbg_vit_dump
    dump.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    full = dict(synth.VIT_B16_448)
    w_full = synth.vit_weights(full, seed=0, trained_like=True)
    T, D = 784, full["dim"]
    for kind, imgs in (("noise", synth.images_u8(1, 448, seed=5)), ("structured[0]", synth.structured_images_u8(448, seed=77)[:1])):
        for depth in (1, 2, 4, 8, 12):
            cfg = dict(full, depth=depth)
            w = {k: v for k, v in w_full.items() if not k.startswith("blocks.") or int(k.split(".")[1]) < depth}
            model = ViTTagger(cfg, w, max_batch=1)
            logits, _ = model.forward_u8(imgs)
            buf = np.empty(T * D * 4 + 4096, np.uint8)
            nb = ctypes.c_size_t()
            assert dump(model._h, b"x", buf.ctypes.data, buf.nbytes, ctypes.byref(nb)) == 0, _lib.last_error()
            raw = buf[:nb.value].view(np.float32)
            x = raw[R.x_index(T, D, D, 1)].astype(np.float64)          # the blocked stream: after the last layer's attention residual
            gamma = w["blocks.%d.norm2.weight" % (depth - 1)].astype(np.float64)
            ms = np.abs(x.mean(1)) / x.std(1)
            print("%-13s depth %2d: bytes %d  finite %s  max |mean|/sigma %.3f (median %.3f)  max |gamma x| %.2f  max |x| %.2f  sigma range %.3f .. %.3f" % (
                kind, depth, nb.value, np.isfinite(x).all(), ms.max(), np.median(ms), np.abs(x * gamma[None, :]).max(), np.abs(x).max(), x.std(1).min(),
                x.std(1).max()), flush=True)
            model.close()


if __name__ == "__main__":
    main()
