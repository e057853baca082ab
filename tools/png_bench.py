#!/usr/bin/env python3
"""Development aid (needs the GPU): device time of the hybrid PNG decode per batch -- hipts_decode_batch_u8 over 64 scanline slots of a
1024 x 768 PNG (RGB, then RGBA) against hipts_resize_batch_u8 over the same images already decoded (what the Pillow workers hand over).
Under `rocprofv3 --kernel-trace --stats` the line of png_unfilter_kernel is the kernel alone (one launch per batch)."""
import io, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "anime-illust-image-searcher_amd"))
import numpy as np
import torch
from PIL import Image
from hiptagsearch import _lib, png_host

N, S = 64, 448
s = torch.cuda.current_stream().cuda_stream
for c in (3, 4):
    rng = np.random.default_rng(3)
    small = rng.integers(0, 256, (24, 32, c), dtype=np.uint8)
    big = np.stack([np.asarray(Image.fromarray(small[:, :, k]).resize((1024, 768), Image.BICUBIC)) for k in range(c)], axis=2)
    a = np.clip(big.astype(np.int16) + rng.integers(-8, 9, (768, 1024, c), dtype=np.int16), 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(a, "RGBA" if c == 4 else "RGB").save(buf, "PNG")
    data = buf.getvalue()
    img = Image.open(io.BytesIO(data))
    if c == 4:
        bg = Image.new("RGB", img.size, (255, 255, 255))
        bg.paste(img, mask=img.split()[-1])
        img = bg
    img = np.asarray(img)
    stride = png_host.slot_bytes(1024, 768, 4) + 64
    slots = torch.empty((N, stride), dtype=torch.uint8).pin_memory()
    raw = torch.empty((N, stride), dtype=torch.uint8).pin_memory()
    t0 = time.perf_counter()
    for i in range(N):
        assert png_host.png_inflate_into(data, slots[i].numpy()) == 0
    t_inflate = (time.perf_counter() - t0) / N
    for i in range(N):
        raw[i, :img.size] = torch.from_numpy(img.reshape(-1).copy())
    filters = np.bincount(slots[0].numpy()[1024:1024 + 768 * (1 + 1024 * c)].reshape(768, -1)[:, 0], minlength=5)
    kinds = np.full(N, 2, np.int32)
    hw = np.ascontiguousarray(np.tile(np.asarray([[768, 1024]], np.int32), (N, 1)))
    out = torch.empty((N, S, S, 3), dtype=torch.uint8, device="cuda")
    ref = torch.empty_like(out)

    def run_png():
        _lib.call("hipts_decode_batch_u8", slots.data_ptr(), stride, _lib.ptr(kinds), _lib.ptr(hw), N, 1, _lib.ptr(out), S, 3, 0, s)

    def run_raw():
        _lib.call("hipts_resize_batch_u8", raw.data_ptr(), _lib.HOST, stride, _lib.ptr(hw), N, 1, _lib.ptr(ref), S, 3, 0, s)

    print("%s 1024 x 768, %.2f MB, rows by filter type %s; host half %.1f ms per file on one core" % ("RGBA" if c == 4 else "RGB", len(data) / 1e6, filters.tolist(), 1e3 * t_inflate))
    for name, fn in (("hybrid decode + pad + resize", run_png), ("pad + resize of decoded images", run_raw)):
        fn(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(10):
            fn()
        e1.record()
        t_host = (time.perf_counter() - t0) / 10
        torch.cuda.synchronize()
        print("  %-34s %.2f ms per batch of %d on the device (%.0f images/s), %.2f ms of host time per call" % (name, e0.elapsed_time(e1) / 10, N, N / (e0.elapsed_time(e1) / 10) * 1e3, t_host * 1e3))
    assert torch.equal(out, ref)
