"""GPU parity of the hybrid PNG decode (hiptagsearch/png_host.py + csrc/png.hip) through the C ABI: the bytes Pillow gives the reference
(Image.open, grey -> RGB, alpha composited over white as Predictor.prepare_image does, tagging.py:100-120) reproduced exactly -- alone,
in front of the pad + resize, inside the multi-process decode pipeline and through the two CLIs.

The kernel's sizes: a band is 64 rows (one wave), a lane walks its row in groups of 4 pixels, a round is 64 group steps, i.e. a column
chunk is 256 pixels, and a band of ceil(w / 4) + 63 group steps takes another round from w = 5 (65 steps) and from w = 261 (129 steps);
bands are dealt to 4 waves, so the fifth band (row 256) is the first that a wave takes after another.  The shapes below sit on and
around each of those."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_ref  # noqa: E402
from test_oracle_jpeg import jpeg_bytes, synth_image  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "anime-illust-image-searcher_amd")

SHAPES = [(1, 1), (1, 200), (200, 1), (63, 65), (64, 64), (65, 63),             # the band of 64 rows, the issue's shapes
          (5, 2 * 256 + 7),                                                     # two column chunks + 7 pixels: the chunk seam
          (3, 3), (3, 4), (3, 5), (2, 255), (2, 256), (2, 257), (3, 260), (3, 261), (3, 264),      # whole / ragged pixel groups, one more round
          (257, 6), (321, 70),                                                  # a wave's second band
          (300, 530)]                                                           # several bands x several chunks in flight at once


def _slot_of(data, stride=None):
    from hiptagsearch import png_host
    w, h = Image.open(io.BytesIO(data)).size
    slot = np.zeros(stride or png_host.slot_bytes(w, h, 4), dtype=np.uint8)
    return png_host.png_inflate_into(data, slot), slot, (h, w)


def _decode(_lib, slot, h, w):
    got = np.empty((h, w, 3), dtype=np.uint8)
    _lib.call("hipts_png_decode_rgb", slot.ctypes.data, slot.nbytes, got.ctypes.data, _lib.HOST, got.nbytes, 0, None)
    return got


def _want(data, c):
    img = Image.open(io.BytesIO(data))
    assert img.mode == png_ref.MODES[c]
    if c == 3:
        return np.asarray(img)                                   # Image.open alone
    if c == 1:
        return np.asarray(img.convert("RGB"))
    bg = Image.new("RGB", img.size, (255, 255, 255))             # the white composite of prepare_image
    bg.paste(img, mask=img.split()[-1])
    return np.asarray(bg)


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_device_decode_equals_pillow(c):
    from hiptagsearch import _lib
    import torch
    rng = np.random.default_rng(100 + c)
    files = []
    for h, w in SHAPES:
        arr = png_ref.noise(rng, h, w, c)
        files.append(((h, w), "pillow", png_ref.pillow_png(arr)))
        files.append(((h, w), "random filters", png_ref.write_png(arr, types=rng.integers(0, 5, h), idat_chunks=2)))
    arr = png_ref.noise(rng, 130, 131, c)
    for k in range(5):      # every filter type on the first row, on the last row of a band and on the first row of the next
        files.append(((130, 131), "filter (y + %d) %% 5" % k, png_ref.write_png(arr, types=[(y + k) % 5 for y in range(130)])))
    for (h, w), name, data in files:
        want = _want(data, c)
        st, slot, _ = _slot_of(data)
        assert st == 0, ((h, w), name)
        got = _decode(_lib, slot, h, w)
        assert np.array_equal(got, want), ((h, w), name, int((got != want).sum()), np.argwhere((got != want).any(axis=2))[:4].tolist())
    assert np.array_equal(want, png_ref.decode_slot(slot))       # (the CPU restatement agrees with Pillow on the last one)
    # device-resident output: a word-aligned one (the store path of widths that are a multiple of 4) and one that is not
    for (h, w), off in (((64, 64), 0), ((64, 64), 1), ((65, 63), 0)):
        data = png_ref.write_png(png_ref.noise(rng, h, w, c))
        st, slot, _ = _slot_of(data)
        assert st == 0
        dev = torch.zeros(h * w * 3 + 8, dtype=torch.uint8, device="cuda")
        _lib.call("hipts_png_decode_rgb", slot.ctypes.data, slot.nbytes, dev.data_ptr() + off, _lib.DEVICE, h * w * 3, 0, None)
        out = dev.cpu().numpy()
        assert np.array_equal(out[off:off + h * w * 3].reshape(h, w, 3), _want(data, c))
        assert not out[:off].any() and not out[off + h * w * 3:].any()          # nothing written around the image
    # a slot that is not one, an output that is one byte short
    got = np.empty((h, w, 3), dtype=np.uint8)
    bad = slot.copy()
    bad[:4] = 0
    with pytest.raises(_lib.HipTagSearchError):
        _lib.call("hipts_png_decode_rgb", bad.ctypes.data, bad.nbytes, got.ctypes.data, _lib.HOST, got.nbytes, 0, None)
    with pytest.raises(_lib.HipTagSearchError):
        _lib.call("hipts_png_decode_rgb", slot.ctypes.data, slot.nbytes, got.ctypes.data, _lib.HOST, got.nbytes - 1, 0, None)
    # a header that disagrees with the slot's size
    with pytest.raises(_lib.HipTagSearchError):
        _lib.call("hipts_png_decode_rgb", slot.ctypes.data, int(slot[32:40].view(np.int64)[0]) - 1, got.ctypes.data, _lib.HOST, got.nbytes, 0, None)
    _lib.call("hipts_png_decode_rgb", slot.ctypes.data, slot.nbytes, got.ctypes.data, _lib.HOST, got.nbytes, 0, None)
    assert np.array_equal(got, _want(data, c))


def _smooth_png(rng, h, w, c):
    small = rng.integers(0, 256, (max(2, h // 16), max(2, w // 16), c), dtype=np.uint8)
    big = np.stack([np.asarray(Image.fromarray(small[:, :, k]).resize((w, h), Image.BICUBIC)) for k in range(c)], axis=2).astype(np.int16)
    return png_ref.pillow_png(np.clip(big + rng.integers(-8, 9, big.shape), 0, 255).astype(np.uint8))


@pytest.mark.parametrize("mode", ["tagger", "ccip"])
def test_batch_of_scanline_coefficient_and_decoded_slots(mode):
    """hipts_decode_batch_u8 = decode on the device + hipts_resize_batch_u8: against the latter fed with Pillow's decode of the same files,
    the three kinds of slot mixed in one call."""
    from hiptagsearch import _lib
    import torch
    rng = np.random.default_rng(21)
    S = 448 if mode == "tagger" else 384
    files = [_smooth_png(rng, 768, 1024, 4), jpeg_bytes(synth_image(rng, 500, 333), quality=80, subsampling=1),
             png_ref.write_png(png_ref.noise(rng, 97, 211, 3)), png_ref.pillow_png(png_ref.noise(rng, 300, 200, 1)),
             jpeg_bytes(synth_image(rng, 240, 320, grey=True), quality=85), png_ref.write_png(png_ref.noise(rng, 333, 222, 2)),
             _smooth_png(rng, 600, 900, 3)]
    buf = io.BytesIO()
    Image.fromarray(png_ref.noise(rng, 120, 90, 3)).convert("P", palette=Image.ADAPTIVE, colors=32).save(buf, format="PNG")
    files.append(buf.getvalue())                                            # refused by the fast path: a decoded slot
    stride = 1024 * 768 * 4 + 768 + 1024
    slots = np.zeros((len(files), stride), dtype=np.uint8)
    ref = np.zeros((len(files), stride), dtype=np.uint8)
    kinds, hw = [], []
    for i, data in enumerate(files):
        img = png_ref.pillow_rgb(data)
        h, w = img.shape[:2]
        ref[i, :img.size] = img.reshape(-1)
        if data[:2] == b"\xff\xd8":
            src = np.frombuffer(data, dtype=np.uint8)
            st, kind = _lib.load().hipts_jpeg_entropy_decode(src.ctypes.data, len(data), slots[i].ctypes.data, stride), 1
        else:
            from hiptagsearch import png_host
            st, kind = png_host.png_inflate_into(data, slots[i]), 2
        if st != 0:
            assert st == 1
            slots[i, :img.size] = img.reshape(-1)
            kind = 0
        kinds.append(kind)
        hw.append((h, w))
    assert kinds == [2, 1, 2, 2, 1, 2, 2, 0]
    kinds = np.asarray(kinds, dtype=np.int32)
    hw = np.ascontiguousarray(np.asarray(hw, dtype=np.int32))
    pad, filt = (1, 3) if mode == "tagger" else (0, 2)
    got = torch.empty((len(files), S, S, 3), dtype=torch.uint8, device="cuda")
    want = torch.empty_like(got)
    s = torch.cuda.current_stream().cuda_stream
    _lib.call("hipts_decode_batch_u8", slots.ctypes.data, stride, _lib.ptr(kinds), _lib.ptr(hw), len(files), pad, _lib.ptr(got), S, filt, 0, s)
    _lib.call("hipts_resize_batch_u8", ref.ctypes.data, _lib.HOST, stride, _lib.ptr(hw), len(files), pad, _lib.ptr(want), S, filt, 0, s)
    torch.cuda.synchronize()
    assert torch.equal(got, want), [bool(torch.equal(got[i], want[i])) for i in range(len(files))]
    # twice in a row on two streams (the staging buffers are shared: the second call is ordered behind the first)
    side = torch.cuda.Stream()
    got2 = torch.empty_like(got)
    _lib.call("hipts_decode_batch_u8", slots.ctypes.data, stride, _lib.ptr(kinds), _lib.ptr(hw), len(files), pad, _lib.ptr(got2), S, filt, 0, side.cuda_stream)
    _lib.call("hipts_decode_batch_u8", slots.ctypes.data, stride, _lib.ptr(kinds), _lib.ptr(hw), len(files), pad, _lib.ptr(got), S, filt, 0, s)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(got2, want)
    # a header that disagrees with the caller is refused, for a scanline slot as for a coefficient slot
    for i in (0, 1):
        hw2 = hw.copy()
        hw2[i, 0] += 1
        with pytest.raises(_lib.HipTagSearchError):
            _lib.call("hipts_decode_batch_u8", slots.ctypes.data, stride, _lib.ptr(kinds), _lib.ptr(hw2), len(files), pad, _lib.ptr(got), S, filt, 0, s)
    # hipts_jpeg_batch_u8 is what it was: it refuses kind 2, and still takes kinds 0 and 1
    with pytest.raises(_lib.HipTagSearchError):
        _lib.call("hipts_jpeg_batch_u8", slots.ctypes.data, stride, _lib.ptr(kinds), _lib.ptr(hw), len(files), pad, _lib.ptr(got), S, filt, 0, s)
    sel = [1, 4, 7]
    part = torch.empty((3, S, S, 3), dtype=torch.uint8, device="cuda")
    sub = np.ascontiguousarray(slots[sel])
    _lib.call("hipts_jpeg_batch_u8", sub.ctypes.data, stride, _lib.ptr(np.ascontiguousarray(kinds[sel])), _lib.ptr(np.ascontiguousarray(hw[sel])), 3, pad,
              _lib.ptr(part), S, filt, 0, s)
    torch.cuda.synchronize()
    assert torch.equal(part, want[sel])


def test_more_scanline_slots_than_one_launch_takes():
    """70 small PNGs in one call: the descriptors of 64 images travel with a launch, the rest with the next."""
    from hiptagsearch import _lib, png_host
    import torch
    rng = np.random.default_rng(33)
    n, stride, S = 70, 4096, 32
    slots = np.zeros((n, stride), dtype=np.uint8)
    ref = np.zeros((n, stride), dtype=np.uint8)
    hw = np.zeros((n, 2), dtype=np.int32)
    for i in range(n):
        h, w, c = int(rng.integers(1, 24)), int(rng.integers(1, 24)), 1 + i % 4
        data = png_ref.write_png(png_ref.noise(rng, h, w, c), types=rng.integers(0, 5, h), idat_chunks=1)
        assert png_host.png_inflate_into(data, slots[i]) == 0
        img = png_ref.pillow_rgb(data)
        ref[i, :img.size] = img.reshape(-1)
        hw[i] = (h, w)
    kinds = np.full(n, 2, dtype=np.int32)
    got = torch.empty((n, S, S, 3), dtype=torch.uint8, device="cuda")
    want = torch.empty_like(got)
    s = torch.cuda.current_stream().cuda_stream
    _lib.call("hipts_decode_batch_u8", slots.ctypes.data, stride, _lib.ptr(kinds), _lib.ptr(hw), n, 1, _lib.ptr(got), S, 3, 0, s)
    _lib.call("hipts_resize_batch_u8", ref.ctypes.data, _lib.HOST, stride, _lib.ptr(hw), n, 1, _lib.ptr(want), S, 3, 0, s)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def _corpus(tmp_path, rng):
    paths = []

    def add(name, data, at=None):
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(data)
        paths.insert(len(paths) if at is None else at, p)
    for i in range(30):
        h, w, c = int(rng.integers(40, 900)), int(rng.integers(40, 900)), 1 + i % 4
        if i % 3 == 0:
            data = png_ref.write_png(png_ref.noise(rng, h, w, c), types=rng.integers(0, 5, h), idat_chunks=1 + i % 4)
        elif i % 3 == 1:
            data = _smooth_png(rng, h, w, c)
        else:
            data = png_ref.pillow_png(png_ref.noise(rng, h, w, c))
        add("img%03d.png" % i, data)
    buf = io.BytesIO()
    Image.fromarray(png_ref.noise(rng, 120, 90, 3)).convert("P", palette=Image.ADAPTIVE, colors=32).save(buf, format="PNG")
    add("palette.png", buf.getvalue(), 5)
    buf = io.BytesIO()
    Image.fromarray(rng.integers(0, 65536, (70, 110), dtype=np.uint16)).save(buf, format="PNG")
    add("deep.png", buf.getvalue(), 11)
    good = png_ref.pillow_png(png_ref.noise(rng, 200, 300, 3))
    add("truncated.png", good[:len(good) // 2], 17)
    pos = good.index(b"IDAT") + 4 + 2000
    add("flipped.png", good[:pos] + bytes([good[pos] ^ 0x40]) + good[pos + 1:], 23)
    add("big.png", _smooth_png(rng, 700, 900, 4))                           # beyond max_pixels: resized by the worker in both runs
    for i in range(4):
        add("photo%d.jpg" % i, jpeg_bytes(synth_image(rng, int(rng.integers(40, 700)), int(rng.integers(40, 900))), quality=85, subsampling=i % 3), 3 + 7 * i)
    return paths


@pytest.mark.parametrize("jpeg", [False, True])
def test_decode_pool_with_device_png_equals_pillow_workers(tmp_path, jpeg):
    """The multi-process pipeline with the hybrid PNG decode against the same pipeline decoding with Pillow: same kept files, same uint8
    model inputs."""
    from hiptagsearch import pipeline
    import torch
    paths = _corpus(tmp_path, np.random.default_rng(9))
    outs = {}
    for png in (False, True):
        kept_all, tens = [], []
        with pipeline.DecodePool(workers=4, size=448, batch=16, mode=pipeline.TAGGER, device_resize=True, max_pixels=600 * 800, device_jpeg=jpeg,
                                 device_png=png) as pool:
            for kept, images in pool.batches(paths):
                kept_all += kept
                tens.append(images.clone())
        torch.cuda.synchronize()
        outs[png] = (kept_all, torch.cat(tens).cpu().numpy())
    assert outs[True][0] == outs[False][0] and len(outs[True][0]) == len(paths) - 2
    assert not any("truncated" in p or "flipped" in p for p in outs[True][0])
    assert np.array_equal(outs[True][1], outs[False][1])


def test_device_png_needs_device_resize():
    from hiptagsearch import pipeline
    with pytest.raises(ValueError):
        pipeline.DecodePool(workers=1, size=64, batch=4, device_png=True)


def test_clis_with_gpu_png_write_the_same_files(tmp_path, monkeypatch):
    """tagging.py / gen_cfeatures.py with --workers N --gpu-png (inflate in the workers, the rest of the PNG decode on the device): the
    tag file and the feature rows of the plain runs, over PNGs of the four colour types, a palette PNG, JPEGs and a file that is not an
    image."""
    from hiptagsearch.index import Similarity
    monkeypatch.chdir(tmp_path)
    os.makedirs("imgs/sub")
    rng = np.random.default_rng(5)
    for i in range(12):
        h, w, c = int(rng.integers(40, 400)), int(rng.integers(40, 500)), 1 + i % 4
        data = _smooth_png(rng, h, w, c) if i % 2 else png_ref.write_png(png_ref.noise(rng, h, w, c), types=rng.integers(0, 5, h))
        open("imgs/%s%02d.png" % ("sub/" if i % 2 else "", i), "wb").write(data)
    Image.fromarray(png_ref.noise(rng, 60, 80, 3)).convert("P", palette=Image.ADAPTIVE, colors=16).save("imgs/palette.png")
    for i in range(2):
        synth_image(rng, 120 + 50 * i, 200).save("imgs/photo%d.jpg" % i, quality=85)
    open("imgs/broken.png", "wb").write(png_ref.SIGNATURE + b" not a png")
    tag_cli, feat_cli = os.path.join(PKG, "tagging.py"), os.path.join(PKG, "gen_cfeatures.py")
    outs = []
    for extra in ([], ["--workers", "2", "--gpu-png"]):
        if os.path.exists("tags-wd-tagger.txt"):
            os.remove("tags-wd-tagger.txt")
        r = subprocess.run([sys.executable, tag_cli, "--dir", "imgs", "--batch", "8", "--model", "vit-tiny"] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(sorted(open("tags-wd-tagger.txt", encoding="utf-8").read().splitlines()))
    assert len(outs[0]) == 15 and outs[0] == outs[1]
    feats = []
    for k, extra in enumerate(([], ["--workers", "2", "--gpu-png"])):
        for f in os.listdir("."):
            if f.startswith("charactor-featues-idx"):
                os.remove(f)
        r = subprocess.run([sys.executable, feat_cli, "--dir", "imgs", "--batch", "8", "--arch", "tiny"] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        paths = open("charactor-featues-idx.csv", encoding="utf-8").read().splitlines()
        m = Similarity.load("charactor-featues-idx").matrix()
        feats.append({p: m[i] for i, p in enumerate(paths)})
    assert sorted(feats[0]) == sorted(feats[1]) and len(feats[0]) == 15
    for p in feats[0]:
        np.testing.assert_allclose(feats[1][p], feats[0][p], atol=1e-5)
