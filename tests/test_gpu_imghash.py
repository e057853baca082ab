"""GPU: hiptagsearch.dedup.image_hashes (hipts_image_hash_u8, csrc/imghash.hip) against tests/imghash_ref.py::hash128, the numpy
restatement test_imghash_reference.py pins.  Everything is integer arithmetic, so every comparison is exact.

The sizes: 9 (cells of one pixel), 18, 64, 384 and 448 (multiples of 16 from 64 on: the 16-byte loads), 100 (byte loads) -- 100 and 448
have cells of unequal areas; 1024 is the largest size (the largest sums and products).  Batches 1, 3 and 65: how many workgroups share an
image follows from the batch, from hundreds of row runs per image down to sixteen.
"""
import ctypes

import numpy as np
import pytest

import imghash_ref as ir

pytestmark = pytest.mark.gpu

SIZES = [9, 18, 64, 100, 384, 448]
BATCHES = [1, 3, 65]
_NOISE = {}


def _noise(size):
    """(uint8 [65, size, size, 3] uniform noise, its hashes by the restatement): every cell mean lies near 127.5, so almost every bit is
    a close call.  Made once per size; the smaller batches are its first images."""
    if size not in _NOISE:
        images = np.random.default_rng(1000 + size).integers(0, 256, (max(BATCHES), size, size, 3), dtype=np.uint8)
        _NOISE[size] = (images, ir.hash128(images))
    return _NOISE[size]


def _hashes(images, on_device=False):
    from hiptagsearch.dedup import image_hashes
    if on_device:
        import torch
        images = torch.from_numpy(np.ascontiguousarray(images)).cuda()
    got = image_hashes(images)
    assert got.dtype == np.uint64 and got.shape == (len(images), 2)
    return got


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("size", SIZES)
def test_bits_equal_the_restatement_on_noise(size, batch, on_device):
    images, want = _noise(size)
    np.testing.assert_array_equal(_hashes(images[:batch], on_device), want[:batch])
    assert len(np.unique(want[:, 0])) == len(want)               # the reference itself tells the images apart


@pytest.mark.parametrize("size", [9, 64, 100, 448])
def test_flat_and_ramps(size):
    got = _hashes(np.stack([ir.flat_image(size), ir.ramp_image(size, True), ir.ramp_image(size, False), ir.flat_image(size, 0),
                            ir.flat_image(size, 255)]))
    assert got.tolist() == [[0, 0], [ir.ALL64, 0], [0, ir.ALL64], [0, 0], [0, 0]]


def test_equal_means_of_unequal_areas_compare_exactly():
    a, b = ir.equal_mean_pair()
    pair = np.stack([a, b])
    got = _hashes(pair)
    assert int(got[0, 0]) == 0 and int(got[1, 0]) == 1 << 7
    np.testing.assert_array_equal(got, ir.hash128(pair))


@pytest.mark.parametrize("size", [448, 1024])
def test_saturated_input(size):
    images = np.stack([ir.saturated_image(size, 254), ir.saturated_image(size, 0), ir.saturated_image(size, 254, (7, 8)),
                       ir.saturated_image(size, 0, (0, 0))])
    want = ir.hash128(images)
    assert int(want[0, 0]) == int(want[1, 0]) == 1 << (8 * 3 + 4) and int(want[3, 0]) == 1 and (want[[0, 1, 3], 1] != 0).all()
    for on_device in (False, True):
        np.testing.assert_array_equal(_hashes(images, on_device), want)


@pytest.mark.parametrize("size", [100, 448])
def test_an_image_of_a_batch_equals_the_image_alone(size):
    images, want = _noise(size)
    images = images[:7]
    together = _hashes(images, True)
    for i in range(len(images)):
        np.testing.assert_array_equal(_hashes(images[i:i + 1], True)[0], together[i], err_msg="image %d" % i)
    np.testing.assert_array_equal(together, want[:7])
    # a copy among different images hashes like its original, wherever it stands
    order = [3, 0, 3, 6, 1, 3]
    np.testing.assert_array_equal(_hashes(images[order]), want[order])


def test_more_images_than_one_call_takes():
    from hiptagsearch import dedup
    images, want = _noise(18)
    n = 2 * dedup.CHUNK + 5
    pick = np.arange(n) % len(images)
    np.testing.assert_array_equal(_hashes(images[pick]), want[pick])
    assert _hashes(images[:0]).shape == (0, 2)


def test_device_output_and_the_callers_stream():
    """the raw entry point with device memory on both sides, on a stream of the caller's: nothing is synchronised by the call"""
    import torch
    from hiptagsearch import _lib
    images, want = _noise(64)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev = torch.from_numpy(images[:9].copy()).cuda()
        out = torch.zeros((9, 2), dtype=torch.int64, device="cuda")
        _lib.call("hipts_image_hash_u8", _lib.ptr(dev), _lib.DEVICE, 9, 64, _lib.ptr(out), _lib.DEVICE, 0, ctypes.c_void_p(stream.cuda_stream))
    stream.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64), want[:9])


def test_refusals():
    from hiptagsearch import HipTagSearchError, _lib
    from hiptagsearch.dedup import image_hashes
    out = np.zeros((1, 2), dtype=np.uint64)
    for size, batch, word in ((8, 1, "size"), (1025, 1, "size"), (64, 0, "batch")):
        buf = np.zeros(64, dtype=np.uint8)               # never read: the arguments are refused first
        with pytest.raises(HipTagSearchError, match=word) as e:
            _lib.call("hipts_image_hash_u8", _lib.ptr(buf), _lib.HOST, batch, size, _lib.ptr(out), _lib.HOST, 0, None)
        assert e.value.status == -1
    with pytest.raises(HipTagSearchError, match="size"):
        image_hashes(np.zeros((2, 8, 8, 3), dtype=np.uint8))
    with pytest.raises(ValueError):
        image_hashes(np.zeros((2, 16, 12, 3), dtype=np.uint8))
    with pytest.raises(ValueError):
        image_hashes(np.zeros((2, 16, 16, 3), dtype=np.float32))
    np.testing.assert_array_equal(_hashes(_noise(9)[0][:2]), _noise(9)[1][:2])       # a valid call right after the refusals
