"""GPU: the device half of the JPEG encode (hipts_jpeg_encode_batch_u8, csrc/jpegenc.hip) against tests/jpegenc_ref.py, the numpy
restatement test_jpegenc_reference.py pins against Pillow, and hiptagsearch.thumbs.jpeg_encode against Pillow's own files.  Everything is
integer arithmetic, so every comparison is exact.

The sizes: 16 x 16 (one MCU), 32 x 48, 40 x 56 (a partial bottom MCU row), 37 x 45 (odd both ways; a width whose rows do not start on a
dword: the byte loads), 64 x 64 (a full workgroup strip), and -- a workgroup takes four MCUs of a row -- 48 x 144 and 24 x 150: three
workgroups per MCU row, the last one partly past the last MCU, with dword and with byte loads.  Batches of 3: noise, structured content
and saturated patches.
"""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

import jpegenc_ref as jr

pytestmark = pytest.mark.gpu

CASES = [((16, 16), 85), ((32, 48), 30), ((40, 56), 100), ((37, 45), 75), ((64, 64), 50), ((48, 144), 90), ((24, 150), 85)]
IDS = ["%dx%d-q%d" % (h, w, q) for (h, w), q in CASES]
_BATCH = {}


def _batch(hw, q):
    """(uint8 [3, h, w, 3], the restatement's three slots): made once per case"""
    if (hw, q) not in _BATCH:
        h, w = hw
        images = np.stack([jr.noise_image(h, w, q), jr.structured_image(h, w, q), jr.saturated_image(h, w)])
        _BATCH[(hw, q)] = (images, [jr.slot(im, q) for im in images])
    return _BATCH[(hw, q)]


def _pillow(image, q):
    buf = io.BytesIO()
    Image.fromarray(image).save(buf, "JPEG", quality=q)
    return buf.getvalue()


def _encode_slots(images, q, on_device, out_on_device, extra=0, fill=0xEE):
    """the raw entry point: uint8 [n, stride] slots (stride = hipts_jpeg_slot_bytes + extra), prefilled with `fill`"""
    import torch
    from hiptagsearch import _lib
    n, h, w = images.shape[:3]
    stride = int(_lib.load().hipts_jpeg_slot_bytes(w, h)) + extra
    src = torch.from_numpy(np.ascontiguousarray(images))
    src = src.cuda() if on_device else src
    out = torch.full((n, stride), fill, dtype=torch.uint8)
    out = out.cuda() if out_on_device else out
    _lib.call("hipts_jpeg_encode_batch_u8", _lib.ptr(src), _lib.DEVICE if on_device else _lib.HOST, n, h, w, q, _lib.ptr(out),
              _lib.DEVICE if out_on_device else _lib.HOST, ctypes.c_int64(stride), 0, _lib.current_stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_slots_equal_the_restatement(case, memory):
    (hw, q) = case
    images, want = _batch(hw, q)
    got = _encode_slots(images, q, memory == "device", memory == "device")
    for i in range(3):
        total = len(want[i])
        f, comps, quant = jr.parse(got[i])
        g, want_comps, want_quant = jr.parse(want[i])
        assert f == g, "image %d" % i
        np.testing.assert_array_equal(quant, want_quant)
        for c in range(3):
            np.testing.assert_array_equal(comps[c], want_comps[c], err_msg="image %d component %d" % (i, c))
        np.testing.assert_array_equal(got[i][:total], want[i])              # and every other byte of the header
        assert (got[i][total:] == 0xEE).all()                               # nothing behind the slot's last block


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_jpeg_encode_writes_pillows_files(case):
    from hiptagsearch.thumbs import jpeg_encode
    import torch
    (hw, q) = case
    images, _ = _batch(hw, q)
    want = [_pillow(im, q) for im in images]
    assert jpeg_encode(images, q) == want
    assert jpeg_encode(torch.from_numpy(images).cuda(), q, threads=1) == want
    # image i of a batch equals the same image encoded alone
    for i in range(3):
        assert jpeg_encode(images[i:i + 1], q) == want[i:i + 1]


@pytest.mark.parametrize("extra", [48, 7], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("out_on_device", [False, True], ids=["host-out", "device-out"])
def test_a_larger_stride_leaves_the_bytes_between_slots_alone(extra, out_on_device):
    images, want = _batch((40, 56), 100)
    for fill in (0xEE, 0x11):
        got = _encode_slots(images, 100, True, out_on_device, extra=extra, fill=fill)
        for i in range(3):
            total = len(want[i])
            np.testing.assert_array_equal(got[i][:total], want[i])
            assert (got[i][total:] == fill).all()


def test_the_slots_feed_the_device_decoder():
    """the encoder's slot goes into hipts_jpeg_decode_rgb as it stands and gives what Pillow decodes from Pillow's file"""
    import torch
    from hiptagsearch import _lib
    images, _ = _batch((37, 45), 75)
    got = _encode_slots(images, 75, True, False)
    for i in range(3):
        rgb = np.zeros((37, 45, 3), dtype=np.uint8)
        _lib.call("hipts_jpeg_decode_rgb", _lib.ptr(np.ascontiguousarray(got[i])), ctypes.c_int64(got.shape[1]), _lib.ptr(rgb), _lib.HOST,
                  ctypes.c_int64(rgb.size), 0, _lib.current_stream_ptr())
        np.testing.assert_array_equal(rgb, np.asarray(Image.open(io.BytesIO(_pillow(images[i], 75))).convert("RGB")))


def test_a_larger_image_and_a_flat_one():
    from hiptagsearch.thumbs import jpeg_encode
    images = np.stack([jr.structured_image(256, 256, 5), jr.white_image(256, 256)])
    assert jpeg_encode(images, 85) == [_pillow(im, 85) for im in images]
    wide = jr.noise_image(33, 530, 9)[None]                                 # nine workgroups per MCU row
    assert jpeg_encode(wide, 60) == [_pillow(wide[0], 60)]


def test_argument_errors():
    from hiptagsearch import HipTagSearchError, _lib
    from hiptagsearch.thumbs import jpeg_encode
    need = int(_lib.load().hipts_jpeg_slot_bytes(16, 16))
    out = np.zeros(need, dtype=np.uint8)
    buf = np.zeros(16 * 16 * 3, dtype=np.uint8)                             # never read: the arguments are refused first
    for h, w, q, stride, word in ((8, 16, 85, need, "size"), (16, 8, 85, need, "size"), (16, 8193, 85, 1 << 30, "size"), (16, 16, 0, need, "quality"),
                                  (16, 16, 101, need, "quality"), (16, 16, 85, need - 1, "slot_stride")):
        with pytest.raises(HipTagSearchError, match=word) as e:
            _lib.call("hipts_jpeg_encode_batch_u8", _lib.ptr(buf), _lib.HOST, 1, h, w, q, _lib.ptr(out), _lib.HOST, ctypes.c_int64(stride), 0, None)
        assert e.value.status == -1
    assert not out.any()
    with pytest.raises(ValueError):
        jpeg_encode(np.zeros((1, 16, 16), dtype=np.uint8))
    with pytest.raises(ValueError):
        jpeg_encode(np.zeros((1, 16, 16, 3), dtype=np.float32))
    assert jpeg_encode(np.zeros((0, 16, 16, 3), dtype=np.uint8)) == []
    image = jr.noise_image(16, 16, 1)                                       # a valid call right after the refusals
    assert jpeg_encode(image[None], 85) == [_pillow(image, 85)]
