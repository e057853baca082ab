"""CPU: the JPEG encoder's arithmetic and its host coder against Pillow itself.

  * tests/jpegenc_ref.py -- the numpy statement of libjpeg's forward path the GPU tests hold csrc/jpegenc.hip to -- gives the quantised
    coefficients of the file PIL.Image.save(..., "JPEG", quality=Q) writes: Pillow's file is read back with hipts_jpeg_entropy_decode
    (libhipts_jpeg_host.so) and every block of every component, filler blocks included, the tables and the header agree.
  * hipts_jpeg_entropy_encode (csrc/jpeg_host.c) turns that slot into Pillow's file byte for byte, and decoding gives the slot back.
  * what the coder refuses, and that it never writes past `capacity` (guard bytes here; a sanitizer build of a stand-alone program,
    tests/jpegenc_host_check.c, for the reads and writes a guard cannot see).

Sizes: 16 x 16 (one MCU), 32 x 48, 40 x 56 (a partial bottom MCU row: downsampled chroma rows are replicated, not full-resolution ones),
37 x 45 and 17 x 33 (odd both ways; filler blocks right, below and in the corner), 24 x 17, 100 x 100, 128 x 91.  Qualities 30 .. 100
(100: all-ones tables, the longest codes).  Content: noise (every coefficient alive), structured (long zero runs, ZRL and EOB codes), flat
white, and saturated patches (the largest coefficients)."""
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpegenc_ref as jr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "anime-illust-image-searcher_amd", "csrc")
HOST_LIB = os.path.join(ROOT, "anime-illust-image-searcher_amd", "libhipts_jpeg_host.so")

SIZES = [(16, 16), (32, 48), (40, 56), (37, 45), (17, 33), (24, 17), (100, 100), (128, 91)]
QUALITIES = [30, 50, 75, 85, 90, 100]
GUARD = 64


def host_lib():
    lib = ctypes.CDLL(HOST_LIB)
    lib.hipts_jpeg_entropy_decode.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
    lib.hipts_jpeg_entropy_encode.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    lib.hipts_jpeg_slot_bytes.restype = ctypes.c_int64
    return lib


def pillow_file(image, quality):
    buf = io.BytesIO()
    Image.fromarray(image).save(buf, "JPEG", quality=quality)
    return buf.getvalue()


def images_of(h, w, q):
    return [("noise", jr.noise_image(h, w, q)), ("structured", jr.structured_image(h, w, q)), ("white", jr.white_image(h, w)),
            ("saturated", jr.saturated_image(h, w))]


_CASES = {}


def cases():
    """[(label, image, quality, Pillow's file, the restatement's slot)], made once"""
    if not _CASES:
        out = []
        for (h, w) in SIZES:
            for q in QUALITIES:
                for kind, image in images_of(h, w, q):
                    out.append(("%dx%d q%d %s" % (h, w, q, kind), image, q, pillow_file(image, q), jr.slot(image, q)))
        _CASES["all"] = out
    return _CASES["all"]


def encode(lib, slot, capacity, slot_bytes=None):
    """(status, nbytes, the output buffer with GUARD bytes of 0xEE after `capacity`)"""
    out = np.full(capacity + GUARD, 0xEE, dtype=np.uint8)
    nb = ctypes.c_int64(-1)
    slot = np.ascontiguousarray(slot)
    st = lib.hipts_jpeg_entropy_encode(slot.ctypes.data, len(slot) if slot_bytes is None else slot_bytes, out.ctypes.data, capacity, ctypes.byref(nb))
    assert (out[capacity:] == 0xEE).all(), "stored past the capacity"
    return st, nb.value, out


def test_restatement_equals_pillows_coefficients():
    lib = host_lib()
    assert len(cases()) == len(SIZES) * len(QUALITIES) * 4
    fillers = 0
    for label, image, q, data, mine in cases():
        h, w = image.shape[:2]
        nb = lib.hipts_jpeg_slot_bytes(w, h)
        slot = np.zeros(nb, dtype=np.uint8)
        arr = np.frombuffer(data, dtype=np.uint8)
        assert lib.hipts_jpeg_entropy_decode(arr.ctypes.data, len(arr), slot.ctypes.data, nb) == 0, label
        f, comps, quant = jr.parse(slot)
        g, mine_comps, mine_quant = jr.parse(mine)
        assert f == g, label
        np.testing.assert_array_equal(quant, mine_quant, err_msg=label)
        for c in range(3):
            np.testing.assert_array_equal(comps[c], mine_comps[c], err_msg="%s component %d" % (label, c))
        np.testing.assert_array_equal(slot[:f["total_bytes"]], mine, err_msg=label)
        fillers += comps[0].shape[0] * comps[0].shape[1] - ((h + 7) // 8) * ((w + 7) // 8)
    assert fillers > 0                                   # the cases do contain filler blocks


def test_host_coder_writes_pillows_file():
    lib = host_lib()
    for label, image, q, data, mine in cases():
        st, nb, out = encode(lib, mine, len(data))       # a capacity of exactly the file
        assert st == 0 and nb == len(data), label
        assert out[:nb].tobytes() == data, label
        back = np.full(len(mine), 0xA5, dtype=np.uint8)
        assert lib.hipts_jpeg_entropy_decode(out.ctypes.data, nb, back.ctypes.data, len(back)) == 0, label
        np.testing.assert_array_equal(back, mine, err_msg=label)


def test_the_file_opens_in_pillow():
    lib = host_lib()
    label, image, q, data, mine = cases()[len(cases()) // 2]
    st, nb, out = encode(lib, mine, len(data) + 100)
    assert st == 0
    im = Image.open(io.BytesIO(out[:nb].tobytes()))
    assert im.size == (image.shape[1], image.shape[0]) and im.mode == "RGB"
    np.testing.assert_array_equal(np.asarray(im), np.asarray(Image.open(io.BytesIO(data))))


def _changed(slot, change):
    s = slot.copy()
    change(s)
    return s


def test_refusals():
    lib = host_lib()
    image = jr.noise_image(40, 56, 3)
    data, slot = pillow_file(image, 85), jr.slot(image, 85)
    head = lambda s: s[:128].view(np.int32)
    coef = lambda s: s[jr.HEADER_BYTES:].view(np.int16)

    def magic(s): head(s)[0] ^= 1
    def s444(s): head(s)[[5, 6, 8, 9]] = 1
    def grey(s): head(s)[4] = 1
    def offset(s): head(s)[8 + 16 + 6] += 64
    def negative_offset(s): head(s)[8 + 8 + 6] = -64
    def dc2048(s): coef(s)[0] = 2048
    def dc_minus_2048(s): coef(s)[64 * 5] = -2048
    def ac1024(s): coef(s)[64 + 9] = 1024
    def blocks(s): head(s)[8 + 2] += 2
    def quant0(s): s[128:130] = 0
    def chroma_tables_differ(s): s[128 + 256] ^= 1

    for change, status in ((magic, 3), (s444, 1), (grey, 1), (offset, 3), (negative_offset, 3), (dc2048, 3), (dc_minus_2048, 3), (ac1024, 3),
                           (blocks, 3), (quant0, 1), (chroma_tables_differ, 1)):
        st, nb, out = encode(lib, _changed(slot, change), len(data))
        assert (st, nb) == (status, 0), change.__name__
    # the largest values that do have a code pass
    def largest(s):
        coef(s)[0:48 * 64:64] = 2047                     # every luminance DC: the first difference is 2047, the others 0
        coef(s)[1] = -1023
    st, nb, out = encode(lib, _changed(slot, largest), 2 * len(data))
    assert st == 0 and nb > 0
    # a slot shorter than its header says, and shorter than a header
    assert encode(lib, slot[:-2], len(data))[:2] == (3, 0)
    assert encode(lib, slot[:100], len(data))[:2] == (2, 0)
    # a capacity one byte short, and everything below it: an error, and the guard bytes behind the capacity stay
    for capacity in [len(data) - 1, len(data) - 2, len(data) // 2, 700, 623, 622, 100, 1, 0]:
        st, nb, out = encode(lib, slot, capacity)
        assert (st, nb) == (2, 0), capacity
    st, nb, out = encode(lib, slot, len(data))
    assert st == 0 and out[:nb].tobytes() == data


def test_host_coder_under_address_and_undefined_sanitizers(tmp_path):
    """jpeg_host.c and tests/jpegenc_host_check.c (its own main) compiled with -fsanitize=address,undefined and run: two slots coded into
    buffers of exactly the files' sizes, decoded back, and the refusal cases on heap copies of exactly the sizes passed."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present: sanitizer builds run on CPU-only machines")
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "jpegenc_host_check")
    subprocess.run([cc, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", CSRC,
                    os.path.join(CSRC, "jpeg_host.c"), os.path.join(ROOT, "tests", "jpegenc_host_check.c"), "-o", exe], check=True)
    args = []
    for i, (image, q) in enumerate(((jr.noise_image(37, 45, 1), 100), (jr.structured_image(40, 56, 2), 75))):
        slot_path, file_path = str(tmp_path / ("slot%d.bin" % i)), str(tmp_path / ("file%d.jpg" % i))
        jr.slot(image, q).tofile(slot_path)
        with open(file_path, "wb") as f:
            f.write(pillow_file(image, q))
        args += [slot_path, file_path]
    run = subprocess.run([exe] + args, capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
