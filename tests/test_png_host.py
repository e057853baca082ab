"""CPU: the host half of the hybrid PNG decode (hiptagsearch/png_host.py).  It takes only completely regular files -- then the slot holds
exactly what zlib gives for the IDAT stream, and undoing the filters (tests/png_ref.py, from the PNG specification) gives the bytes the
Pillow worker hands on -- and refuses everything else with the status codes of hipts_jpeg_entropy_decode, leaving the verdict on the
file to Pillow."""
import os
import struct
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_ref  # noqa: E402
from png_ref import SIGNATURE, chunk, ihdr  # noqa: E402


def _idat_payload(data: bytes) -> bytes:
    pos, out = 8, []
    while pos < len(data):
        n, = struct.unpack_from(">I", data, pos)
        if data[pos + 4:pos + 8] == b"IDAT":
            out.append(data[pos + 8:pos + 8 + n])
        pos += 12 + n
    return zlib.decompress(b"".join(out))


def _inflate(data: bytes, nbytes=None):
    from hiptagsearch import png_host
    slot = np.full(nbytes if nbytes is not None else 1 << 20, 0xAB, dtype=np.uint8)
    return png_host.png_inflate_into(data, slot), slot


def _old_path(tmp_path, data: bytes):
    from hiptagsearch import pipeline
    p = str(tmp_path / "file.png")
    with open(p, "wb") as f:
        f.write(data)
    return pipeline.decode_image(p, 448, pipeline.TAGGER, raw_max_pixels=1 << 24)


def _smooth(rng, h, w, c):
    small = rng.integers(0, 256, (max(2, h // 8), max(2, w // 8), c), dtype=np.uint8)
    big = np.stack([np.asarray(Image.fromarray(small[:, :, k]).resize((w, h), Image.BICUBIC)) for k in range(c)], axis=2).astype(np.int16)
    return np.clip(big + rng.integers(-8, 9, big.shape), 0, 255).astype(np.uint8)


def _regular_files():
    rng = np.random.default_rng(11)
    for c in (1, 2, 3, 4):
        yield "pillow noise %d" % c, c, (37, 53), png_ref.pillow_png(png_ref.noise(rng, 37, 53, c))
        yield "pillow smooth %d" % c, c, (90, 120), png_ref.pillow_png(_smooth(rng, 90, 120, c))      # the adaptive filter mixes the types
        yield "hand %d" % c, c, (70, 131), png_ref.write_png(png_ref.noise(rng, 70, 131, c), idat_chunks=3)
    yield "ancillary chunks", 3, (9, 7), png_ref.write_png(png_ref.noise(rng, 9, 7, 3), before_idat=[chunk(b"gAMA", struct.pack(">I", 45455)),
                                                                                                      chunk(b"tEXt", b"Comment\0hello")],
                                                           after_idat=[chunk(b"tIME", bytes(7))])


def test_regular_files_fill_the_slot_with_what_zlib_gives(tmp_path):
    from hiptagsearch import png_host
    n = 0
    for name, c, (h, w), data in _regular_files():
        st, slot = _inflate(data)
        assert st == 0, name
        hd = slot[:32].view(np.int32)
        total = int(slot[32:40].view(np.int64)[0])
        assert [int(v) for v in hd[:5]] == [png_host.MAGIC, 2, w, h, c], name
        assert total == png_host.HEADER_BYTES + h * (1 + w * c) == png_host.slot_bytes(w, h, c), name
        assert slot[png_host.HEADER_BYTES:total].tobytes() == _idat_payload(data), name
        assert int(slot[total]) == 0xAB, name                              # nothing written behind the scanlines
        want = _old_path(tmp_path, data)
        got = png_ref.decode_slot(slot)
        assert want is not None and got.shape == want.shape == (h, w, 3) and np.array_equal(got, want), name
        assert np.array_equal(want, png_ref.pillow_rgb(data)), name
        # a slot of exactly the right size is enough, one byte less is not
        assert _inflate(data, total)[0] == 0 and _inflate(data, total - 1)[0] == 2, name
        n += 1
    assert n == 13


def test_hand_encoded_file_reads_back_through_pillow_and_uses_every_filter():
    rng = np.random.default_rng(2)
    for c in (1, 2, 3, 4):
        arr = png_ref.noise(rng, 70, 131, c)
        data = png_ref.write_png(arr, idat_chunks=3)
        assert data.count(b"IDAT") >= 3
        import io
        back = np.asarray(Image.open(io.BytesIO(data)))
        assert np.array_equal(back.reshape(70, 131, c), arr)
        scan = np.frombuffer(_idat_payload(data), dtype=np.uint8).reshape(70, 1 + 131 * c)
        assert sorted(set(scan[:, 0].tolist())) == [0, 1, 2, 3, 4]
        assert np.array_equal(png_ref.unfilter(scan.tobytes(), 131, 70, c), arr)


def _raw_file(w, h, colour, raw, depth=8, interlace=0, extra=(), ihdr_crc=None, end=True):
    return (SIGNATURE + ihdr(w, h, depth, colour, interlace=interlace, crc=ihdr_crc) + b"".join(extra) + chunk(b"IDAT", zlib.compress(raw))
            + (chunk(b"IEND") if end else b""))


def _refusals():
    """(name, file bytes, status, what the Pillow path does with the file: True decodes, False drops)"""
    import io
    rng = np.random.default_rng(3)
    rgb = png_ref.noise(rng, 20, 30, 3)
    scan = png_ref.filter_rows(rgb, [y % 5 for y in range(20)])
    good = png_ref.write_png(rgb, idat_chunks=2)
    buf = io.BytesIO()
    Image.fromarray(rng.integers(0, 65536, (20, 30), dtype=np.uint16)).save(buf, format="PNG")
    yield "16-bit grey", buf.getvalue(), 1, True
    yield "16-bit RGB", _raw_file(30, 20, 2, b"".join(b"\0" + rng.integers(0, 256, 30 * 6, dtype=np.uint8).tobytes() for _ in range(20)), depth=16), 1, True
    pal = Image.fromarray(rgb).convert("P", palette=Image.ADAPTIVE, colors=16)
    buf = io.BytesIO()
    pal.save(buf, format="PNG")
    yield "palette", buf.getvalue(), 1, True
    buf = io.BytesIO()
    pal.save(buf, format="PNG", transparency=0)
    assert b"tRNS" in buf.getvalue()
    yield "palette + tRNS", buf.getvalue(), 1, True
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="PNG", transparency=(1, 2, 3))
    assert b"tRNS" in buf.getvalue()
    yield "RGB + tRNS", buf.getvalue(), 1, True
    yield "interlace flag set", _raw_file(30, 20, 2, scan, interlace=1), 1, None
    yield "an acTL chunk", png_ref.write_png(rgb, before_idat=[chunk(b"acTL", struct.pack(">II", 1, 0))]), 1, True
    yield "an unknown critical chunk", png_ref.write_png(rgb, before_idat=[chunk(b"ABCD", b"xyz")]), 1, True
    yield "surplus bytes after the last row", png_ref.write_png(rgb, surplus=bytes(50)), 1, True
    yield "not a PNG", b"not a png at all, not even close", 1, False
    wide = png_ref.noise(rng, 1, 8193, 3)
    yield "width over the kernel's limit", png_ref.write_png(wide, types=[1]), 1, True
    yield "IDAT chunks not consecutive", png_ref.write_png(rgb, idat_chunks=2, between=chunk(b"tEXt", b"k\0v")), 1, None
    # a flipped byte inside the compressed data, with and without the chunk's CRC repaired
    pos = good.index(b"IDAT") + 4
    n, = struct.unpack_from(">I", good, pos - 8)
    body = bytearray(good[pos:pos + n])
    body[n // 2] ^= 0x10
    flipped = good[:pos] + bytes(body) + good[pos + n:]
    yield "flipped IDAT byte", flipped, 3, False
    yield "flipped IDAT byte, CRC repaired", good[:pos - 8] + chunk(b"IDAT", bytes(body)) + good[pos + n + 4:], 3, False
    yield "bad IHDR CRC", _raw_file(30, 20, 2, scan, ihdr_crc=12345), 3, False
    yield "filter byte 5", png_ref.write_png(rgb, types=[5 if y == 7 else y % 5 for y in range(20)]), 3, False
    yield "short data", _raw_file(30, 20, 2, scan[:-91 * 2]), 3, True                 # a complete stream two rows short: Pillow leaves them black
    z = zlib.compress(scan)
    yield "short data, stream cut", SIGNATURE + ihdr(30, 20, 8, 2) + chunk(b"IDAT", z[:len(z) // 2]) + chunk(b"IEND"), 3, False
    yield "file cut in half", good[:len(good) // 2], 3, False
    yield "missing IEND", good[:-12], 3, True


def test_everything_else_is_refused_and_left_to_pillow(tmp_path):
    seen = []
    for name, data, status, old in _refusals():
        st, slot = _inflate(data)
        assert st == status, (name, st)
        got = _old_path(tmp_path, data)
        if old is not None:
            assert (got is not None) == old, name
        seen.append(name)
    assert len(seen) == 20, seen
    # the slot one byte short, with an otherwise regular file
    good = png_ref.write_png(png_ref.noise(np.random.default_rng(4), 20, 30, 4))
    need = 1024 + 20 * (1 + 30 * 4)
    assert _inflate(good, need)[0] == 0 and _inflate(good, need - 1)[0] == 2


def test_inflate_is_bounded_by_the_image_size(monkeypatch):
    """A zlib stream that inflates to far more than h (1 + w c) bytes never produces more than max_length = that + 1 bytes."""
    from hiptagsearch import png_host
    lengths = []

    class Spy:
        def __init__(self):
            self._d = zlib.decompressobj()

        def decompress(self, data, max_length=0):
            out = self._d.decompress(data, max_length)
            lengths.append((max_length, len(out)))
            return out

        def __getattr__(self, k):
            return getattr(self._d, k)

    class Zlib:
        error, crc32 = zlib.error, staticmethod(zlib.crc32)
        decompressobj = staticmethod(Spy)

    monkeypatch.setattr(png_host, "zlib", Zlib)
    bomb = SIGNATURE + ihdr(4, 4, 8, 2) + chunk(b"IDAT", zlib.compress(bytes(50_000_000), 9)) + chunk(b"IEND")
    assert len(bomb) < 100_000
    st, _ = _inflate(bomb)
    assert st == 1                                    # surplus data: Pillow's to judge
    expected = 4 * (1 + 4 * 3)
    assert lengths and all(ml == expected + 1 and n <= expected + 1 for ml, n in lengths)
