"""CPU restatement of the device half of the hybrid PNG decode, written from the PNG specification (section 9, filtering), and a PNG
writer that forces a filter type per row and splits the IDAT stream -- what tests/test_png_host.py and tests/test_gpu_png.py build their
files with.  Pillow is the oracle of both: a hand-encoded file must read back identical through it, and unfilter() + to_rgb() must
equal its decode."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOUR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}        # channels -> colour type at bit depth 8
HEADER_BYTES = 1024


def chunk(ctype: bytes, data: bytes = b"", crc=None) -> bytes:
    c = zlib.crc32(ctype + data) if crc is None else crc
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", c & 0xFFFFFFFF)


def ihdr(width, height, depth=8, colour=2, compression=0, filter_method=0, interlace=0, crc=None) -> bytes:
    return chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, colour, compression, filter_method, interlace), crc)


def filter_rows(arr: np.ndarray, types) -> bytes:
    """uint8 [h][w][c] -> the scanlines with filter byte types[y] in front of row y (Filt(x) = Orig(x) - pred(a, b, c) mod 256)."""
    h, w, c = arr.shape
    x = arr.astype(np.int32)
    a = np.zeros_like(x)
    a[:, 1:] = x[:, :-1]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    cc = np.zeros_like(x)
    cc[1:, 1:] = x[:-1, :-1]
    p = a + b - cc
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - cc)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, cc))
    preds = [np.zeros_like(x), a, b, (a + b) >> 1, paeth]
    out = np.empty((h, 1 + w * c), dtype=np.uint8)
    for y in range(h):
        t = int(types[y])
        out[y, 0] = t
        out[y, 1:] = ((x[y] - (preds[t][y] if t <= 4 else 0)) & 255).reshape(-1)
    return out.tobytes()


def write_png(arr: np.ndarray, types=None, idat_chunks: int = 3, before_idat=(), between=None, after_idat=(), surplus: bytes = b"") -> bytes:
    """uint8 [h][w][c] (c = 1..4) -> file bytes.  types: filter type per row (default: y % 5); the zlib stream is cut into `idat_chunks`
    IDAT chunks; `surplus` is appended to the scanline data inside the zlib stream; extra chunks go before / between / after the IDATs."""
    h, w, c = arr.shape
    if types is None:
        types = [y % 5 for y in range(h)]
    z = zlib.compress(filter_rows(arr, types) + surplus, 6)
    n = max(1, min(idat_chunks, len(z)))
    cuts = [len(z) * i // n for i in range(n + 1)]
    parts = [chunk(b"IDAT", z[cuts[i]:cuts[i + 1]]) for i in range(n)]
    if between is not None:
        parts.insert(1, between)
    return SIGNATURE + ihdr(w, h, 8, COLOUR_TYPE[c]) + b"".join(before_idat) + b"".join(parts) + b"".join(after_idat) + chunk(b"IEND")


def unfilter(scan, width: int, height: int, channels: int) -> np.ndarray:
    """The inflated scanlines -> uint8 [h][w][channels]: Recon(x) = Filt(x) + pred(Recon(a), Recon(b), Recon(c)) mod 256."""
    stride = 1 + width * channels
    scan = bytes(scan)
    assert len(scan) == height * stride
    bpp = channels
    prev = bytearray(width * channels)
    rows = []
    for y in range(height):
        ft = scan[y * stride]
        line = bytearray(scan[y * stride + 1:(y + 1) * stride])
        if ft == 1:
            for i in range(bpp, len(line)):
                line[i] = (line[i] + line[i - bpp]) & 255
        elif ft == 2:
            for i in range(len(line)):
                line[i] = (line[i] + prev[i]) & 255
        elif ft == 3:
            for i in range(len(line)):
                a = line[i - bpp] if i >= bpp else 0
                line[i] = (line[i] + ((a + prev[i]) >> 1)) & 255
        elif ft == 4:
            for i in range(len(line)):
                a = line[i - bpp] if i >= bpp else 0
                b = prev[i]
                c = prev[i - bpp] if i >= bpp else 0
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                line[i] = (line[i] + (a if pa <= pb and pa <= pc else b if pb <= pc else c)) & 255
        else:
            assert ft == 0, ft
        rows.append(bytes(line))
        prev = line
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(height, width, channels)


def to_rgb(px: np.ndarray) -> np.ndarray:
    """uint8 [h][w][c] -> uint8 [h][w][3]: grey replicated, alpha composited over white with Pillow's rounding
    (t = 255 (255 - alpha) + v alpha + 128; ((t >> 8) + t) >> 8)."""
    c = px.shape[2]
    if c == 3:
        return px.copy()
    if c == 1:
        return np.repeat(px, 3, axis=2)
    v = px[:, :, :c - 1].astype(np.int64)
    al = px[:, :, c - 1:].astype(np.int64)
    t = 255 * (255 - al) + v * al + 128
    out = (((t >> 8) + t) >> 8).astype(np.uint8)
    return np.repeat(out, 3, axis=2) if c == 2 else out


def decode_slot(slot: np.ndarray) -> np.ndarray:
    """A slot of csrc/png_slot.h -> uint8 [h][w][3], what the device half must produce."""
    magic, kind, w, h, ch = (int(v) for v in slot[:20].view(np.int32))
    total = int(slot[32:40].view(np.int64)[0])
    assert magic == 0x20474E50 and kind == 2 and total == HEADER_BYTES + h * (1 + w * ch)
    return to_rgb(unfilter(slot[HEADER_BYTES:total], w, h, ch))


def pillow_rgb(data: bytes) -> np.ndarray:
    """What the decode workers hand on for this file (pipeline.decode_image before pad and resize)."""
    import io
    from PIL import Image
    img = Image.open(io.BytesIO(data))
    img.load()
    if img.mode in ("RGBA", "LA"):
        bg = Image.new("RGB", img.size, (255, 255, 255))
        bg.paste(img, mask=img.split()[-1])
        img = bg
    elif img.mode != "RGB":
        img = img.convert("RGB")
    return np.asarray(img, dtype=np.uint8)


MODES = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}


def noise(rng, h: int, w: int, c: int) -> np.ndarray:
    """Uniform noise (the worst case for Paeth ties); alpha takes 0 and 255 often."""
    a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if c in (2, 4):
        al = a[:, :, c - 1]
        pick = rng.integers(0, 4, (h, w))
        al[pick == 0] = 0
        al[pick == 1] = 255
    return a


def pillow_png(arr: np.ndarray, **kw) -> bytes:
    import io
    from PIL import Image
    c = arr.shape[2]
    buf = io.BytesIO()
    Image.fromarray(arr[:, :, 0] if c == 1 else arr, MODES[c]).save(buf, format="PNG", **kw)
    return buf.getvalue()
