"""Host half of the hybrid PNG decode (csrc/png_slot.h describes the split; csrc/png.hip is the device half).

Runs in the decode worker processes and uses only struct, zlib and numpy.  It walks the chunk stream of a PNG file, takes it only if it is
completely regular, and inflates the IDAT stream -- the serial bit stream of the format -- into a ring slot: a 1024-byte header, then the
scanlines as zlib returned them, filter bytes included.  Undoing the filters, grey -> RGB and the composite over white happen on the device.

The rule: take only what is regular and never judge a file dropped.  On every status but 0 the caller decodes the file with Pillow as
before, so Pillow alone decides whether a file decodes."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAGIC = 0x20474E50            # HIPTS_PNG_MAGIC, "PNG "
KIND = 2
HEADER_BYTES = 1024           # HIPTS_PNG_HEADER_BYTES
MAX_WIDTH = 8192              # HIPTS_PNG_MAX_WIDTH: two LDS row buffers of 4 * width bytes in the kernel

OK, NOT_TAKEN, SLOT_TOO_SMALL, IRREGULAR = 0, 1, 2, 3       # the status codes of hipts_jpeg_entropy_decode

_CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}        # colour type -> bytes per pixel at bit depth 8
# ancillary chunks that Pillow lets change no pixel; PLTE, tRNS, the APNG chunks and everything unknown send the file to Pillow
_IGNORED = frozenset((b"gAMA", b"cHRM", b"sRGB", b"iCCP", b"pHYs", b"tEXt", b"zTXt", b"iTXt", b"tIME", b"bKGD", b"eXIf", b"sBIT"))


def slot_bytes(width: int, height: int, channels: int = 4) -> int:
    """Bytes of the slot of a width x height image."""
    return HEADER_BYTES + height * (1 + width * channels)


def png_inflate_into(data: bytes, slot: np.ndarray) -> int:
    """File bytes -> slot (uint8, contiguous).  0: the slot is filled; 1: not a file the fast path takes; 2: the slot is too small;
    3: the stream is irregular."""
    if len(data) < 8 or data[:8] != SIGNATURE:
        return NOT_TAKEN
    view = memoryview(data)
    n = len(data)
    pos = 8
    first = True
    idat = []
    idat_over = False
    seen_end = False
    width = height = channels = 0
    while pos < n:
        if pos + 12 > n:
            return IRREGULAR
        length, = struct.unpack_from(">I", data, pos)
        ctype = data[pos + 4:pos + 8]
        end = pos + 12 + length
        if end > n:
            return IRREGULAR
        if first and (ctype != b"IHDR" or length != 13):
            return NOT_TAKEN
        if zlib.crc32(view[pos + 4:end - 4]) != struct.unpack_from(">I", data, end - 4)[0]:
            return IRREGULAR
        if first:
            width, height, depth, colour, compression, filter_method, interlace = struct.unpack_from(">IIBBBBB", data, pos + 8)
            if depth != 8 or colour not in _CHANNELS or compression != 0 or filter_method != 0 or interlace != 0:
                return NOT_TAKEN
            if width < 1 or height < 1 or width > MAX_WIDTH or height > 0x7FFFFFFF:
                return NOT_TAKEN
            channels = _CHANNELS[colour]
            first = False
        elif ctype == b"IDAT":
            if idat_over:
                return NOT_TAKEN
            idat.append(view[pos + 8:end - 4])
        elif ctype == b"IEND":
            seen_end = True
            break
        elif ctype in _IGNORED:
            idat_over = bool(idat)         # the IDAT chunks must be consecutive
        else:
            return NOT_TAKEN
        pos = end
    if not seen_end or not idat:
        return IRREGULAR
    stride = 1 + width * channels
    expected = height * stride
    if HEADER_BYTES + expected > slot.nbytes:
        return SLOT_TOO_SMALL
    inflater = zlib.decompressobj()
    try:
        out = inflater.decompress(idat[0] if len(idat) == 1 else b"".join(idat), expected + 1)
    except zlib.error:
        return IRREGULAR
    if len(out) > expected or inflater.unconsumed_tail:
        return NOT_TAKEN            # surplus scanline data: Pillow accepts it
    if len(out) < expected or not inflater.eof:
        return IRREGULAR
    if inflater.unused_data:
        return NOT_TAKEN
    lines = np.frombuffer(out, dtype=np.uint8)
    if int(lines.reshape(height, stride)[:, 0].max()) > 4:
        return IRREGULAR
    flat = slot.reshape(-1)
    head = flat[:HEADER_BYTES]
    head[:] = 0
    head[:32].view(np.int32)[:5] = (MAGIC, KIND, width, height, channels)
    head[32:40].view(np.int64)[0] = HEADER_BYTES + expected
    flat[HEADER_BYTES:HEADER_BYTES + expected] = lines
    return OK
