"""The JPEG encoder's arithmetic, stated once in numpy: libjpeg-turbo as PIL.Image.save(..., "JPEG", quality=Q) drives it (4:2:0, three
components, baseline tables), all of it integers.  tests/test_jpegenc_reference.py pins this statement against Pillow's own files; the
GPU tests compare the device kernel (csrc/jpegenc.hip) with it.

  tables      jpeg_set_quality: s = 5000 // Q below 50, else 200 - 2 Q; clip((std * s + 50) // 100, 1, 255) of the Annex K tables
  colour      jccolor.c, 16 fractional bits
  edges       Y and full-resolution chroma are replicated to the right up to whole MCUs; chroma gets one replicated row when the height is
              odd, is downsampled (h2v2_downsample: bias 1, 2, 1, 2 along the output columns), and the DOWNSAMPLED rows are replicated
              down to whole blocks
  DCT         jfdctint.c (jpeg_fdct_islow) on samples - 128
  quantise    d = 8 q, t = |c| + d / 2, sign(c) * (t // d if t >= d else 0)
  filler      a luminance block wholly beyond ceil(w / 8) columns or ceil(h / 8) rows: AC zero, DC of the block before it in the MCU's
              coding order (top-left, top-right, bottom-left, bottom-right)

slot() lays the result out as csrc/jpeg_slot.h describes it.
"""
import numpy as np

STD_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
                     100, 103, 99], dtype=np.int64)
STD_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99,
                       99] + [99] * 32, dtype=np.int64)

HEADER_BYTES = 1024
MAGIC = 0x4745504a


def quant_tables(quality):
    """(luma, chroma): int64 [64] each, natural order"""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((t * s + 50) // 100, 1, 255) for t in (STD_LUMA, STD_CHROMA))


def _fix(x):
    return int(x * 65536 + 0.5)


def ycc(rgb):
    """uint8 [h, w, 3] -> Y, Cb, Cr as int64 [h, w]"""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(plane, rows, cols):
    return np.pad(plane, ((0, rows - plane.shape[0]), (0, cols - plane.shape[1])), mode="edge")


def planes(rgb):
    """the three sample planes the DCT sees: Y [16 my, 16 mx], Cb and Cr [8 my, 8 mx]"""
    h, w = rgb.shape[:2]
    mx, my = (w + 15) // 16, (h + 15) // 16
    y, cb, cr = ycc(rgb)
    out = [_pad(y, 16 * my, 16 * mx)]
    bias = np.tile(np.array([1, 2], dtype=np.int64), 4 * mx)
    for c in (cb, cr):
        c = _pad(c, h + (h & 1), 16 * mx)
        d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        out.append(_pad(d, 8 * my, 8 * mx))
    return out


F_0_298631336, F_0_390180644, F_0_541196100, F_0_765366865, F_0_899976223, F_1_175875602 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501321110, F_1_847759065, F_1_961570560, F_2_053119869, F_2_562915447, F_3_072711026 = 12299, 15137, 16069, 16819, 20995, 25172


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """one pass of jpeg_fdct_islow along the last axis of int64 [..., 8]"""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = np.empty_like(d)
    n = 11 if first else 15
    if first:
        out[..., 0] = (t10 + t11) << 2
        out[..., 4] = (t10 - t11) << 2
    else:
        out[..., 0] = _descale(t10 + t11, 2)
        out[..., 4] = _descale(t10 - t11, 2)
    z1 = (t12 + t13) * F_0_541196100
    out[..., 2] = _descale(z1 + t13 * F_0_765366865, n)
    out[..., 6] = _descale(z1 - t12 * F_1_847759065, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175875602
    t4, t5, t6, t7 = t4 * F_0_298631336, t5 * F_2_053119869, t6 * F_3_072711026, t7 * F_1_501321110
    z1, z2 = -z1 * F_0_899976223, -z2 * F_2_562915447
    z3, z4 = -z3 * F_1_961570560 + z5, -z4 * F_0_390180644 + z5
    out[..., 7] = _descale(t4 + z1 + z3, n)
    out[..., 5] = _descale(t5 + z2 + z4, n)
    out[..., 3] = _descale(t6 + z2 + z3, n)
    out[..., 1] = _descale(t7 + z1 + z4, n)
    return out


def fdct_quant(plane, q):
    """int64 [8 bh, 8 bw] samples -> int16 [bh, bw, 64] quantised coefficients, natural order"""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    d = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128            # [bh, bw, row, col]
    d = _fdct_pass(d, True)                                                # along the rows' samples
    d = _fdct_pass(d.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)   # along the columns
    c = d.reshape(bh, bw, 64)
    div = 8 * q
    t = np.abs(c) + (div >> 1)
    return (np.sign(c) * np.where(t >= div, t // div, 0)).astype(np.int16)


def coefficients(rgb, quality):
    """[Y, Cb, Cr] as int16 [blocks_h, blocks_w, 64], filler blocks included, and the two tables"""
    h, w = rgb.shape[:2]
    ql, qc = quant_tables(quality)
    py, pcb, pcr = planes(rgb)
    y = fdct_quant(py, ql)
    real_w, real_h = (w + 7) // 8, (h + 7) // 8
    for by in range(y.shape[0]):
        for bx in range(y.shape[1]):
            if by < real_h and bx < real_w:
                continue
            # the block before it in the MCU's coding order: the one to the left for a right-hand block, the top-right one for the bottom-left
            py_, px_ = (by, bx - 1) if bx & 1 else (by - 1, bx + 1)
            y[by, bx, :] = 0
            y[by, bx, 0] = y[py_, px_, 0]
    return [y, fdct_quant(pcb, qc), fdct_quant(pcr, qc)], (ql, qc)


def slot_bytes(width, height):
    """hipts_jpeg_slot_bytes"""
    return HEADER_BYTES + 3 * ((width + 15) // 16 * 2) * ((height + 15) // 16 * 2) * 128


def slot(rgb, quality):
    """uint8 [total_bytes]: the slot (csrc/jpeg_slot.h) the encoder writes for this image"""
    h, w = rgb.shape[:2]
    comps, (ql, qc) = coefficients(rgb, quality)
    mx, my = (w + 15) // 16, (h + 15) // 16
    head = np.zeros(HEADER_BYTES // 4, dtype=np.int32)
    head[:8] = [MAGIC, 1, w, h, 3, 2, 2, 0]
    off = 0
    for c in range(3):
        f = 2 if c == 0 else 1
        head[8 + 8 * c:16 + 8 * c] = [f, f, mx * f, my * f, w if c == 0 else (w + 1) // 2, h if c == 0 else (h + 1) // 2, off, 0]
        off += mx * f * my * f * 64
    raw = head.view(np.uint8).copy()
    raw[128:512] = np.concatenate([ql, qc, qc]).astype(np.uint16).view(np.uint8)
    total = HEADER_BYTES + 2 * off
    raw[512:520] = np.array([total], dtype=np.int64).view(np.uint8)
    return np.concatenate([raw] + [c.reshape(-1).view(np.uint8) for c in comps])


def parse(slot_u8):
    """(header fields as a dict, [Y, Cb, Cr] int16 [blocks_h, blocks_w, 64], quant uint16 [3, 64]) of a slot"""
    s = np.ascontiguousarray(slot_u8)
    head = s[:128].view(np.int32)
    f = dict(zip(("magic", "kind", "width", "height", "ncomp", "hmax", "vmax", "reserved"), head[:8].tolist()))
    f["comp"] = [head[8 + 8 * c:16 + 8 * c].tolist() for c in range(3)]
    f["total_bytes"] = int(s[512:520].view(np.int64)[0])
    coef = s[HEADER_BYTES:f["total_bytes"]].view(np.int16)
    comps = []
    for c in range(f["ncomp"]):
        _, _, bw, bh, _, _, off, _ = f["comp"][c]
        comps.append(coef[off:off + bw * bh * 64].reshape(bh, bw, 64))
    return f, comps, s[128:512].view(np.uint16).reshape(3, 64)


# ---- test content


def noise_image(h, w, seed=0):
    return np.random.default_rng(seed * 100003 + h * 1009 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def structured_image(h, w, seed=0):
    """smooth colour gradients, a hard edge and a little noise: few non-zero coefficients, long zero runs"""
    rng = np.random.default_rng(7 + seed * 100003 + h * 1009 + w)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.stack([127 + 120 * np.sin(xx / 9.0 + seed) * np.cos(yy / 13.0), 255 * xx / max(1, w - 1), 255 * yy / max(1, h - 1)], axis=-1)
    a[h // 3:, w // 2:] = 255 - a[h // 3:, w // 2:]
    a += rng.integers(-3, 4, (h, w, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


def white_image(h, w):
    return np.full((h, w, 3), 255, dtype=np.uint8)


def saturated_image(h, w):
    """primary colours in hard-edged patches: the largest chroma swings and coefficients"""
    a = np.zeros((h, w, 3), dtype=np.uint8)
    a[:h // 2, :w // 2] = (255, 0, 0)
    a[:h // 2, w // 2:] = (0, 255, 0)
    a[h // 2:, :w // 2] = (0, 0, 255)
    a[h // 2:, w // 2:] = (255, 255, 255)
    a[h // 4:h // 4 + 3, ::2] = (255, 0, 255)
    return a
