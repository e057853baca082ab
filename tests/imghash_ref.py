"""Shared by test_imghash_reference.py, test_gpu_imghash.py, test_gpu_hamming.py and test_gpu_find_duplicates.py: a pure-numpy
restatement of the image hash and of the Hamming relation, and the corpus the near-duplicate tests use.  Nothing here imports the package.

Hash         uint64 [2] per image uint8 [S,S,3], all of it integer arithmetic:
               grey      g = (19595 R + 38470 G + 7471 B + 0x8000) >> 16                      (Pillow's convert("L"))
               grids     Rr rows x Cc columns, boundaries floor(k S / Rr) and floor(k S / Cc); sum(r, c) over a cell, area(r, c) its pixels
               brighter  cell b is brighter than cell a  <=>  sum(b) area(a) > sum(a) area(b)  (exact: Python ints / int64)
               word 0    grid 8 x 9, bit 8 r + c: cell (r, c + 1) is brighter than cell (r, c)
               word 1    grid 9 x 8, bit 8 r + c: cell (r + 1, c) is brighter than cell (r, c)
Relation     j in N(i)  <=>  popcount(h_i[0] ^ h_j[0]) + popcount(h_i[1] ^ h_j[1]) <= T, for every j (j == i included).
Groups       cluster_ref.dbscan_ref with min_samples = 2 on that relation: the connected components of the rows that have another
             neighbour, numbered by their smallest row; every other row -1.
"""
import io

import numpy as np

from cluster_ref import dbscan_ref, lists_of  # noqa: F401  (lists_of is reused by the tests as it is)

SAME_MAX = 10                # the CLI's default max_distance: copies of one picture must lie within it ...
DIFFERENT_MIN = 2 * SAME_MAX  # ... and different pictures beyond twice that (asserted on the corpus, not assumed)


def grey(images):
    """int64 [..., S, S] from uint8 [..., S, S, 3]"""
    a = np.asarray(images).astype(np.int64)
    return (19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16


def bounds(size, parts):
    return [k * size // parts for k in range(parts + 1)]


def cell_sums(g, rows, cols):
    """(sum int64 [rows, cols], area int64 [rows, cols]) of one grey image [S, S]"""
    size = g.shape[0]
    rb, cb = bounds(size, rows), bounds(size, cols)
    s = np.zeros((rows, cols), dtype=np.int64)
    a = np.zeros((rows, cols), dtype=np.int64)
    for r in range(rows):
        for c in range(cols):
            s[r, c] = g[rb[r]:rb[r + 1], cb[c]:cb[c + 1]].sum()
            a[r, c] = (rb[r + 1] - rb[r]) * (cb[c + 1] - cb[c])
    return s, a


def hash128(images):
    """uint64 [n, 2] of uint8 [n, S, S, 3]"""
    images = np.asarray(images)
    assert images.ndim == 4 and images.shape[1] == images.shape[2] and images.shape[3] == 3 and images.dtype == np.uint8
    out = np.zeros((len(images), 2), dtype=np.uint64)
    for n, g in enumerate(grey(images)):
        sh, ah = cell_sums(g, 8, 9)
        sv, av = cell_sums(g, 9, 8)
        w0 = w1 = 0
        for r in range(8):
            for c in range(8):
                if int(sh[r, c + 1]) * int(ah[r, c]) > int(sh[r, c]) * int(ah[r, c + 1]):
                    w0 |= 1 << (8 * r + c)
                if int(sv[r + 1, c]) * int(av[r, c]) > int(sv[r, c]) * int(av[r + 1, c]):
                    w1 |= 1 << (8 * r + c)
        out[n] = (w0, w1)
    return out


def hamming(H):
    """int64 [n, n]: differing bits of the 128-bit rows of uint64 [n, 2]"""
    H = np.ascontiguousarray(H, dtype=np.uint64).reshape(-1, 2)
    bits = np.unpackbits(H.view(np.uint8).reshape(len(H), 16), axis=1).astype(np.int64)
    ones = bits.sum(axis=1)
    return ones[:, None] + ones[None, :] - 2 * (bits @ bits.T)


def set_bits(H):
    H = np.ascontiguousarray(H, dtype=np.uint64).reshape(-1, 2)
    return np.unpackbits(H.view(np.uint8).reshape(len(H), 16), axis=1).sum(axis=1).astype(np.int64)


def groups_ref(H, max_distance, min_set_bits=0):
    """labels int32 [n] by the definition at the top; rows with fewer than min_set_bits set bits are left out and get -1"""
    H = np.ascontiguousarray(H, dtype=np.uint64).reshape(-1, 2)
    labels = np.full(len(H), -1, dtype=np.int32)
    keep = np.flatnonzero(set_bits(H) >= min_set_bits)
    if len(keep):
        labels[keep] = dbscan_ref(hamming(H[keep]) <= max_distance, 2)
    return labels


def flip_bits(row, positions):
    """a copy of the uint64 [2] row with the given bits (0..127; 64.. are word 1) inverted"""
    out = np.array(row, dtype=np.uint64).copy()
    for p in positions:
        out[p // 64] ^= np.uint64(1) << np.uint64(p % 64)
    return out


# ---- constructed images, with the hash each must have by the definition (not by hash128) ------------------------------------------
ALL64 = (1 << 64) - 1


def flat_image(size, value=200):
    return np.full((size, size, 3), value, dtype=np.uint8)


def ramp_image(size, horizontal):
    """grey rises strictly from cell to cell along one axis and is constant along the other (R = G = B = v gives g = v)"""
    v = (np.arange(size) * 255 // (size - 1)).astype(np.uint8)
    g = np.broadcast_to(v[None, :] if horizontal else v[:, None], (size, size))
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


def equal_mean_pair(size=100):
    """(image, image with one pixel raised): at size 100 the cells (0, 7) and (0, 8) of the 8 x 9 grid are 12 x 11 and 12 x 12 pixels.
    The left one alternates 90 / 110 (66 pixels each: sum 13200 over 132 pixels), everything else is 100 (sum 14400 over 144 pixels):
    13200 * 144 == 14400 * 132, the means are equal and bit 7 of word 0 is clear although the right SUM is larger.  One pixel of the
    right cell raised by 1 makes it brighter: bit 7 is set, and it is the only bit of word 0."""
    assert size == 100 and bounds(100, 9)[7:] == [77, 88, 100] and bounds(100, 8)[:2] == [0, 12]
    a = np.full((size, size), 100, dtype=np.uint8)
    yy, xx = np.mgrid[0:12, 77:88]
    a[0:12, 77:88] = np.where((yy + xx) % 2 == 0, 90, 110)
    b = a.copy()
    b[5, 95] += 1
    return np.repeat(a[:, :, None], 3, axis=2), np.repeat(b[:, :, None], 3, axis=2)


def saturated_image(size, value, cell=(3, 4)):
    """all 255 except cell (r, c) of the 8 x 9 grid, which holds `value`: the largest sums and products the comparison meets"""
    a = np.full((size, size, 3), 255, dtype=np.uint8)
    rb, cb = bounds(size, 8), bounds(size, 9)
    a[rb[cell[0]]:rb[cell[0] + 1], cb[cell[1]]:cb[cell[1] + 1]] = value
    return a


# ---- the corpus ---------------------------------------------------------------------------------------------------------------------
def tagger_input(img, size=448):
    """the tagger's own input of a PIL image: composite over white, centred pad to a square, bicubic resize -> uint8 [size, size, 3]"""
    from PIL import Image
    if img.mode in ("RGBA", "LA"):
        bg = Image.new("RGB", img.size, (255, 255, 255))
        bg.paste(img, mask=img.split()[-1])
        img = bg
    else:
        img = img.convert("RGB")
    w, h = img.size
    m = max(w, h)
    padded = Image.new("RGB", (m, m), (255, 255, 255))
    padded.paste(img, ((m - w) // 2, (m - h) // 2))
    if padded.size != (size, size):
        padded = padded.resize((size, size), Image.BICUBIC)
    return np.asarray(padded, dtype=np.uint8)


def synthetic_picture(rng, width=512, height=384):
    """a PIL RGB picture: a 8 x 6 random field upsampled bicubically, plus uniform noise of +-6"""
    from PIL import Image
    field = Image.fromarray(rng.integers(0, 256, (6, 8, 3), dtype=np.uint8), "RGB").resize((width, height), Image.BICUBIC)
    noisy = np.asarray(field, dtype=np.int16) + rng.integers(-6, 7, (height, width, 3), dtype=np.int16)
    return Image.fromarray(np.clip(noisy, 0, 255).astype(np.uint8), "RGB")


def near_duplicate_corpus(seed, pictures=5, singles=3):
    """[(file name, picture id, file bytes)]: every one of `pictures` pictures as the original (PNG), a copy resized to 320 x 240
    (PNG) and a JPEG-quality-75 copy of the original; then `singles` unrelated pictures (PNG).  The singles have ids of their own: two
    entries show the same picture exactly when their ids agree."""
    from PIL import Image
    rng = np.random.default_rng(seed)

    def encoded(img, fmt, **kw):
        buf = io.BytesIO()
        img.save(buf, fmt, **kw)
        return buf.getvalue()
    out = []
    for p in range(pictures + singles):
        pic = synthetic_picture(rng)
        out.append(("pic%02d_orig.png" % p, p, encoded(pic, "PNG")))
        if p >= pictures:
            continue
        out.append(("pic%02d_small.png" % p, p, encoded(pic.resize((320, 240), Image.BICUBIC), "PNG")))
        out.append(("pic%02d_q75.jpg" % p, p, encoded(pic, "JPEG", quality=75)))
    return out


def corpus_inputs(corpus, size=448):
    """uint8 [n, size, size, 3]: every file decoded by Pillow and taken through tagger_input"""
    from PIL import Image
    return np.stack([tagger_input(Image.open(io.BytesIO(data)), size) for _, _, data in corpus])


def assert_separation(H, ids):
    """the condition the near-duplicate tests rest on: same picture <= SAME_MAX bits apart, different pictures > DIFFERENT_MIN"""
    d = hamming(H)
    ids = np.asarray(ids)
    same = ids[:, None] == ids[None, :]
    assert d[same].max() <= SAME_MAX, "copies of one picture lie %d bits apart" % d[same].max()
    assert d[~same].min() > DIFFERENT_MIN, "two different pictures lie only %d bits apart" % d[~same].min()
    return int(d[same].max()), int(d[~same].min())
