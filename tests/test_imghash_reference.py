"""CPU: pins tests/imghash_ref.py, the numpy restatement the GPU tests of the image hash and of the Hamming relation are held against --
the grey formula to Pillow, hash128 to images whose hash follows from the definition by hand, the separation of the near-duplicate
corpus (asserted, not assumed), and the groups to scipy's connected components."""
import numpy as np
import pytest

import imghash_ref as ir


def test_grey_equals_pillow():
    from PIL import Image
    rgb = np.random.default_rng(1).integers(0, 256, (97, 131, 3), dtype=np.uint8)
    rgb[0, :6] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 1, 1]]
    want = np.asarray(Image.fromarray(rgb, "RGB").convert("L"))
    np.testing.assert_array_equal(ir.grey(rgb), want)


@pytest.mark.parametrize("size", [9, 100, 448])
def test_flat_image_sets_no_bit(size):
    assert ir.hash128(ir.flat_image(size)[None]).tolist() == [[0, 0]]


@pytest.mark.parametrize("size", [9, 100, 448])
def test_ramps_set_one_whole_word(size):
    got = ir.hash128(np.stack([ir.ramp_image(size, True), ir.ramp_image(size, False)]))
    assert got.tolist() == [[ir.ALL64, 0], [0, ir.ALL64]]


def test_equal_means_of_unequal_areas_compare_exactly():
    a, b = ir.equal_mean_pair()
    ha, hb = ir.hash128(np.stack([a, b]))
    assert int(ha[0]) == 0                       # equal means although the sums differ: 13200 / 132 == 14400 / 144
    assert int(hb[0]) == 1 << 7                  # one grey level in one pixel decides
    sums, areas = ir.cell_sums(ir.grey(a), 8, 9)
    assert (int(sums[0, 7]), int(areas[0, 7]), int(sums[0, 8]), int(areas[0, 8])) == (13200, 132, 14400, 144)


def test_saturated_cells():
    for value in (254, 0):
        h = ir.hash128(ir.saturated_image(72, value)[None])[0]
        # the dark cell (3, 4): its right neighbour is brighter (bit 8 * 3 + 4), it is not brighter than its left one; the cell below it
        # in the 9 x 8 grid overlaps it differently, so only word 0 is stated here
        assert int(h[0]) == 1 << (8 * 3 + 4)


def test_hamming_counts_both_words():
    H = np.array([[0, 0], [0b1011, 0], [0, 1 << 63], [ir.ALL64, ir.ALL64]], dtype=np.uint64)
    assert ir.hamming(H).tolist() == [[0, 3, 1, 128], [3, 0, 4, 125], [1, 4, 0, 127], [128, 125, 127, 0]]
    assert ir.set_bits(H).tolist() == [0, 3, 1, 128]
    assert ir.flip_bits(H[0], [0, 64, 127]).tolist() == [1, (1 << 63) | 1]


@pytest.fixture(scope="module")
def corpus():
    c = ir.near_duplicate_corpus(20260301)
    return c, ir.hash128(ir.corpus_inputs(c))


def test_corpus_separates(corpus):
    c, H = corpus
    assert len(c) == 18
    same, different = ir.assert_separation(H, [pid for _, pid, _ in c])
    print("same picture: at most %d bits; different pictures: at least %d bits" % (same, different))
    assert (ir.set_bits(H) >= 8).all()           # none of them is a flat picture


def test_groups_equal_connected_components(corpus):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    c, H = corpus
    rng = np.random.default_rng(2)
    H = H[rng.permutation(len(H))]
    for T in (0, 10, 30, 60):
        rel = ir.hamming(H) <= T
        got = ir.groups_ref(H, T)
        _, comp = connected_components(csr_matrix(rel), directed=False)
        size = np.bincount(comp)[comp]
        assert ((got >= 0) == (size > 1)).all()
        first = {}
        for i in np.flatnonzero(size > 1):           # ascending: components numbered by their smallest row
            first.setdefault(int(comp[i]), len(first))
            assert got[i] == first[int(comp[i])]
    pid = np.array([p for _, p, _ in c])
    want = ir.groups_ref(ir.hash128(ir.corpus_inputs(c)), ir.SAME_MAX)
    assert want.tolist() == [p if p < 5 else -1 for p in pid]       # the planted groups, the singles alone


def test_min_set_bits_leaves_flat_rows_out():
    H = np.array([[0, 0], [0xff00ff, 0xff], [0, 1], [0xff00ff, 0xfe], [3, 0]], dtype=np.uint64)
    assert ir.groups_ref(H, 10, 0).tolist() == [0, 1, 0, 1, 0]      # the sparse rows pair with each other
    assert ir.groups_ref(H, 10, 8).tolist() == [-1, 0, -1, 0, -1]
