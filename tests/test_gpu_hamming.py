"""GPU: ImageHashIndex.neighbors / .groups (hipts_radius_create_hamming: hamming_pairs_kernel of csrc/radius.hip, and everything
hipts_radius_* shares with the cosine relation) against tests/imghash_ref.py -- numpy on the unpacked bits, pinned by
test_imghash_reference.py.  Integer arithmetic: the lists are compared exactly.

Rows are random 128-bit values: two of them lie within 10 bits of each other with negligible probability (their distance is binomial
around 64), so at T <= 10 every hit is a planted one -- a copy with exactly T flipped bits next to one with exactly T + 1 -- while at
T = 64 about half of all pairs are hits.  The sizes: one block of 256 rows and less, the exact block edge, two blocks with a ragged
second one, three blocks with off-diagonal pairs on both sides.
"""
import ctypes

import numpy as np
import pytest

import cluster_ref as cr
import imghash_ref as ir

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 255, 256, 257, 545]
# (row, its copy at distance T, its copy at distance T + 1, the words the flips go to): partners in the same block, at the block edge, in
# the next block, two blocks on, and the first and the last row (negative rows count from the end)
PLANTS = [(0, -1, -2, "both"), (3, 7, 9, "word0"), (10, 261, 262, "word1"), (250, 252, 251, "both"), (300, 542, 513, "both"),
          (20, 540, 530, "word1"), (100, 101, 400, "word0")]


def _random_rows(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 64, (n, 2), dtype=np.uint64)


def _flipped(row, count, words, rng):
    """`row` with exactly `count` bits inverted: all in word 0, all in word 1, or spread over both with at least one in each"""
    if words == "word0" and count <= 64:
        pos = rng.choice(64, count, replace=False)
    elif words == "word1" and count <= 64:
        pos = 64 + rng.choice(64, count, replace=False)
    elif count >= 2:
        k = int(rng.integers(max(1, count - 64), min(64, count - 1) + 1))
        pos = np.concatenate([rng.choice(64, k, replace=False), 64 + rng.choice(64, count - k, replace=False)])
    else:
        pos = rng.choice(128, count, replace=False)
    return ir.flip_bits(row, [int(p) for p in pos])


def _planted(n, T, seed=7):
    H = _random_rows(n, seed + n)
    rng = np.random.default_rng(seed)
    used = set()
    for a, b, c, words in PLANTS:
        a, b, c = (x % n if x < 0 else x for x in (a, b, c))
        if max(a, b) >= n or a == b or {a, b} & used:
            continue
        H[b] = _flipped(H[a], T, words, rng)
        used |= {a, b}
        if c < n and c not in used:
            H[c] = _flipped(H[a], T + 1, words, rng)
            used.add(c)
    return H


def _index(H):
    from hiptagsearch.dedup import ImageHashIndex
    index = ImageHashIndex()
    index.add(["img%05d.png" % i for i in range(len(H))], H)
    return index


def _assert_lists(ptr, ids, rel):
    """the checks of test_gpu_cluster.py"""
    n = len(rel)
    want_ptr, want_ids = ir.lists_of(rel)
    assert ptr.dtype == np.int64 and ids.dtype == np.int32 and ptr.shape == (n + 1,)
    assert ptr[0] == 0 and ptr[-1] == len(ids)
    for i in range(n):
        row = ids[ptr[i]:ptr[i + 1]]
        assert (np.diff(row) > 0).all(), "row %d does not ascend" % i
    np.testing.assert_array_equal(ptr, want_ptr)
    np.testing.assert_array_equal(ids, want_ids)


@pytest.mark.parametrize("T", [0, 1, 10, 64])
@pytest.mark.parametrize("n", SIZES)
def test_lists_equal_the_restatement(n, T):
    H = _planted(n, T)
    d = ir.hamming(H)
    rel = d <= T
    if n >= 255:                                 # the plants are there: both sides of the cut, within a block and across blocks
        assert d[0, n - 1] == T and d[0, n - 2] == T + 1 and d[3, 7] == T and d[3, 9] == T + 1
    if n == 545:
        assert d[10, 261] == T and d[10, 262] == T + 1 and d[300, 542] == T and d[300, 513] == T + 1 and d[20, 540] == T
    if T <= 10:
        assert rel.sum() <= n + 2 * len(PLANTS)  # nothing but the diagonal and the plants
    ptr, ids = _index(H).neighbors(T)
    _assert_lists(ptr, ids, rel)
    assert (rel == rel.T).all() and rel.diagonal().all()         # symmetric, every row its own neighbour


@pytest.mark.parametrize("n", [33, 257])
def test_every_pair_at_128(n):
    H = _random_rows(n, 3)
    H[1] = ~H[0]                                 # distance 128 exactly
    ptr, ids = _index(H).neighbors(128)
    assert ptr[-1] == n * n
    _assert_lists(ptr, ids, np.ones((n, n), dtype=bool))
    ptr, ids = _index(H).neighbors(127)
    _assert_lists(ptr, ids, ir.hamming(H) <= 127)
    assert ptr[-1] <= n * n - 2


def test_both_words_count():
    rng = np.random.default_rng(5)
    H = _random_rows(300, 11)
    H[1] = _flipped(H[0], 11, "word1", rng)      # word 0 identical: a kernel that compares one word takes these for neighbours
    H[2] = _flipped(H[0], 11, "word0", rng)
    H[3] = ir.flip_bits(H[0], [0, 9, 18, 27, 36, 64, 73, 82, 91, 100])       # five and five
    H[299] = ir.flip_bits(H[0], [63, 127])
    ptr, ids = _index(H).neighbors(10)
    assert ids[ptr[0]:ptr[1]].tolist() == [0, 3, 299]
    _assert_lists(ptr, ids, ir.hamming(H) <= 10)


def test_max_pairs_refuses_with_the_count():
    from hiptagsearch import HipTagSearchError, _lib
    H = np.tile(_random_rows(1, 1), (257, 1))
    index = _index(H)
    with pytest.raises(HipTagSearchError, match=r"\b66049 neighbour pairs"):
        index.neighbors(10, max_pairs=1000)
    with pytest.raises(HipTagSearchError, match=r"\b66049 neighbour pairs"):
        index.groups(10, max_pairs=66048)
    handle = ctypes.c_void_p(12345)
    status = _lib.load().hipts_radius_create_hamming(_lib.ptr(H), _lib.HOST, 257, 10, 1000, 0, None, ctypes.byref(handle))
    assert status == -1 and handle.value is None                 # no handle is left behind
    ptr, ids = index.neighbors(10, max_pairs=66049)               # a valid call right after the refusals
    assert ptr[-1] == 66049 and (index.groups(10) == 0).all()


def test_refusals():
    from hiptagsearch import HipTagSearchError
    index = _index(_random_rows(5, 2))
    for T in (-1, 129):
        with pytest.raises(HipTagSearchError, match="max_distance"):
            index.neighbors(T)
    with pytest.raises(HipTagSearchError, match="empty input"):
        _index(np.zeros((0, 2), dtype=np.uint64)).neighbors(10)
    assert _index(np.zeros((0, 2), dtype=np.uint64)).groups(10).shape == (0,)


# ---- groups -------------------------------------------------------------------------------------------------------------------------
def _group_rows(n=545, seed=21):
    """random rows with: a chain a - b - c whose ends are 16 bits apart (rows 530, 2, 300), a pair across blocks (5, 270), a triple
    inside a block (40, 41, 42), and sparse rows (at most 3 set bits: rows 0, 100, 256, 544) that all pair with each other"""
    H = _random_rows(n, seed)
    H[2] = ir.flip_bits(H[530], range(0, 8))
    H[300] = ir.flip_bits(H[2], range(64, 72))
    H[270] = ir.flip_bits(H[5], [1, 65, 127])
    H[41] = ir.flip_bits(H[40], [3])
    H[42] = ir.flip_bits(H[40], [3, 4, 99])
    H[0], H[100], H[256], H[544] = [0, 0], [1, 0], [0, 6], [1 << 63, 1 << 63]
    return H


def test_groups_equal_the_definition():
    H = _group_rows()
    assert ir.hamming(H)[530, 300] == 16
    index = _index(H)
    for min_set_bits in (0, 8):
        want = ir.groups_ref(H, 10, min_set_bits)
        got = index.groups(10, min_set_bits)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, want)
    everything = index.groups(10, 0)
    assert everything[0] == everything[100] == everything[256] == everything[544] == 0       # the sparse rows: one group, met first
    assert everything[2] == everything[530] == everything[300] == 1                           # the chain is one group
    kept = index.groups()                                                                     # the defaults: 10 and 8
    assert kept[[0, 100, 256, 544]].tolist() == [-1] * 4
    assert (kept[2], kept[5], kept[40]) == (0, 1, 2)                                          # numbered by their smallest row
    assert kept[270] == 1 and kept[41] == kept[42] == 2 and kept[530] == kept[300] == 0
    rest = np.ones(len(H), dtype=bool)
    rest[[0, 100, 256, 544, 2, 530, 300, 5, 270, 40, 41, 42]] = False
    assert (kept[rest] == -1).all()                                                           # singles
    np.testing.assert_array_equal(np.where(everything > 0, everything - 1, -1)[rest | (kept >= 0)], kept[rest | (kept >= 0)])
    # the labels are those of dbscan_ref with min_samples = 2 on the 0/1 relation
    np.testing.assert_array_equal(everything, cr.dbscan_ref(ir.hamming(H) <= 10, 2))


def test_two_runs_give_the_same_bytes():
    H = _planted(545, 64)
    index = _index(H)
    ptr, ids = index.neighbors(64)
    ptr2, ids2 = index.neighbors(64)
    assert ptr.tobytes() == ptr2.tobytes() and ids.tobytes() == ids2.tobytes() and len(ids) > 100000
    assert index.groups(64).tobytes() == index.groups(64).tobytes()


def test_device_hashes_through_the_raw_entry_point():
    import torch
    from hiptagsearch import _lib
    H = _planted(545, 10)
    dev = torch.from_numpy(H.view(np.int64)).cuda()
    handle = ctypes.c_void_p()
    _lib.call("hipts_radius_create_hamming", _lib.ptr(dev), _lib.DEVICE, ctypes.c_int64(545), 10, ctypes.c_int64(0), 0, _lib.current_stream_ptr(),
              ctypes.byref(handle))
    try:
        rows, pairs = ctypes.c_int64(), ctypes.c_int64()
        _lib.call("hipts_radius_info", handle, ctypes.byref(rows), ctypes.byref(pairs))
        ptr, ids = np.empty(rows.value + 1, dtype=np.int64), np.empty(pairs.value, dtype=np.int32)
        _lib.call("hipts_radius_read", handle, _lib.ptr(ptr), _lib.ptr(ids))
    finally:
        _lib.call("hipts_radius_destroy", handle)
    _assert_lists(ptr, ids, ir.hamming(H) <= 10)


# ---- the cosine relation still goes through the shared code -------------------------------------------------------------------------
def test_radius_create_is_unchanged():
    """one case of test_gpu_cluster.py's kind (n = 257, dim = 64); that file remains the real check"""
    from hiptagsearch.cfeatures import CharacterFeatureIndex
    from hiptagsearch.index import Similarity

    def encoder(_x):
        raise AssertionError("no image is encoded here")
    feats = np.ascontiguousarray(cr.chain_fixture(90, 768)[:257, :64])
    ci = CharacterFeatureIndex(encoder=encoder)
    ci.index.close()
    ci.index = Similarity("charactor-featues-idx", None, 64)
    ci.add_features(["img%05d.png" % i for i in range(len(feats))], feats)
    rows = ci.index.matrix()
    rel = np.empty((257, 257), dtype=bool)
    for s in range(0, 257, 256):
        rel[s:s + 256] = (np.float32(1) - ci.index.query(rows[s:s + 256])) < np.float32(cr.T)
    ptr, ids = ci.radius_neighbors(cr.T)
    _assert_lists(ptr, ids, rel)
    from hiptagsearch import HipTagSearchError
    with pytest.raises(HipTagSearchError, match=r"hipts_radius_create: %d neighbour pairs under the threshold" % int(ptr[-1])):
        ci.radius_neighbors(cr.T, max_pairs=int(ptr[-1]) - 1)
