"""GPU: CharacterFeatureIndex.radius_neighbors / .cluster (hipts_radius_*, csrc/radius.hip) and cluster_cfeatures.py.

Two yardsticks for the neighbour lists: the EXISTING Similarity.query, 256 rows at a time, compared in float32 (bit level: the lists
must be exactly the sets it gives), and float64 numpy on the unit rows under the margin condition (independent of every kernel here;
each use asserts the margin on its own input first).  The labels are held against tests/cluster_ref.py::dbscan_ref, the pure-numpy
restatement of the definition that test_cluster_reference.py pins to scikit-learn.

Decision recorded here: an EMPTY index is refused (HipTagSearchError), it does not return empty arrays.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_ref as cr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F1 = np.float32(1)


def _index(feats):
    from hiptagsearch.cfeatures import CharacterFeatureIndex
    from hiptagsearch.index import Similarity

    def encoder(_x):
        raise AssertionError("no image is encoded here")
    ci = CharacterFeatureIndex(encoder=encoder)
    feats = np.asarray(feats, dtype=np.float32)
    if feats.shape[1] != 768:
        ci.index.close()
        ci.index = Similarity("charactor-featues-idx", None, feats.shape[1])
    if len(feats):
        ci.add_features(["img%05d.png" % i for i in range(len(feats))], feats)
    return ci


def _query_relation(ci, t32):
    """bool [n, n] from the existing index product: row i as the query, 256 queries per call"""
    rows = ci.index.matrix()
    rel = np.empty((len(rows), len(rows)), dtype=bool)
    for s in range(0, len(rows), 256):
        d = F1 - ci.index.query(rows[s:s + 256])
        assert d.dtype == np.float32
        rel[s:s + 256] = d < np.float32(t32)
    return rel


def _assert_lists(ptr, ids, rel):
    n = len(rel)
    want_ptr, want_ids = cr.lists_of(rel)
    assert ptr.dtype == np.int64 and ids.dtype == np.int32 and ptr.shape == (n + 1,)
    assert ptr[0] == 0 and ptr[-1] == len(ids)
    for i in range(n):
        row = ids[ptr[i]:ptr[i + 1]]
        assert (np.diff(row) > 0).all(), "row %d does not ascend" % i
    np.testing.assert_array_equal(ptr, want_ptr)
    np.testing.assert_array_equal(ids, want_ids)


def _case_feats(n, dim):
    """the first n rows of the 545-row fixture; where the recipe needs more dimensions than `dim` has (185), its first `dim` columns:
    no chains then, just rows -- enough for the bit-level comparison, which needs no margin"""
    recipe_dim = dim if dim >= 2 * 90 + 5 else 768
    if recipe_dim not in _FIX:
        _FIX[recipe_dim] = cr.chain_fixture(90, recipe_dim)
    return np.ascontiguousarray(_FIX[recipe_dim][:n, :dim])


_FIX = {}
SIZES = [1, 2, 31, 33, 257, 545]     # one tile; a ragged tile; two row blocks, the last ragged; three row blocks (off-diagonal blocks on both sides)


# ---- 1, 2: the lists ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [768, 300, 64, 4])       # 300: K % 8 == 4; 4: the smallest K, the chunk of 4 alone
@pytest.mark.parametrize("n", SIZES)
def test_lists_equal_the_index_query_bit_for_bit(n, dim):
    ci = _index(_case_feats(n, dim))
    rel = _query_relation(ci, cr.T)
    ptr, ids = ci.radius_neighbors(cr.T)
    _assert_lists(ptr, ids, rel)
    assert (rel == rel.T).all()
    if dim >= 185:
        assert rel.diagonal().all() and (n < 33 or rel.sum() > n)       # every row its own neighbour; chains give more than that


@pytest.mark.parametrize("dim", [768, 300])              # the dims the recipe (185 orthonormal directions) exists for
@pytest.mark.parametrize("n", SIZES)
def test_lists_equal_the_float64_oracle(n, dim):
    feats = _case_feats(n, dim)
    rel = cr.relation64(cr.unit_rows(feats), cr.T)       # asserts the margin
    ptr, ids = _index(feats).radius_neighbors(cr.T)
    _assert_lists(ptr, ids, rel)


def test_lists_equal_the_float64_oracle_small_dim():
    feats = cr.chain_fixture(6, 64)                      # the 41-row fixture fits into 64 dimensions
    for n in (1, 2, 31, 33, 41):
        rel = cr.relation64(cr.unit_rows(feats[:n]), cr.T)
        ptr, ids = _index(feats[:n]).radius_neighbors(cr.T)
        _assert_lists(ptr, ids, rel)


# ---- 3: the labels -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixtures():
    out = {}
    for g in cr.FIXTURE_GROUPS:
        feats = cr.chain_fixture(g)
        out[g] = (feats, cr.relation64(cr.unit_rows(feats), cr.T))
    return out


@pytest.mark.parametrize("groups", cr.FIXTURE_GROUPS)
def test_labels_equal_the_definition(fixtures, groups):
    feats, rel = fixtures[groups]
    ci = _index(feats)
    perm = np.random.default_rng(5).permutation(len(feats))
    ci_shuffled = _index(feats[perm])
    for m in (1, 2, 3, 5):
        want = cr.dbscan_ref(rel, m)
        got = ci.cluster(cr.T, m)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, want, err_msg="min_samples %d" % m)
        if m == 5:
            assert (got == -1).all()
        if m == 1:
            assert (got >= 0).all()
        # row order does not change membership: the shuffled copy's labels, carried back to the original rows and renumbered by
        # smallest core row, are the same labels (the fixture has no contested border row)
        back = np.empty(len(feats), dtype=np.int32)
        back[perm] = ci_shuffled.cluster(cr.T, m)
        np.testing.assert_array_equal(cr.relabel_by_smallest_core(back, cr.core_rows(rel, m)), want, err_msg="shuffled, min_samples %d" % m)
    if groups == 90:
        got, core = ci.cluster(cr.T, 3), cr.core_rows(rel, 3)
        assert (int(got.max()) + 1, int(core.sum()), int(((got >= 0) & ~core).sum()), int((got < 0).sum())) == (80, 360, 160, 25)
    np.testing.assert_array_equal(ci.cluster(cr.T), cr.dbscan_ref(rel, 2))          # the default min_samples is 2


# ---- 4: a border row two clusters contend for --------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", cr.CONTESTED_ORDERS)
def test_contested_border_takes_the_smaller_label(order):
    feats = cr.plane_rows(cr.CONTESTED_ANGLES[order])
    rel = cr.relation64(cr.unit_rows(feats), cr.T)
    assert not cr.core_rows(rel, 4)[order.index(0)]
    got = _index(feats).cluster(cr.T, 4)
    assert got.tolist() == cr.CONTESTED_LABELS
    np.testing.assert_array_equal(got, cr.dbscan_ref(rel, 4))


# ---- 5: propagation depth ----------------------------------------------------------------------------------------------------------
def test_one_long_chain_is_one_cluster_within_the_sweep_cap():
    n = 150
    feats = cr.plane_rows(0.03 * np.random.default_rng(11).permutation(n))
    rel = cr.relation64(cr.unit_rows(feats), 1e-3, margin=1e-4)       # 1 - cos 0.03 = 4.5e-4, 1 - cos 0.06 = 1.8e-3; the chain's error bound is 4.6e-5
    assert rel.sum() == 3 * n - 2                                      # a path: itself and the rows one step away
    ci = _index(feats)
    got = ci.cluster(1e-3, 2)
    assert (got == 0).all()
    clusters, sweeps = ci.last_cluster_stats
    print("propagation depth: %d sweeps for a shuffled path of %d rows" % (sweeps, n))
    assert clusters == 1 and 1 <= sweeps <= n


# ---- 6: edges ----------------------------------------------------------------------------------------------------------------------
def test_zero_rows_and_duplicates():
    feats = cr.chain_fixture(6).copy()
    feats[7] = 0
    feats[20] = 0
    feats[30] = feats[3] * 2                             # the same unit row as row 3
    ci = _index(feats)
    ptr, ids = ci.radius_neighbors(cr.T)
    _assert_lists(ptr, ids, _query_relation(ci, cr.T))
    for z in (7, 20):
        assert ptr[z] == ptr[z + 1] and z not in ids
    assert 30 in ids[ptr[3]:ptr[4]] and 3 in ids[ptr[30]:ptr[31]]
    for m in (1, 2, 3):
        got = ci.cluster(cr.T, m)
        assert got[7] == -1 and got[20] == -1
        assert got[3] == got[30] >= 0 or m == 3
    rel = cr.relation64(cr.unit_rows(feats), cr.T)
    np.testing.assert_array_equal(ci.cluster(cr.T, 1), cr.dbscan_ref(rel, 1))


def test_long_rows_are_sorted_too():
    """Rows of 2049 neighbours (one more than the LDS sort holds: sorted in place in global memory) and of 1500 (the LDS sort at a
    length that is no power of two), made of scaled copies of two orthogonal rows scattered among the 41-row fixture."""
    base = cr.chain_fixture(6)
    Q = cr.orthonormal(768, 99)
    rng = np.random.default_rng(3)
    feats = np.concatenate([base, np.outer(rng.uniform(0.5, 3, 2049), Q[0]), np.outer(rng.uniform(0.5, 3, 1500), Q[1])]).astype(np.float32)
    feats = feats[rng.permutation(len(feats))]
    ci = _index(feats)
    rel = _query_relation(ci, cr.T)
    assert sorted(set(rel.sum(axis=1).tolist()))[-2:] == [1500, 2049]
    ptr, ids = ci.radius_neighbors(cr.T)
    _assert_lists(ptr, ids, rel)
    np.testing.assert_array_equal(ci.cluster(cr.T, 3), cr.dbscan_ref(rel, 3))


def test_refusals_leave_a_clean_state():
    from hiptagsearch import HipTagSearchError
    with pytest.raises(HipTagSearchError, match="multiple of 4"):
        _index(np.ones((5, 6), np.float32)).radius_neighbors(cr.T)
    with pytest.raises(HipTagSearchError, match="empty index"):
        _index(np.zeros((0, 768), np.float32)).radius_neighbors(cr.T)
    ci = _index(cr.chain_fixture(6))
    with pytest.raises(HipTagSearchError, match="min_samples"):
        ci.cluster(cr.T, 0)
    ptr, ids = ci.radius_neighbors(cr.T)
    total = int(ptr[-1])
    with pytest.raises(HipTagSearchError, match=r"\b%d neighbour pairs" % total):
        ci.radius_neighbors(cr.T, max_pairs=total - 1)
    with pytest.raises(HipTagSearchError, match=r"\b%d neighbour pairs" % total):
        ci.cluster(cr.T, max_pairs=total - 1)
    ptr2, ids2 = ci.radius_neighbors(cr.T, max_pairs=total)             # a valid call right after the refusal
    np.testing.assert_array_equal(ptr2, ptr)
    np.testing.assert_array_equal(ids2, ids)


def test_threshold_is_compared_in_float32():
    ci = _index(cr.chain_fixture(6))
    rows = ci.index.matrix()
    rel = _query_relation(ci, cr.T)
    i = int(np.flatnonzero(rel.sum(axis=1) > 1)[0])
    j = int(np.flatnonzero(rel[i] & (np.arange(len(rel)) != i))[0])
    d = (F1 - ci.index.query(rows[i:i + 1]))[0, j]
    assert d.dtype == np.float32 and d > 0
    ptr, ids = ci.radius_neighbors(d)                                   # T = d: d < d is false
    assert j not in ids[ptr[i]:ptr[i + 1]] and i not in ids[ptr[j]:ptr[j + 1]]
    ptr, ids = ci.radius_neighbors(np.nextafter(d, np.float32(np.inf)))
    assert j in ids[ptr[i]:ptr[i + 1]] and i in ids[ptr[j]:ptr[j + 1]]
    # a float64 cut between the two float32 values behaves like the upper one (numpy's comparison of a float32 with a float64)
    ptr, ids = ci.radius_neighbors(np.float64(d) + 1e-12)
    assert j in ids[ptr[i]:ptr[i + 1]]


# ---- 7: five thousand rows ---------------------------------------------------------------------------------------------------------
def test_five_thousand_rows():
    rng = np.random.default_rng(4242)
    n, centres, scale = 5000, 200, 0.3
    c = rng.standard_normal((centres, 768))
    member = rng.integers(0, centres, n)
    feats = (c[member] + scale * rng.standard_normal((n, 768))).astype(np.float32)
    d = cr.differences64(cr.unit_rows(feats))
    # the intended cut is 0.3: above the differences inside a group (about 0.08), below those between groups (about 1).  T goes to the
    # middle of the widest gap between consecutive differences in [0.15, 0.6]
    near = np.sort(d[(d > 0.15) & (d < 0.6)])
    edges = np.concatenate(([0.15], near, [0.6]))
    k = int(np.argmax(np.diff(edges)))
    t = np.float32((edges[k] + edges[k + 1]) / 2)
    rel = cr.relation64(cr.unit_rows(feats), t)          # asserts the margin
    ci = _index(feats)
    np.testing.assert_array_equal(rel, _query_relation(ci, t))
    ptr, ids = ci.radius_neighbors(t)
    _assert_lists(ptr, ids, rel)
    ptr2, ids2 = ci.radius_neighbors(t)
    assert ptr.tobytes() == ptr2.tobytes() and ids.tobytes() == ids2.tobytes()
    for m in (2, 20):
        want = cr.dbscan_ref(rel, m)
        got = ci.cluster(t, m)
        np.testing.assert_array_equal(got, want)
        assert got.tobytes() == ci.cluster(t, m).tobytes()
    assert 0 < (cr.dbscan_ref(rel, 20) < 0).sum() < n     # groups smaller than 20 are noise there, the others are not


# ---- 8: the command-line tool ------------------------------------------------------------------------------------------------------
def test_cli_writes_path_label_lines(tmp_path):
    feats = cr.chain_fixture(6)
    ci = _index(feats)
    ci.paths = ["pics/a%03d.png" % i for i in range(len(feats))]
    ci.index.save(str(tmp_path / "charactor-featues-idx"))
    (tmp_path / "charactor-featues-idx.csv").write_text("".join(p + "\n" for p in ci.paths), encoding="utf-8")
    script = os.path.join(ROOT, "anime-illust-image-searcher_amd", "cluster_cfeatures.py")
    res = subprocess.run([sys.executable, script, "--threshold", str(cr.T), "--min-samples", "3", "--out", "groups.csv"], cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    want = ci.cluster(cr.T, 3)
    lines = (tmp_path / "groups.csv").read_text(encoding="utf-8").splitlines()
    assert lines == ["%s,%d" % (p, l) for p, l in zip(ci.paths, want.tolist())]
    noise = int((want < 0).sum())
    assert "%d clusters, %d clustered rows, %d noise rows" % (int(want.max()) + 1, len(want) - noise, noise) in res.stdout
