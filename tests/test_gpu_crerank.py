"""GPU: the device rerank of the character-oriented mode (hipts_crerank_*, cfeatures.DeviceReranker) against the host path it stands
beside (cfeatures.cfeatures_rerank, webui.py:303-335), called with the same arguments in the same process.  Every comparison is list
equality: the same doc ids in the same order and the same float scores (==, no tolerance).  Each case first asserts on the HOST
result that it landed in the regime it was built for:

  no survivor    nothing beyond the pinned pairs
  small          1 <= n <= 2048   (one workgroup, sort in LDS)
  large          n > 2048         (the radix sort)
  everything     threshold 2.5, above any 1 - cosine: n = the rows whose path has a tag entry
"""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL_MAX = 2048
TOP10 = [(7, 0.9), (3, 0.5)]


def _corpus(n, clusters, ties, seed):
    """n x 768 features; clusters: (first, last, centre row, eps low, eps high) -> feats[first:last] = feats[centre] + eps_i * noise;
    ties: (rows, source row) -> exact copies.  Tag lines in shuffled order (doc id != feature row); every 7th path has no tag
    entry, one path is on two lines with different tags, one feature path occurs twice."""
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((n, 768)).astype(np.float32)
    for a, b, c, e0, e1 in clusters:
        eps = rng.uniform(e0, e1, (b - a, 1)).astype(np.float32)
        feats[a:b] = feats[c] + eps * rng.standard_normal((b - a, 768)).astype(np.float32)
    for rows, src in ties:
        feats[rows] = feats[src]
    paths = ["dir/img%06d.png" % i for i in range(n)]
    paths[n - 1] = paths[104]                                  # a duplicated feature path (two rows, one tag entry)
    vocab = ["t%d" % i for i in range(30)]
    lines = []
    for i in rng.permutation(n):
        if i % 7 == 3:
            continue                                           # rows without a tag entry
        tags = [vocab[j] for j in rng.choice(30, rng.integers(3, 9), replace=False)]
        if i % 3 != 0:
            tags.append("a")
        if i % 5 == 0:
            tags.append("b")
        if i % 11 == 0:
            tags.append("")                                    # an empty tag
        if i % 13 == 0:
            tags.append("re:zero")
        lines.append(paths[i] + "," + ",".join(tags))
    lines.append(paths[102] + ",a,only_here")                  # path 102 again: the last line wins (doc id and tags)
    return feats, paths, lines


def _setup(feats, paths, lines):
    from hiptagsearch.cfeatures import CharacterFeatureIndex, DeviceReranker
    ci = CharacterFeatureIndex(encoder=lambda x: np.zeros((len(x), 768), np.float32))
    half = len(paths) // 2
    ci.add_features(paths[:half], feats[:half])
    ci.add_features(paths[half:], feats[half:])
    tags = {l.split(",")[0]: {t: True for t in l.split(",")[1:]} for l in lines}       # search.py:67-68
    docid = {l.split(",")[0]: i for i, l in enumerate(lines)}
    return ci, tags, docid, DeviceReranker(ci, lines)


def _both(env, qfeats, req, exc, thr, top10=TOP10):
    from hiptagsearch.cfeatures import cfeatures_rerank
    ci, tags, docid, rr = env
    host = cfeatures_rerank(top10, qfeats, ci, tags, docid, req, exc, thr)
    dev = rr.rerank(top10, qfeats, req, exc, thr)
    assert host[:len(top10)] == list(top10)
    return host, dev, len(host) - len(top10)


def _regime(n, entries):
    return "none" if n == 0 else "everything" if n == entries else "small" if n <= SMALL_MAX else "large"


@pytest.fixture(scope="module")
def env5k():
    # 40 near-duplicates of row 7; 3500 of row 8 (the radix regime); exact copies of row 9, and of row 2000 inside the large cluster
    feats, paths, lines = _corpus(5000, [(100, 140, 7, 0.04, 0.06), (800, 4300, 8, 0.05, 0.4)],
                                  [([60, 61, 4500, 4501, 4502, 4503, 4504, 4600], 9), ([3000, 3001, 3002, 3500, 4000], 2000)], seed=3)
    env = _setup(feats, paths, lines)
    return env + (feats, paths, lines)


CASES_5K = [
    # name, query rows, required, excluded, threshold, regime
    ("no_survivor_threshold", [7], [], [], -1.0, "none"),
    ("no_survivor_unknown_required", [7], ["no_such_tag"], [], 0.05, "none"),
    ("no_survivor_unknown_required_among_known", [8], ["a", "no_such_tag"], [], 0.2, "none"),
    ("small_plain", [7], [], [], 0.05, "small"),
    ("small_required", [7], ["a"], [], 0.05, "small"),
    ("small_excluded", [7], [], ["b"], 0.05, "small"),
    ("small_both", [7], ["a"], ["b"], 0.05, "small"),
    ("small_unknown_excluded", [7], ["a"], ["no_such_tag", "b"], 0.05, "small"),
    ("small_empty_tag_required", [8], [""], [], 0.2, "small"),
    ("small_colon_tag_excluded_two_required", [8], ["a", "t3"], ["re:zero"], 0.2, "small"),
    ("small_mean_of_ten", [100, 101, 102, 103, 104, 105, 106, 107, 108, 109], [], ["b"], 0.05, "small"),
    ("small_ties", [9], [], [], 0.05, "small"),
    ("small_last_line_wins", [7], ["only_here"], [], 0.05, "small"),
    ("large_plain", [8], [], [], 0.2, "large"),
    ("large_excluded", [8], [], ["b"], 0.2, "large"),
    ("large_mean_of_ten", [800, 900, 1000, 1100, 1200, 1300, 1400, 1500, 1600, 1700], [], [], 0.2, "large"),
    ("everything", [8], [], [], 2.5, "everything"),
    ("everything_but_b", [7], [], ["b"], 2.5, "large"),
]


@pytest.mark.parametrize("case", CASES_5K, ids=[c[0] for c in CASES_5K])
def test_device_rerank_equals_host_5k(env5k, case):
    _, rows, req, exc, thr, regime = case
    feats, lines = env5k[4], env5k[6]
    entries = sum(1 for p in env5k[5] if p in env5k[1])
    host, dev, n = _both(env5k[:4], [feats[r] for r in rows], req, exc, thr)
    print("%s: %d survivors of %d rows with a tag entry" % (case[0], n, entries))
    assert _regime(n, entries) == regime                       # the host result itself says which path the device took
    assert [d for d, _ in dev] == [d for d, _ in host]
    assert [s for _, s in dev] == [s for _, s in host]
    assert dev == host
    for d, _ in host[len(TOP10):]:                             # the filter did what the case says (on the host result)
        t = lines[d].split(",")[1:]
        assert all(x in t for x in req) and all(x not in t for x in exc)


def test_ties_keep_ascending_feature_row_order(env5k):
    """The same feature row added several times: equal scores, ranked in ascending row order -- in the LDS sort (copies of row 9) and
    in the radix sort (copies of row 2000 inside the large cluster)."""
    ci, tags, docid, rr, feats, paths, lines = env5k
    for qrow, thr, copies, regime in [(9, 0.05, [9, 60, 61, 4500, 4501, 4502, 4503, 4504, 4600], "small"),
                                      (8, 0.2, [2000, 3000, 3001, 3002, 3500, 4000], "large")]:
        host, dev, n = _both(env5k[:4], [feats[qrow]], [], [], thr)
        assert _regime(n, -1) == regime
        assert dev == host
        want = [docid[paths[r]] for r in copies if paths[r] in docid]           # ascending rows, as doc ids
        assert len(want) >= 4
        pos = [[d for d, _ in dev[len(TOP10):]].index(d) for d in want]
        scores = {dev[len(TOP10) + p][1] for p in pos}
        assert len(scores) == 1                                                  # an exact tie
        assert pos == sorted(pos)                                                # ranked in ascending row order


def test_threshold_is_compared_in_float32(env5k):
    """A threshold of exactly float(diff[r]) excludes row r; one float32 step above includes it."""
    ci, tags, docid, rr, feats, paths, lines = env5k
    q = [feats[7]]
    diffs = ci.differences(np.average(np.stack(q), axis=0))
    r = 110
    assert paths[r] in docid and diffs[r] > 0
    doc = docid[paths[r]]
    at = float(diffs[r])
    above = float(np.nextafter(diffs[r], np.float32(np.inf)))
    host, dev, n = _both(env5k[:4], q, [], [], at)
    assert 1 <= n <= SMALL_MAX and doc not in [d for d, _ in host[len(TOP10):]]
    assert dev == host
    host2, dev2, n2 = _both(env5k[:4], q, [], [], above)
    assert doc in [d for d, _ in host2[len(TOP10):]] and n2 > n
    assert dev2 == host2
    # a float64 threshold a hair above the float32 value rounds back onto it (numpy compares in float32): still excluded
    host3, dev3, n3 = _both(env5k[:4], q, [], [], at + 1e-12)
    assert n3 == n and dev3 == host3


def test_duplicated_path_and_rows_without_entry(env5k):
    ci, tags, docid, rr, feats, paths, lines = env5k
    host, dev, n = _both(env5k[:4], [feats[8]], [], [], 2.5)
    assert dev == host
    docs = [d for d, _ in dev[len(TOP10):]]
    assert docs.count(docid[paths[104]]) == 2                                    # the path that occurs on two feature rows
    assert docid[paths[102]] == len(lines) - 1 and docs.count(len(lines) - 1) == 1
    assert n == sum(1 for p in paths if p in docid) < len(paths)                 # rows without a tag entry never pass


def test_topn_cuts_the_survivors_not_the_pinned_pairs(env5k):
    ci, tags, docid, rr, feats, paths, lines = env5k
    for qrow, thr in [(7, 0.05), (8, 0.2)]:
        host, dev, n = _both(env5k[:4], [feats[qrow]], [], [], thr)
        assert n > 5
        assert rr.rerank(TOP10, [feats[qrow]], [], [], thr, topn=5) == host[:len(TOP10) + 5]
        assert rr.rerank(TOP10, [feats[qrow]], [], [], thr, topn=10 ** 6) == host


def test_rerank_batch_of_mixed_queries_equals_single_calls(env5k):
    from hiptagsearch.cfeatures import cfeatures_rerank
    ci, tags, docid, rr, feats, paths, lines = env5k
    picks = [CASES_5K[i] for i in (0, 3, 6, 13, 1, 16, 11, 14)]
    assert {c[5] for c in picks} == {"none", "small", "large", "everything"}
    tops = [[(i, 1.0 - 0.01 * i)] for i in range(len(picks))]
    qf = [[feats[r] for r in c[1]] for c in picks]
    got = rr.rerank_batch(tops, qf, [c[2] for c in picks], [c[3] for c in picks], [c[4] for c in picks])
    assert len(got) == 8
    for i, c in enumerate(picks):
        assert got[i] == rr.rerank(tops[i], qf[i], c[2], c[3], c[4]), c[0]
        assert got[i] == cfeatures_rerank(tops[i], qf[i], ci, tags, docid, c[2], c[3], c[4]), c[0]
    # one threshold for all, and the index's own cut
    ci.cosine_diff_threshold = 0.05
    got = rr.rerank_batch(tops[:3], qf[:3], [[], ["a"], []], [[], [], ["b"]])
    for i, (req, exc) in enumerate([([], []), (["a"], []), ([], ["b"])]):
        assert got[i] == cfeatures_rerank(tops[i], qf[i], ci, tags, docid, req, exc)


def test_more_tags_than_the_cap(env5k):
    """More required or excluded tags than HIPTS_CRERANK_MAX_TAGS: the C entry point refuses (bad argument), DeviceReranker serves
    the query through the host path."""
    from hiptagsearch import _lib
    from hiptagsearch.cfeatures import CRERANK_MAX_TAGS
    ci, tags, docid, rr, feats, paths, lines = env5k
    many = ["a"] * (CRERANK_MAX_TAGS + 1)
    before = dict(rr.stats)
    host, dev, n = _both(env5k[:4], [feats[7]], many, [], 0.05)
    assert n >= 1 and dev == host and rr.stats["host_fallbacks"] == before["host_fallbacks"] + 1
    host, dev, n = _both(env5k[:4], [feats[7]], [], ["b"] * (CRERANK_MAX_TAGS + 1), 0.05)
    assert n >= 1 and dev == host and rr.stats["host_fallbacks"] == before["host_fallbacks"] + 2
    # exactly the cap runs on the device
    host, dev, n = _both(env5k[:4], [feats[7]], ["a"] * CRERANK_MAX_TAGS, ["b"] * CRERANK_MAX_TAGS, 0.05)
    assert n >= 1 and dev == host and rr.stats["host_fallbacks"] == before["host_fallbacks"] + 2
    q = np.ascontiguousarray(feats[7:8] / np.linalg.norm(feats[7]), dtype=np.float32)
    thr = np.array([0.05], dtype=np.float32)
    ids = np.zeros(CRERANK_MAX_TAGS + 1, dtype=np.int32)
    counts = np.zeros(1, dtype=np.int64)
    for req_n, exc_n in [(CRERANK_MAX_TAGS + 1, 0), (0, CRERANK_MAX_TAGS + 1)]:
        with pytest.raises(_lib.HipTagSearchError) as e:
            _lib.call("hipts_crerank_run", rr._h, ci.index._h, _lib.ptr(q), _lib.HOST, 1, _lib.ptr(thr), _lib.ptr(np.array([0, req_n], np.int32)),
                      _lib.ptr(ids), _lib.ptr(np.array([0, exc_n], np.int32)), _lib.ptr(ids), _lib.ptr(counts), None)
        assert e.value.status == -1 and "HIPTS_CRERANK_MAX_TAGS" in str(e.value)


def test_rows_mismatch_is_refused_and_the_reranker_rebuilds():
    from hiptagsearch import _lib
    from hiptagsearch.cfeatures import cfeatures_rerank
    feats, paths, lines = _corpus(600, [(100, 140, 7, 0.04, 0.06)], [], seed=11)
    ci, tags, docid, rr = _setup(feats[:500], paths[:500], lines)
    host = cfeatures_rerank(TOP10, [feats[7]], ci, tags, docid, [], [], 0.05)
    assert len(host) > len(TOP10) and rr.rerank(TOP10, [feats[7]], [], [], 0.05) == host
    feats[520:530] = feats[7]                                                    # new rows that pass
    ci.add_features(paths[500:], feats[500:])
    q = np.ascontiguousarray(feats[7:8] / np.linalg.norm(feats[7]), dtype=np.float32)
    zero = np.zeros(2, dtype=np.int32)
    counts = np.zeros(1, dtype=np.int64)
    with pytest.raises(_lib.HipTagSearchError) as e:                             # the handle still holds the tables of 500 rows
        _lib.call("hipts_crerank_run", rr._h, ci.index._h, _lib.ptr(q), _lib.HOST, 1, _lib.ptr(np.array([0.05], np.float32)), _lib.ptr(zero),
                  _lib.ptr(zero), _lib.ptr(zero), _lib.ptr(zero), _lib.ptr(counts), None)
    assert e.value.status == -1 and "500" in str(e.value) and "600" in str(e.value)
    host2 = cfeatures_rerank(TOP10, [feats[7]], ci, tags, docid, [], [], 0.05)
    assert len(host2) > len(host)
    assert rr.rerank(TOP10, [feats[7]], [], [], 0.05) == host2 and rr.stats["table_rebuilds"] == 1 and rr.rows == 600
    with pytest.raises(_lib.HipTagSearchError):                                  # read past the ranked entries
        _lib.call("hipts_crerank_read", rr._h, 0, ctypes.c_int64(0), ctypes.c_int64(len(host2)), _lib.ptr(np.zeros(1000, np.int32)),
                  _lib.ptr(np.zeros(1000, np.float64)))


def test_device_rerank_equals_host_100k():
    """Once at the size the project is measured at: 100 000 x 768, clusters of 10, 300 and 5000 near-duplicates."""
    feats, paths, lines = _corpus(100000, [(1000, 1010, 7, 0.04, 0.06), (2000, 2300, 8, 0.04, 0.06), (50000, 55000, 9, 0.05, 0.3)],
                                  [([70000, 70001, 99000], 9), ([52000, 52001, 54000], 51000)], seed=45)
    env = _setup(feats, paths, lines)
    entries = sum(1 for p in paths if p in env[2])
    for name, rows, req, exc, thr, regime in [("c10", [7], [], [], 0.05, "small"), ("c300", [8], ["a"], ["b"], 0.05, "small"),
                                              ("c5000", [9], [], [], 0.2, "large"), ("c5000_tags", [9], ["a"], ["b"], 0.2, "large"), ("c5000_two_required", [9], ["a", "t3"], ["b"], 0.2, "small"),
                                              ("c5000_mean", [50000, 50500, 51000, 51500, 52000, 52500, 53000, 53500, 54000, 54500], [], ["re:zero"], 0.2, "large"),
                                              ("none", [9], ["no_such_tag"], [], 0.2, "none"), ("everything", [9], [], [], 2.5, "everything")]:
        host, dev, n = _both(env, [feats[r] for r in rows], req, exc, thr)
        print("%s: %d survivors" % (name, n))
        assert _regime(n, entries) == regime, name
        assert dev == host, name
    got = env[3].rerank_batch([TOP10] * 3, [[feats[7]], [feats[9]], [feats[9]]], [[], [], []], [[], [], ["b"]], [0.05, 0.2, 2.5])
    for g, (r, exc, thr) in zip(got, [(7, [], 0.05), (9, [], 0.2), (9, ["b"], 2.5)]):
        assert g == _both(env, [feats[r]], [], exc, thr)[0]


def test_character_oriented_mode_end_to_end_with_device_rerank(tmp_path):
    """The set-up of the character-oriented end-to-end test: find_similar_documents after enable_device_crerank() returns the list
    it returned before (the host loop), for the same three queries."""
    from PIL import Image
    from hiptagsearch import synth
    from hiptagsearch.bm25 import BM25Index
    from hiptagsearch.cfeatures import CCIPEncoder, CharacterFeatureIndex, gen_image_ndarray
    from hiptagsearch.d2v import Doc2VecInference
    from hiptagsearch.index import Similarity
    from hiptagsearch.search import SearchEngine
    V, D, dim, epochs = 60, 40, 300, 5
    rng = np.random.default_rng(9)
    toks = synth.vocab_tokens(V)
    os.makedirs(tmp_path / "imgs")
    base = rng.integers(0, 256, (8, 64, 64, 3), dtype=np.uint8)
    paths, docs = [], []
    for i in range(D):
        ch = i % 8
        im = np.clip(base[ch].astype(np.int32) + rng.integers(-6, 7, base[ch].shape), 0, 255).astype(np.uint8)
        p = str(tmp_path / "imgs" / ("%03d.png" % i))
        Image.fromarray(im).save(p)
        paths.append(p)
        doc = [toks[ch], toks[8 + (i % 5)], toks[20 + (i % 3)], toks[30 + rng.integers(0, 30)]]
        docs.append(list(dict.fromkeys(doc)))
    lines = [p + "," + ",".join(d) for p, d in zip(paths, docs)]
    token2id = {t: i for i, t in enumerate(toks)}
    ptr = np.cumsum([0] + [len(d) for d in docs]).astype(np.int64)
    terms = np.array([token2id[t] for d in docs for t in d], dtype=np.int32)
    m = synth.d2v_model(synth.term_counts(ptr, terms, V), dim=dim, seed=44)
    model = Doc2VecInference(m["syn1neg"], m["cum_table"], m["sample_int"], token2id, epochs=epochs)
    index = Similarity("idx", None, dim, capacity=D)
    index.add_matrix(model.infer_vectors(docs))
    bm = BM25Index.from_tokens(docs, token2id)
    ccfg = dict(synth.CCIP_TINY)
    enc = CCIPEncoder(ccfg, synth.ccip_weights(ccfg, seed=3), max_batch=8)
    cindex = CharacterFeatureIndex(enc)
    if enc.out_dim != 768:
        cindex.index = Similarity("c", None, enc.out_dim)
    arrs = [gen_image_ndarray(p, ccfg["image_size"]) for p in paths]
    feats = np.concatenate([cindex.ccip_batch_extract_features(arrs[s:s + 8]) for s in range(0, D, 8)])
    cindex.add_features(paths, feats)
    unit = cindex.index.matrix()
    eng = SearchEngine(model, index, token2id, bm, lines, search_mode="character oriented")
    eng.cindex = cindex
    sims = unit @ unit.T
    same = np.array([[i % 8 == j % 8 for j in range(D)] for i in range(D)])
    lo, hi = (1 - sims[same]).max(), (1 - sims[~same]).min()
    assert lo < hi
    cindex.cosine_diff_threshold = float((lo + hi) / 2)
    queries = [toks[0], toks[1] + " " + toks[9] + ":+1", toks[2] + " " + toks[21] + ":-1"]
    assert eng.crerank is None                                                   # off by default
    before = [eng.find_similar_documents(q, topn=50) for q in queries]
    rr = eng.enable_device_crerank()
    after = [eng.find_similar_documents(q, topn=50) for q in queries]
    assert rr.stats["device_queries"] == 3 and rr.stats["host_fallbacks"] == 0
    assert any(len(b) > 10 for b in before)                                      # something beyond the pinned ten was ranked
    for q, b, a in zip(queries, before, after):
        assert a == b, q
    eng.enable_device_crerank(False)
    assert [eng.find_similar_documents(q, topn=50) for q in queries] == before
