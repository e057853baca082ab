"""GPU: related tags -- BM25Index.related (hipts_bm25_related, csrc/related.hip), SearchEngine.related_tags / related_tags_table,
query.py --related and genmodel.py --related-tags -- held to tests/related_ref.py, the numpy restatement of the definition that
test_related_reference.py pins.  Everything is integer counts and float64 expressions of exact integers, so every comparison is
assert_array_equal: ids, counts, matched, and the BITS of the scores.

The kernel's constants these cases are built around (csrc/related.hip): a workgroup takes a chunk of REL_CHUNK = 1024 entries of a
query's driving list (the shortest include posting list, or the document range), four per thread (256 threads); sixteen lanes walk
a matching row; the adds go through a histogram of the vocabulary in LDS, which a vocabulary above REL_LDS_MAX_V = 32768 terms does
not fit: its adds go into the global count row directly (REL_DIRECT_MAX = 0: no driving list is short enough to take that arm
otherwise -- it measured slower); a device pass takes 256 queries.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import related_ref as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "anime-illust-image-searcher_amd")
CHUNK = 1024
# driving-list lengths: around the wave, the workgroup (256 threads), the chunk (one entry into the second chunk, four chunks and one
# entry) and every power of two +- 1 up to the chunk
PLANTED_DF = sorted({1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097} |
                    {p + s for p in (2 ** e for e in range(1, 11)) for s in (-1, 0, 1)})
assert max(p for p in PLANTED_DF if p <= CHUNK + 1) == CHUNK + 1 and len(PLANTED_DF) == 30
V_MAIN = 10861                      # the wd-tagger vocabulary
TOP = 0                             # the term of ~80 % of the documents
ZIPF = np.arange(1, 301)            # the terms drawn by rank
BAND = np.arange(1000, 1130)        # the long rows' terms: BAND[:64], BAND[:65], BAND[:130] are one document each
PLANTED0 = 2000                     # PLANTED0 + i occurs in exactly PLANTED_DF[i] documents
UNUSED = 5000                       # df = 0


def _zipf_docs(rng, D, top, ranked, draws=6.0):
    """D documents: `top` with probability 0.8, and Poisson(draws) draws (repeats happen: tf > 1) from `ranked` by a 1 / rank law"""
    p = 1.0 / np.arange(1, len(ranked) + 1)
    n = rng.poisson(draws, D)
    flat = np.asarray(ranked)[rng.choice(len(ranked), size=int(n.sum()), p=p / p.sum())]
    docs = [list(map(int, part)) for part in np.split(flat, np.cumsum(n)[:-1])]
    for d in np.flatnonzero(rng.random(D) < 0.8):
        docs[d].insert(0, top)
    return docs


def _index(docs, V):
    from hiptagsearch.bm25 import BM25Index
    ptr = np.zeros(len(docs) + 1, np.int64)
    ptr[1:] = np.cumsum([len(d) for d in docs])
    idx = BM25Index(ptr, np.asarray([t for d in docs for t in d], np.int32), V)
    e = idx.export()
    want = rr.export_of(docs, V)
    for name in ("csr_ptr", "csr_term", "df"):                  # the arrays the reference reads are the ones the device index holds
        np.testing.assert_array_equal(e[name], want[name])
    return idx, e


@pytest.fixture(scope="module")
def main():
    rng = np.random.default_rng(20240607)
    docs = _zipf_docs(rng, 4900, TOP, ZIPF)
    for i, df in enumerate(PLANTED_DF):
        for d in rng.choice(len(docs), size=df, replace=False):
            docs[d].append(PLANTED0 + i)
    docs += [[-1, V_MAIN, -7],                                   # no term of the dictionary: an empty row
             [7000],                                             # one term, its own
             list(map(int, BAND[:64])), list(map(int, BAND[:65])), list(map(int, BAND[:130])),
             [7001, 7002, 7001, 7001, 7002, TOP, 7001]]          # repeated tags count once
    idx, e = _index(docs, V_MAIN)
    lens = np.diff(e["csr_ptr"])
    assert len(docs) <= 5000 and 7.0 <= lens.mean() <= 9.0 and 0.78 <= e["df"][TOP] / len(docs) <= 0.82
    assert sorted(lens[-6:]) == [0, 1, 3, 64, 65, 130] and e["df"][UNUSED] == 0
    np.testing.assert_array_equal(e["df"][PLANTED0:PLANTED0 + len(PLANTED_DF)], PLANTED_DF)
    yield idx, e
    idx.close()


def _assert_equal(got, want):
    for g, w, name in zip(got, want, ("ids", "scores", "counts", "matched")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if name == "scores":
            g, w = g.view(np.uint64), w.view(np.uint64)
        np.testing.assert_array_equal(g, w, err_msg=name)


def _check(idx, e, queries, k, measure="jaccard", min_count=1):
    got = idx.related(queries, k, measure, min_count)
    _assert_equal(got, rr.related_ref(e, queries, k, measure, min_count))
    return got


@pytest.mark.parametrize("measure", rr.MEASURES)
def test_driving_list_lengths_around_every_split(main, measure):
    idx, e = main
    for i, df in enumerate(PLANTED_DF):
        t = PLANTED0 + i
        ids, _, _, matched = _check(idx, e, [([t], [])], 16, measure)
        assert matched[0] == df and ids[0, 0] >= 0
        # the same list drives when a longer one is included too (its term is then TESTED against the rows), and under an exclusion
        _check(idx, e, [([TOP, t], [])], 16, measure)
        _check(idx, e, [([t], [int(ZIPF[0])])], 16, measure)


def test_row_shapes(main):
    idx, e = main
    D = len(e["csr_ptr"]) - 1
    for measure in rr.MEASURES:
        _, _, counts, matched = _check(idx, e, [([7000], [])], 4, measure)               # the one-term row: no candidate at all
        assert matched[0] == 1 and counts.sum() == 0
        ids, _, counts, matched = _check(idx, e, [([7001], [])], 4, measure)             # tf > 1 counts once
        assert matched[0] == 1 and sorted(ids[0, :2]) == [TOP, 7002] and list(counts[0]) == [1, 1, 0, 0]
        for n_terms, docs_with in ((130, 1), (65, 2), (64, 3)):                          # rows longer than the sixteen lanes, than a wave, than two
            ids, _, counts, matched = _check(idx, e, [([int(BAND[n_terms - 1])], [])], 200, measure)
            assert matched[0] == docs_with and (ids[0] >= 0).sum() == 129
    _, _, _, matched = _check(idx, e, [([], [])], 8, "count")                            # the empty row is a document of the empty query
    assert matched[0] == D


def test_empty_query_counts_are_df_and_lift_is_one(main):
    idx, e = main
    used = np.flatnonzero(e["df"])
    ids, scores, counts, matched = _check(idx, e, [([], [])], 1024, "lift")
    assert matched[0] == len(e["csr_ptr"]) - 1 and len(used) < 1024
    np.testing.assert_array_equal(ids[0, :len(used)], used)                              # all ties: ascending ids
    np.testing.assert_array_equal(counts[0, :len(used)], e["df"][used])
    np.testing.assert_array_equal(scores[0, :len(used)].view(np.uint64), np.ones(len(used)).view(np.uint64))
    assert (ids[0, len(used):] == -1).all() and np.isneginf(scores[0, len(used):]).all() and (counts[0, len(used):] == 0).all()


@pytest.mark.parametrize("measure", rr.MEASURES)
def test_query_shapes(main, measure):
    idx, e = main
    band = list(map(int, BAND))
    for n_inc in (1, 2, 8, 32):
        _, _, _, matched = _check(idx, e, [(band[:n_inc], [])], 20, measure)
        assert matched[0] == 3
        _check(idx, e, [([TOP] + list(map(int, ZIPF[:n_inc - 1])), [])], 20, measure)
    _, _, _, matched = _check(idx, e, [(band[64:96], band[100:132 - 2] + [7000, 7001])], 20, measure)    # 32 and 32
    assert matched[0] == 0
    _, _, _, matched = _check(idx, e, [(band[:32], band[65:97])], 20, measure)           # the 130-term row is excluded
    assert matched[0] == 2
    _, _, _, matched = _check(idx, e, [([], [TOP])], 20, measure)                        # exclude only
    assert 0 < matched[0] < 0.25 * len(e["csr_ptr"])
    _check(idx, e, [([], [TOP, int(ZIPF[0]), int(ZIPF[1])])], 20, measure)
    _check(idx, e, [([], [UNUSED])], 20, measure)                                        # a term of no document may be excluded ...
    ids, scores, counts, matched = _check(idx, e, [([TOP, UNUSED], [])], 20, measure)    # ... or included: nothing matches
    assert matched[0] == 0 and (ids == -1).all() and np.isneginf(scores).all() and (counts == 0).all()
    ids, _, _, matched = _check(idx, e, [([TOP, int(ZIPF[0])], [int(ZIPF[3]), TOP])], 20, measure)       # the same term in both lists
    assert matched[0] == 0 and (ids == -1).all()


def test_refusals(main):
    import hiptagsearch
    idx, e = main
    terms = list(range(33))

    def refused(queries, k=4, measure="jaccard"):
        with pytest.raises(hiptagsearch.HipTagSearchError) as err:
            idx.related(queries, k, measure)
        assert err.value.status == -1                            # HIPTS_ERR_INVALID
    refused([(terms, [])])
    refused([([], terms)])
    refused([([TOP], []), ([V_MAIN], [])])
    refused([([], [-1])])
    refused([([TOP], [])], k=0)
    refused([([TOP], [])], k=1025)
    with pytest.raises(ValueError):
        idx.related([([TOP], [])], 4, "cosine")
    _check(idx, e, [(terms[:32], terms[:32])], 4)                # 32 is legal
    _check(idx, e, [([V_MAIN - 1], [])], 1024)


def test_ranking_ties_padding_and_min_count(main):
    idx, e = main
    # one matching document of 130 terms: 129 candidates share the count 1 -- the id order decides
    ids, scores, counts, matched = _check(idx, e, [([int(BAND[129])], [])], 1024, "count")
    assert matched[0] == 1 and list(ids[0, :129]) == list(map(int, BAND[:129])) and (scores[0, :129] == 1.0).all()
    assert (ids[0, 129:] == -1).all()                            # k = 1024 with 129 candidates: padding
    for measure in rr.MEASURES:
        for t in (TOP, PLANTED0 + 20, int(BAND[3])):
            _check(idx, e, [([t], [])], 1, measure)
            _, _, _, matched = _check(idx, e, [([t], [])], 1024, measure)
            for mc in (0, 1, 2, int(matched[0]), int(matched[0]) + 1):
                ids, _, _, _ = _check(idx, e, [([t], [])], 50, measure, mc)
            assert (ids == -1).all()                             # min_count = n + 1 leaves nothing


def _pool():
    q = [([PLANTED0 + i], []) for i in range(len(PLANTED_DF))]
    q += [([TOP], []), ([], []), ([], [TOP]), ([TOP, int(ZIPF[0])], [int(ZIPF[2])]), ([int(BAND[0])], [int(BAND[100])]),
          ([UNUSED], []), ([TOP], [TOP]), (list(map(int, BAND[:32])), []), ([int(ZIPF[5])], [int(ZIPF[0]), int(ZIPF[1])])]
    return q


@pytest.mark.parametrize("measure", ("jaccard", "lift"))
def test_batches_equal_single_calls(main, measure):
    idx, e = main
    pool = _pool()
    single = [idx.related([q], 12, measure, 2) for q in pool]
    want = rr.related_ref(e, pool, 12, measure, 2)
    for j, s in enumerate(single):
        _assert_equal(s, tuple(w[j:j + 1] for w in want))
    for nq in (1, 2, 256, 257):                                  # 257: two device passes
        pick = [(5 * j + 3) % len(pool) for j in range(nq)]
        got = idx.related([pool[p] for p in pick], 12, measure, 2)
        _assert_equal(got, tuple(np.concatenate([single[p][a] for p in pick]) for a in range(4)))
        again = idx.related([pool[p] for p in pick], 12, measure, 2)
        _assert_equal(again, got)


def _small(V, D, seed, ranked):
    rng = np.random.default_rng(seed)
    return _zipf_docs(rng, D, int(ranked[0]), ranked[1:], draws=5.0)


@pytest.mark.parametrize("V", (1, 5, 70000))
def test_vocabulary_arms(V):
    """V = 1 and 5: a histogram smaller than a wave; V = 70000: above the LDS arm's limit, every query adds into global memory.
    (10 861, the LDS arm, is the corpus of every other test here.)"""
    if V == 1:
        docs, ranked = [[0], [0, 0], [], [0, -1], [3]], [0]
    else:
        ranked = np.arange(V) if V == 5 else (np.arange(300) * 233 + 17) % V          # ~300 used terms spread over the vocabulary
        docs = _small(V, 300, 11 + V, ranked) + [[V - 1, int(ranked[0])]]
        if V == 70000:                                           # one list longer than a chunk would be without the limit
            docs += [[int(ranked[0]), int(ranked[1])]] * 1100
    idx, e = _index(docs, V)
    try:
        terms = [int(t) for t in ranked[:4]] + [V - 1]
        queries = [([], [])] + [([t], []) for t in terms] + [([], [terms[0]])] + [([terms[0]], [terms[-1]])]
        if V > 1:
            queries += [([terms[0], terms[1]], []), ([terms[1]], [terms[0]])]
        for measure in rr.MEASURES:
            for k in (1, 3, 400):
                _check(idx, e, queries, k, measure)
            for q in queries:
                _check(idx, e, [q], 7, measure, 2)
    finally:
        idx.close()


@pytest.fixture(scope="module")
def engine300():
    """300 terms named t000 .. t299 over 600 documents, behind a SearchEngine without model and dense index"""
    from hiptagsearch.search import SearchEngine
    ranked = np.random.default_rng(5).permutation(300)
    docs = _small(300, 600, 77, ranked)
    idx, e = _index(docs, 300)
    token2id = {"t%03d" % t: t for t in range(300)}
    token2id["re:zero"] = token2id.pop("t%03d" % ranked[1])      # a tag with a colon inside, and a frequent one
    yield SearchEngine(None, None, token2id, idx, []), e, ranked
    idx.close()


def test_table_equals_single_calls(engine300):
    eng, e, _ = engine300
    ids, scores = eng.related_tags_table(8, "jaccard", 2)
    assert ids.shape == scores.shape == (300, 8) and ids.dtype == np.int32 and scores.dtype == np.float64
    want = rr.related_ref(e, [([t], []) for t in range(300)], 8, "jaccard", 2)
    np.testing.assert_array_equal(ids, want[0])
    np.testing.assert_array_equal(scores.view(np.uint64), want[1].view(np.uint64))
    for t in range(300):
        one = eng.bm25.related([([t], [])], 8, "jaccard", 2)
        np.testing.assert_array_equal(ids[t], one[0][0])
        np.testing.assert_array_equal(scores[t].view(np.uint64), one[1][0].view(np.uint64))
    assert (ids >= 0).sum() > 500 and (ids == -1).any()


def test_search_engine_related_tags(engine300):
    from hiptagsearch import search
    eng, e, ranked = engine300
    name = {i: t for t, i in eng.token2id.items()}
    a, b, c = (int(ranked[i]) for i in (0, 1, 4))
    assert name[b] == "re:zero"
    for query, inc, exc, kw in (("%s re:zero:3 %s:-1" % (name[a], name[c]), [a, b], [c], {}),
                                ("re:zero", [b], [], {"topn": 300, "measure": "lift", "min_count": 3}),
                                ("%s:-2" % name[a], [], [a], {"topn": 5, "measure": "count"})):
        got = eng.related_tags(query, **kw)
        k = kw.get("topn", 20)
        ids, scores, counts, _ = rr.related_ref(e, [(inc, exc)], k, kw.get("measure", "jaccard"), kw.get("min_count", 1))
        want = [(name[int(t)], float(s), int(n)) for t, s, n in zip(ids[0], scores[0], counts[0]) if t >= 0]
        assert got == want and 0 < len(got) <= k
        assert all(type(t) is str and type(s) is float and type(n) is int for t, s, n in got)
    search.set_engine(eng)
    try:
        assert search.related_tags("re:zero", 3) == eng.related_tags("re:zero", 3)
    finally:
        search.set_engine(None)
    with pytest.raises(KeyError):
        eng.related_tags("re:zero no_such_tag")


def test_command_line_tools(tmp_path):
    """genmodel.py --related-tags 5 writes related-tags.csv beside its other files; query.py --related prints score, count, tag"""
    from hiptagsearch.textio import Dictionary
    rng = np.random.default_rng(9)
    names = ["1girl", "solo", "hat", "re:zero", "hat_(blue)"] + ["tag%02d" % i for i in range(25)]
    docs = [d for d in _zipf_docs(rng, 80, 0, np.arange(1, len(names)), draws=5.0) if len(d) >= 3]
    with open(tmp_path / "tags-wd-tagger.txt", "w", encoding="utf-8") as f:
        for i, d in enumerate(docs):
            f.write(",".join(["imgs/%03d.png" % i] + [names[t] for t in d]) + "\n")
    token2id = Dictionary([[names[t] for t in d] for d in docs]).token2id
    name = {i: t for t, i in token2id.items()}
    e = rr.export_of([[token2id[names[t]] for t in d] for d in docs], len(token2id))

    def run(script, *args):
        r = subprocess.run([sys.executable, os.path.join(PKG, script)] + list(args), cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout
    run("genmodel.py", "--synthetic-d2v", "--epochs", "2", "--related-tags", "5")
    ids, _, _, _ = rr.related_ref(e, [([t], []) for t in range(len(token2id))], 5, "jaccard", 2)
    want = [",".join([name[t]] + [name[int(u)] for u in ids[t] if u >= 0]) for t in range(len(token2id))]
    assert open(tmp_path / "related-tags.csv", encoding="utf-8").read().splitlines() == want
    assert any("," in line for line in want)
    for args, inc, exc, k, measure, mc in ((["1girl hat:-1"], ["1girl"], ["hat"], 20, "jaccard", 1),
                                           (["re:zero solo:+2", "--topn", "7", "--measure", "lift", "--min-count", "2"],
                                            ["re:zero", "solo"], [], 7, "lift", 2),
                                           (["hat_(blue)", "--measure", "count", "--topn", "4"], ["hat_(blue)"], [], 4, "count", 1)):
        out = run("query.py", "--related", *args).splitlines()
        ids, scores, counts, _ = rr.related_ref(e, [([token2id[t] for t in inc], [token2id[t] for t in exc])], k, measure, mc)
        rows = [(name[int(t)], float(s), int(n)) for t, s, n in zip(ids[0], scores[0], counts[0]) if t >= 0]
        assert out[-len(rows):] == rr.format_related(rows) and rows
        assert [l for l in out if "\t" in l] == rr.format_related(rows)
