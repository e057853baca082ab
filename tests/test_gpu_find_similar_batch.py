"""GPU: hipts_rerank_finish against its numpy model (tests/rerank_finish_ref.py) on planted score rows, and
SearchEngine.find_similar_documents_batch against find_similar_documents and the oracle: the same ids and the same float bits."""
import ctypes
import zlib

import numpy as np
import pytest

from rerank_finish_ref import finish, planted_rows, ranked_prefix

pytestmark = pytest.mark.gpu

TOPNS = (5, 10, 11, 800, 5000)


# --------------------------------------------------------------------------------- the kernel through the C ABI
def _device_finish(rows, top10, topn):
    """rf rows float64 [nq, D] -> hipts_topk (device outputs) -> hipts_rerank_finish."""
    import torch
    from hiptagsearch import _lib
    nq, D = rows.shape
    k = min(1024, D)
    dev = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    rids = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    rvals = torch.empty((nq, k), dtype=torch.float64, device="cuda")
    _lib.call("hipts_topk", _lib.ptr(dev), nq, ctypes.c_int64(D), k, _lib.ptr(rids), _lib.ptr(rvals), _lib.DEVICE, 0, _lib.current_stream_ptr())
    cap = min(topn, 10 + k)
    docs = np.full((nq, cap), -7, np.int32)
    scores = np.full((nq, cap), np.nan)
    counts = np.full(nq, -7, np.int32)
    status = np.full(nq, -7, np.int32)
    _lib.call("hipts_rerank_finish", _lib.ptr(rids), _lib.ptr(rvals), nq, k, ctypes.c_int64(D), _lib.ptr(np.ascontiguousarray(top10, dtype=np.int32)),
              topn, _lib.ptr(docs), _lib.ptr(scores), _lib.ptr(counts), _lib.ptr(status), 0, _lib.current_stream_ptr())
    return docs, scores, counts, status


@pytest.mark.parametrize("D", [11, 12, 1024, 1025, 2500])
def test_rerank_finish_kernel_matches_the_model(D):
    """Planted rows (ten ids at the first ranks / scattered with one at rank k - 1 / one or all beyond the prefix; 0-3 cut points, one
    at index 9, the non-cut 1.0, two in the last two places; equal runs, -inf tails, all rest -inf, maximum 0 and negative, a
    maximum that makes the division round), launched as nq = 1, 2 and 37 with different cases in one launch, at every topn."""
    rng = np.random.default_rng(100 + D)
    k = min(1024, D)
    cases = planted_rows(D, k, rng)
    assert len(cases) >= 10
    prefixes = [ranked_prefix(row, k) for _, row, _ in cases]
    launches, c0 = [], 0
    for nq in [1, 2] + [37] * len(cases):
        if c0 >= len(cases):
            break
        launches.append(range(c0, min(len(cases), c0 + nq)))
        c0 += nq
    assert {len(l) for l in launches} >= {1, 2} and (len(cases) < 40 or 37 in {len(l) for l in launches})
    seen = [0, 0]
    for topn in TOPNS:
        for sel in launches:
            rows = np.stack([cases[i][1] for i in sel])
            top10 = np.stack([cases[i][2] for i in sel])
            docs, scores, counts, status = _device_finish(rows, top10, topn)
            for q, i in enumerate(sel):
                want, want_status = finish(prefixes[i][0], prefixes[i][1], cases[i][2], topn, D)
                name = (cases[i][0], topn, len(sel))
                assert int(status[q]) == want_status, name
                assert int(counts[q]) == len(want), name
                c = len(want)
                assert docs[q, :c].tolist() == [d for d, _ in want], name
                assert scores[q, :c].tobytes() == np.array([s for _, s in want], np.float64).tobytes(), name
                seen[want_status] += 1
    assert seen[0] > 0 and (seen[1] > 0 or k == D), seen


# --------------------------------------------------------------------------------- the batch function against the single one
@pytest.fixture(scope="module")
def corpus3000():
    """The set-up of test_gpu_query.py::test_find_similar_documents_matches_oracle; the index rows are inferred on the device (that
    test pins them to the oracle's)."""
    from hiptagsearch import synth
    from hiptagsearch.bm25 import BM25Index
    from hiptagsearch.d2v import Doc2VecInference, pseudorandom_weak_vector
    from hiptagsearch.index import Similarity
    from oracle import bm25 as obm25, d2v as od2v
    V, D, dim, epochs = 400, 3000, 300, 8
    ptr, terms = synth.tag_corpus(D=D, V=V, seed=11)
    toks = synth.vocab_tokens(V)
    docs = [[toks[t] for t in terms[ptr[d]:ptr[d + 1]]] for d in range(D)]
    lines = ["img%05d.png," % d + ",".join(docs[d]) for d in range(D)]
    token2id = {t: i for i, t in enumerate(toks)}
    m = synth.d2v_model(synth.term_counts(ptr, terms, V), dim=dim, seed=44)
    model = Doc2VecInference(m["syn1neg"], m["cum_table"], m["sample_int"], token2id, epochs=epochs)

    def oracle_infer(list_of_docs):
        p = np.zeros(len(list_of_docs) + 1, dtype=np.int64)
        ids = []
        for i, d in enumerate(list_of_docs):
            ids.extend(token2id.get(t, -1) for t in d)
            p[i + 1] = len(ids)
        v0 = np.stack([pseudorandom_weak_vector(dim, " ".join(d)) for d in list_of_docs])
        seeds = np.asarray([model._seed_for(d) for d in list_of_docs], dtype=np.uint64)
        return od2v.infer(m["syn1neg"], m["cum_table"], m["sample_int"], p, np.asarray(ids, np.int32), v0, seeds, epochs)

    rows = model.infer_vectors(docs)
    index = Similarity("idx", None, dim, capacity=D)
    index.add_matrix(rows)
    bm = BM25Index.from_tokens(docs, token2id)
    queries = [toks[3], "%s %s:+2" % (toks[1], toks[7]), "%s:-1 %s %s:3" % (toks[0], toks[5], toks[9]), toks[2] + ":+1",
               toks[3],                                      # a duplicate
               "%s %s" % (toks[4], toks[4]),                 # a repeated tag
               toks[6]]                                      # one tag
    return dict(docs=docs, lines=lines, token2id=token2id, model=model, index=index, bm=bm, rows=rows, queries=queries, dim=dim, D=D,
                oracle_infer=oracle_infer, oracle_bm25=obm25.bm25_build(docs, token2id))


def _same(got, want, what):
    assert [d for d, _ in got] == [d for d, _ in want], what
    assert np.array([s for _, s in got]).tobytes() == np.array([s for _, s in want]).tobytes(), what
    assert all(type(d) is int and type(s) is float for d, s in got), what


@pytest.mark.parametrize("compat", [False, True])
def test_batch_equals_single_and_oracle(corpus3000, compat):
    from hiptagsearch.search import SearchEngine
    from oracle import bm25 as obm25, search as osearch
    c = corpus3000
    eng = SearchEngine(c["model"], c["index"], c["token2id"], c["bm"], c["lines"], compat_rerank=compat)
    qs = c["queries"]
    single = [eng.find_similar_documents(q, 50) for q in qs]
    before = dict(eng.stats)
    batch = eng.find_similar_documents_batch(qs, 50)
    assert batch == single
    for q, g, w in zip(qs, batch, single):
        _same(g, w, q)
    assert eng.stats["batch_single_reruns"] == 0
    assert eng.stats["queries"] == before["queries"] + len(qs)
    corpus, idf, avgdl, _, dl = c["oracle_bm25"]
    rows, dim, D = c["rows"], c["dim"], c["D"]
    for query, got in zip(qs, batch):
        d2v_terms, allw, bm_terms = osearch.parse_query(query)
        qvec = osearch.query_vector(d2v_terms, allw, lambda words: c["oracle_infer"]([words])[0], dim)
        sims = osearch.similarity(rows, qvec.astype(np.float32))
        b = obm25.bm25_score(corpus, idf, avgdl, D, dl, osearch.query_weights(bm_terms, c["token2id"]))
        final = osearch.combine(b, sims)

        def rerank_sims(top_ids, top_scores):
            vecs = c["oracle_infer"]([c["docs"][int(i)] for i in top_ids]).astype(np.float64)
            mean = np.average(vecs, axis=0, weights=top_scores)
            if compat:                                       # webui.py:200-203 as SearchEngine restates it: the query is +-e0
                q = np.zeros_like(mean)
                q[0] = 1.0 if mean.sum() >= 0 else -1.0
            else:
                q = mean / np.linalg.norm(mean)
            return osearch.similarity(rows, q.astype(np.float32))

        _same(got, osearch.rerank(final, 50, rerank_sims), query)


# --------------------------------------------------------------------------------- continuation past rank 1024
class _E0Model:
    """Every document infers to e0 (the stub of test_rerank_continues_past_rank_1024_on_the_device)."""
    vector_size = 4

    def infer_vectors(self, docs):
        v = np.zeros((len(docs), 4), np.float32)
        v[:, 0] = 1.0
        return v


@pytest.fixture(scope="module")
def planted2500():
    """The planted corpus of test_rerank_continues_past_rank_1024_on_the_device behind a whole engine: every document carries the one
    tag, so BM25 is the same for all (1.0 after its normalisation), the query vector and the rerank query are e0, and both stages'
    similarities are the planted column: spacing 3e-4 with two near-ties at ranks 1500 and 2000."""
    from hiptagsearch.bm25 import BM25Index
    from hiptagsearch.index import Similarity
    D, dim = 2500, 4
    a = (1.0 - 3e-4 * np.arange(D)).astype(np.float32)
    a[1500] = np.nextafter(a[1499], np.float32(0))
    a[2000] = np.nextafter(a[1999], np.float32(0))
    perm = np.random.default_rng(3).permutation(D)
    rows = np.zeros((D, dim), np.float32)
    rows[perm, 0] = a
    index = Similarity("idx", None, dim, capacity=D)
    index.add_matrix(rows)
    docs = [["t"]] * D
    bm = BM25Index.from_tokens(docs, {"t": 0})
    return dict(rows=rows, index=index, bm=bm, docs=docs, lines=["img%05d.png,t" % d for d in range(D)], D=D)


def _planted_oracle(p, topn):
    from oracle import bm25 as obm25, search as osearch
    corpus, idf, avgdl, _, dl = obm25.bm25_build(p["docs"], {"t": 0})
    e0 = np.array([1, 0, 0, 0], np.float32)
    sims = osearch.similarity(p["rows"], e0)
    final = osearch.combine(obm25.bm25_score(corpus, idf, avgdl, p["D"], dl, {0: 1}), sims)
    return osearch.rerank(final, topn, lambda ids, scores: sims)


def test_batch_continuation_past_rank_1024(planted2500):
    from hiptagsearch.search import SearchEngine
    p = planted2500
    eng = SearchEngine(_E0Model(), p["index"], {"t": 0}, p["bm"], p["lines"])
    single = eng.find_similar_documents("t", 5000)
    assert len(single) > 1024 and eng.stats["rank_continuations"] >= 1
    batch = eng.find_similar_documents_batch(["t", "t"], 5000)
    for got in batch:
        _same(got, single, "topn 5000")
    assert eng.stats["batch_single_reruns"] >= 1
    _same(single, _planted_oracle(p, 5000), "oracle, topn 5000")
    # topn = 800: the prefix holds no cut point and 800 entries lie below its last one -- complete without a rerun
    eng = SearchEngine(_E0Model(), p["index"], {"t": 0}, p["bm"], p["lines"])
    batch = eng.find_similar_documents_batch(["t", "t", "t"], 800)
    assert eng.stats["batch_single_reruns"] == 0 and eng.stats["rank_continuations"] == 0
    single = eng.find_similar_documents("t", 800)
    assert len(single) == 800
    for got in batch:
        _same(got, single, "topn 800")
    _same(single, _planted_oracle(p, 800), "oracle, topn 800")


# --------------------------------------------------------------------------------- errors and small cases
class _HashModel:
    """A stub that is a pure function of each document's words, counting its calls."""
    def __init__(self, dim):
        self.vector_size = dim
        self.calls = 0

    def infer_vectors(self, docs):
        self.calls += 1
        out = np.empty((len(docs), self.vector_size), np.float32)
        for i, d in enumerate(docs):
            out[i] = np.random.default_rng(zlib.crc32(" ".join(d).encode())).standard_normal(self.vector_size)
        return out


def _small_engine(D, V=40, dim=8, seed=5):
    from hiptagsearch.bm25 import BM25Index
    from hiptagsearch.index import Similarity
    from hiptagsearch.search import SearchEngine
    rng = np.random.default_rng(seed)
    toks = ["w%02d" % i for i in range(V)]
    docs = [[toks[t] for t in rng.choice(V, rng.integers(2, 7), replace=False)] for _ in range(D)]
    token2id = {t: i for i, t in enumerate(toks)}
    model = _HashModel(dim)
    rows = model.infer_vectors(docs)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    index = Similarity("idx", None, dim, capacity=D)
    index.add_matrix(rows)
    bm = BM25Index.from_tokens(docs, token2id)
    eng = SearchEngine(model, index, token2id, bm, ["img%05d.png," % d + ",".join(docs[d]) for d in range(D)])
    return eng, toks, rng


def test_unknown_tag_raises_before_anything_is_launched():
    eng, toks, _ = _small_engine(300)
    calls, stats = eng.model.calls, dict(eng.stats)
    with pytest.raises(KeyError):
        eng.find_similar_documents_batch([toks[1], "%s no_such_tag:+1" % toks[2], toks[3]], 50)
    assert eng.model.calls == calls and eng.stats == stats


def test_empty_batch():
    from hiptagsearch import search
    eng, _, _ = _small_engine(300)
    assert eng.find_similar_documents_batch([], 50) == []
    search.set_engine(eng)
    try:
        assert search.find_similar_documents_batch([], 50) == []
        assert search.find_similar_documents_batch(["w01"], 5) == [eng.find_similar_documents("w01", 5)]
    finally:
        search.set_engine(None)


def test_batch_of_300_is_chunked():
    eng, toks, rng = _small_engine(300)
    qs = []
    for i in range(300):
        tags = rng.choice(len(toks), rng.integers(1, 4), replace=False)
        qs.append(" ".join(toks[t] + ("", ":2", ":+1", ":-1")[(i + j) % 4 if j else 0] for j, t in enumerate(tags)))
    single = [eng.find_similar_documents(q, 50) for q in qs]
    calls = eng.model.calls
    batch = eng.find_similar_documents_batch(qs, 50)
    assert batch == single
    for q, g, w in zip(qs, batch, single):
        _same(g, w, q)
    assert eng.model.calls == calls + 4                      # two chunks (256 + 44), two inference calls each
    assert eng.stats["queries"] == 600 and eng.stats["batch_single_reruns"] == 0


def test_small_corpus_takes_the_per_query_path():
    eng, toks, _ = _small_engine(8, V=12)
    qs = [toks[0], "%s %s:2" % (toks[1], toks[2]), toks[3]]
    single = [eng.find_similar_documents(q, 50) for q in qs]
    assert eng.find_similar_documents_batch(qs, 50) == single
    assert eng.stats["queries"] == 6 and eng.stats["batch_single_reruns"] == 0
