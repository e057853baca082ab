"""Related tags: the numpy restatement of the definition in include/hip_tagsearch.h (hipts_bm25_related), on the arrays of
BM25Index.export().  test_related_reference.py pins it to a Python-set statement and a hand-computed corpus; test_gpu_related.py holds
the device to it bit for bit.

  T(d)   the distinct term ids of document d (csr_term[csr_ptr[d] : csr_ptr[d + 1]]; tf is ignored)
  M      { d : include is a subset of T(d) and exclude does not meet T(d) },  n = |M|   (both lists empty: every document)
  c[u]   |{ d in M : u in T(d) }|
  score  count: c;  jaccard: c / (n + df[u] - c);  lift: (c / n) / (df[u] / D)      float64, one rounding per operation
  candidates: c[u] >= max(min_count, 1), u in neither list; ranked by (score descending, id ascending); rows padded with (-1, -inf, 0)
"""
import numpy as np

MEASURES = ("count", "jaccard", "lift")


def match_mask(csr_ptr, csr_term, vocab, include, exclude):
    """bool [D]: the documents of M"""
    D = len(csr_ptr) - 1
    doc_of = np.repeat(np.arange(D), np.diff(csr_ptr))
    ok = np.ones(D, dtype=bool)
    for t in include:
        ok &= np.bincount(doc_of[csr_term == t], minlength=D) > 0
    for t in exclude:
        ok &= np.bincount(doc_of[csr_term == t], minlength=D) == 0
    return ok


def related_one(csr_ptr, csr_term, df, include, exclude, k, measure="jaccard", min_count=1):
    """ids int32 [k], scores float64 [k], counts int64 [k], matched"""
    assert measure in MEASURES
    D, V = len(csr_ptr) - 1, len(df)
    doc_of = np.repeat(np.arange(D), np.diff(csr_ptr))
    ok = match_mask(csr_ptr, csr_term, V, include, exclude)
    n = int(ok.sum())
    c = np.bincount(csr_term[ok[doc_of]], minlength=V).astype(np.int64)
    cand = c >= max(int(min_count), 1)
    cand[np.asarray(list(include) + list(exclude), dtype=np.int64)] = False
    u = np.flatnonzero(cand)
    cu, dfu = c[u], np.asarray(df, dtype=np.int64)[u]
    if measure == "count":
        s = cu.astype(np.float64)
    elif measure == "jaccard":
        s = cu.astype(np.float64) / (np.int64(n) + dfu - cu).astype(np.float64)
    else:
        s = (cu.astype(np.float64) / np.float64(n)) / (dfu.astype(np.float64) / np.float64(D))
    order = np.lexsort((u, -s))[:k]                      # primary key -s (score descending), then id ascending
    ids = np.full(k, -1, np.int32)
    scores = np.full(k, -np.inf, np.float64)
    counts = np.zeros(k, np.int64)
    ids[:len(order)] = u[order]
    scores[:len(order)] = s[order]
    counts[:len(order)] = cu[order]
    return ids, scores, counts, n


def related_ref(export, queries, k, measure="jaccard", min_count=1):
    """`export`: the dict of BM25Index.export() (csr_ptr, csr_term, df are read); `queries`: a sequence of (include ids, exclude ids).
    Returns ids int32 [nq, k], scores float64 [nq, k], counts int64 [nq, k], matched int64 [nq]."""
    rows = [related_one(export["csr_ptr"], export["csr_term"], export["df"], list(inc), list(exc), k, measure, min_count)
            for inc, exc in queries]
    return (np.array([r[0] for r in rows], np.int32).reshape(len(rows), k), np.array([r[1] for r in rows], np.float64).reshape(len(rows), k),
            np.array([r[2] for r in rows], np.int64).reshape(len(rows), k), np.array([r[3] for r in rows], np.int64))


def export_of(docs, vocab):
    """The arrays hipts_bm25_build makes of token-id documents (ids outside [0, vocab) dropped, first-occurrence order, tf counted):
    what BM25Index.export() returns, without a device -- for the CPU tests and for building expectations before an index exists."""
    ptr, term, tf = [0], [], []
    df = np.zeros(vocab, np.int64)
    for d in docs:
        seen = {}
        for t in d:
            t = int(t)
            if 0 <= t < vocab:
                seen[t] = seen.get(t, 0) + 1
        term.extend(seen.keys())
        tf.extend(seen.values())
        for t in seen:
            df[t] += 1
        ptr.append(len(term))
    return {"csr_ptr": np.asarray(ptr, np.int64), "csr_term": np.asarray(term, np.int32), "csr_tf": np.asarray(tf, np.int32), "df": df}


def format_related(rows):
    """query.py --related prints one such line per (tag, score, count)"""
    return ["%.6f\t%d\t%s" % (score, count, tag) for tag, score, count in rows]
