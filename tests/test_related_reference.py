"""CPU: tests/related_ref.py (the numpy restatement of the related-tags definition that test_gpu_related.py holds the device to) against
a brute-force Python-set statement of the same definition and a hand-computed corpus; and search.parse_related_query, the pure parse
behind SearchEngine.related_tags."""
import math

import numpy as np
import pytest

import related_ref as rr


def _brute(docs, V, include, exclude, k, measure, min_count):
    """the definition word by word, on Python sets and Python floats (IEEE doubles, one rounding per operation)"""
    T = [set(t for t in d if 0 <= t < V) for d in docs]
    D = len(docs)
    M = [d for d in range(D) if set(include) <= T[d] and not (set(exclude) & T[d])]
    n = len(M)
    df = [sum(1 for d in range(D) if u in T[d]) for u in range(V)]
    rows = []
    for u in range(V):
        c = sum(1 for d in M if u in T[d])
        if c < max(min_count, 1) or u in include or u in exclude:
            continue
        if measure == "count":
            s = float(c)
        elif measure == "jaccard":
            s = float(c) / float(n + df[u] - c)
        else:
            s = (float(c) / float(n)) / (float(df[u]) / float(D))
        rows.append((-s, u, c))
    rows.sort()
    rows = rows[:k]
    pad = k - len(rows)
    return ([u for _, u, _ in rows] + [-1] * pad, [-s for s, _, _ in rows] + [-math.inf] * pad, [c for _, _, c in rows] + [0] * pad, n)


def _assert_same(got, want):
    ids, scores, counts, n = got
    wi, ws, wc, wn = want
    np.testing.assert_array_equal(ids, np.asarray(wi, np.int32))
    np.testing.assert_array_equal(scores.view(np.uint64), np.asarray(ws, np.float64).view(np.uint64))
    np.testing.assert_array_equal(counts, np.asarray(wc, np.int64))
    assert n == wn


@pytest.mark.parametrize("seed", range(12))
def test_reference_equals_the_set_statement_on_random_corpora(seed):
    rng = np.random.default_rng(seed)
    D, V = int(rng.integers(1, 41)), int(rng.integers(1, 13))
    # ids -1 and V are "tags outside the dictionary", repeated ids count once, some documents are empty
    docs = [list(rng.integers(-1, V + 1, size=int(rng.integers(0, 9)))) for _ in range(D)]
    e = rr.export_of(docs, V)
    assert e["csr_ptr"][-1] == len(e["csr_term"]) and e["df"].sum() == len(e["csr_term"])
    for _ in range(25):
        terms = rng.permutation(V)
        ni = int(rng.integers(0, min(V, 3) + 1))
        nx = int(rng.integers(0, min(V - ni, 2) + 1))
        include, exclude = list(map(int, terms[:ni])), list(map(int, terms[ni:ni + nx]))
        if ni and rng.random() < 0.1:
            exclude = exclude + [include[0]]                         # a term in both lists: n = 0
        for measure in rr.MEASURES:
            k, mc = int(rng.integers(1, V + 3)), int(rng.integers(0, 4))
            got = rr.related_one(e["csr_ptr"], e["csr_term"], e["df"], include, exclude, k, measure, mc)
            _assert_same(got, _brute(docs, V, include, exclude, k, measure, mc))


# Five documents over the terms 0 .. 5 (term 5 is in no document):
#   d0 {0, 1, 2}   d1 {0, 1}   d2 {0, 2, 3}   d3 {1, 3}   d4 {0, 1, 2, 4}            df = [4, 4, 3, 2, 1, 0], D = 5
HAND_DOCS = [[0, 1, 2], [0, 1, 1], [0, 2, 3, -1], [1, 3], [0, 1, 2, 4]]


def test_hand_computed_corpus():
    e = rr.export_of(HAND_DOCS, 6)
    np.testing.assert_array_equal(e["df"], [4, 4, 3, 2, 1, 0])
    one = lambda inc, exc, k, m, mc=1: rr.related_one(e["csr_ptr"], e["csr_term"], e["df"], inc, exc, k, m, mc)
    # include {0}: M = {d0, d1, d2, d4}, n = 4; c = [4, 3, 3, 1, 1, 0]
    #   jaccard  u1: 3 / (4 + 4 - 3) = 0.6   u2: 3 / (4 + 3 - 3) = 0.75   u3: 1 / (4 + 2 - 1) = 0.2   u4: 1 / (4 + 1 - 1) = 0.25
    _assert_same(one([0], [], 5, "jaccard"), ([2, 1, 4, 3, -1], [0.75, 0.6, 0.25, 0.2, -math.inf], [3, 3, 1, 1, 0], 4))
    #   count: u1 and u2 tie at 3, u3 and u4 at 1 -- the lower id first
    _assert_same(one([0], [], 3, "count"), ([1, 2, 3], [3.0, 3.0, 1.0], [3, 3, 1], 4))
    #   lift  u1: (3/4) / (4/5)   u2: (3/4) / (3/5)   u3: (1/4) / (2/5)   u4: (1/4) / (1/5)
    #   (u2 and u4 both round to 1.25: the lower id first)
    assert 0.75 / 0.6 == 0.25 / 0.2 == 1.25
    _assert_same(one([0], [], 4, "lift"), ([2, 4, 1, 3], [1.25, 1.25, 0.75 / 0.8, 0.25 / 0.4], [3, 1, 3, 1], 4))
    #   min_count 2 leaves u1 and u2
    _assert_same(one([0], [], 3, "jaccard", 2), ([2, 1, -1], [0.75, 0.6, -math.inf], [3, 3, 0], 4))
    # include {0, 1}, exclude {3}: M = {d0, d1, d4}, n = 3; c = [3, 3, 2, 0, 1, 0]; candidates u2: 2 / (3 + 3 - 2), u4: 1 / (3 + 1 - 1)
    _assert_same(one([0, 1], [3], 2, "jaccard"), ([2, 4], [0.5, 1 / 3], [2, 1], 3))
    # exclude only {0}: M = {d3}; c = [0, 1, 0, 1, 0, 0]; u1: 1 / (1 + 4 - 1), u3: 1 / (1 + 2 - 1)
    _assert_same(one([], [0], 2, "jaccard"), ([3, 1], [0.5, 0.25], [1, 1], 1))
    # the empty query: c = df, n = D, lift is 1.0 for every term that occurs, ids ascending
    _assert_same(one([], [], 6, "lift"), ([0, 1, 2, 3, 4, -1], [1.0] * 5 + [-math.inf], [4, 4, 3, 2, 1, 0], 5))
    # a term no document carries, and a term in both lists: nothing matches, everything is padding
    _assert_same(one([5], [], 2, "count"), ([-1, -1], [-math.inf] * 2, [0, 0], 0))
    _assert_same(one([0], [0], 2, "count"), ([-1, -1], [-math.inf] * 2, [0, 0], 0))
    # the batch form stacks the rows
    ids, scores, counts, matched = rr.related_ref(e, [([0], []), ([], [0])], 2, "jaccard")
    np.testing.assert_array_equal(ids, [[2, 1], [3, 1]])
    np.testing.assert_array_equal(scores, [[0.75, 0.6], [0.5, 0.25]])
    np.testing.assert_array_equal(counts, [[3, 3], [1, 1]])
    np.testing.assert_array_equal(matched, [4, 1])
    assert ids.dtype == np.int32 and scores.dtype == np.float64 and counts.dtype == np.int64 and matched.dtype == np.int64


def test_parse_related_query():
    from hiptagsearch.search import parse_related_query
    token2id = {"a": 0, "b": 1, "c": 2, ":d": 3, "re:zero": 4, "re": 5, "hat_(blue)": 6}
    assert parse_related_query("a b:+2 c:-1", token2id) == ([0, 1], [2])
    assert parse_related_query(":d", token2id) == ([3], [])                  # a tag that contains ':' and has no weight
    assert parse_related_query(":d:-2 a", token2id) == ([0], [3])
    assert parse_related_query("re:zero:3", token2id) == ([4], [])           # digits are a weight; its value is ignored
    assert parse_related_query("re:zero", token2id) == ([4], [])
    assert parse_related_query("hat_(blue)", token2id) == ([6], [])          # looked up as typed: no parenthesis escaping
    assert parse_related_query("a a:5 b:-1 b:-3", token2id) == ([0], [1])    # ids are kept once
    assert parse_related_query("a a:-1", token2id) == ([0], [0])             # in both lists: legal, matches nothing
    assert parse_related_query("", token2id) == ([], [])
    with pytest.raises(KeyError):
        parse_related_query("a unknown_tag", token2id)
    with pytest.raises(KeyError):
        parse_related_query("hat_\\(blue\\)", token2id)
