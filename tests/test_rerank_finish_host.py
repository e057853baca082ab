"""CPU: the completion rule of hipts_rerank_finish.  Whenever the numpy model of the kernel (tests/rerank_finish_ref.py) calls a
ranked prefix complete, its list is the list oracle.search.rerank computes from the FULL score row -- over random rows and over the
planted rows the GPU test feeds the kernel.  No GPU, no product code."""
import numpy as np
import pytest

from rerank_finish_ref import finish, planted_rows, ranked_prefix

from oracle import search as osearch


def _check(final, rs, k, topn, seen):
    """final float64 [D] (first stage), rs float32 [D] (rerank similarities): model on the prefix against the oracle on the row."""
    D = len(final)
    rf = osearch.ORIGINAL_SCORE_WEIGHT * final + osearch.RERANKED_SCORE_WEIGHT * rs          # webui.py:208, as oracle.search.rerank
    top10 = osearch.stable_rank(final)[:10]
    rids, rvals = ranked_prefix(rf, k)
    got, status = finish(rids, rvals, top10, topn, D)
    seen[status] += 1
    if status == 0:
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            want = osearch.rerank(final, topn, lambda ids, scores: rs)
        assert [d for d, _ in got] == [d for d, _ in want]
        assert np.array([s for _, s in got]).tobytes() == np.array([s for _, s in want]).tobytes()
    return status


def test_random_rows():
    rng = np.random.default_rng(5)
    seen = [0, 0]
    for D, k in [(11, 11), (12, 12), (40, 40), (40, 16), (300, 64), (300, 300), (700, 128)]:
        for trial in range(40):
            final = np.round(rng.random(D), 2 if trial % 2 else 6)                          # coarse rounding: ties in the first stage
            rs = np.round(rng.standard_normal(D), 2 + trial % 3).astype(np.float32)         # ... and runs of equal rerank scores
            if trial % 4 == 1:                                                              # near-ties one float32 step apart
                for i in rng.choice(D, 4, replace=False):
                    rs[i] = np.nextafter(rs[(i + 1) % D], np.float32(-np.inf))
            if trial % 4 == 2:
                final[rng.choice(D, D // 3, replace=False)] = -np.inf                       # excluded documents
            if trial % 8 == 3:
                final -= 2.0; rs -= np.float32(3.0)                                         # nothing positive: no normalisation
            for topn in (5, 10, 11, 50, 5000):
                _check(final, rs, k, topn, seen)
    assert seen[0] > 100 and seen[1] > 100, seen                                            # both outcomes are exercised


@pytest.mark.parametrize("D,k", [(11, 11), (12, 12), (64, 64), (65, 64), (200, 64)])
def test_planted_rows(D, k):
    """The planted rows of the kernel test at a short prefix: ten ids at the first ranks / scattered / beyond the prefix, 0-3 cut
    points, cuts in the last two places, equal runs, -inf tails, a non-positive maximum.  The first stage marks the ten ids
    with scores small enough to vanish in 0.7 * final + 0.3 * rs, so rf is 0.3 * the planted float32 row."""
    rng = np.random.default_rng(D)
    seen = [0, 0]
    rows = planted_rows(D, k, rng, dtype=np.float32)
    assert len(rows) >= 10
    for name, rs, top10 in rows:
        final = np.zeros(D)
        final[top10] = (10 - np.arange(10)) * 1e-200
        for topn in (5, 10, 11, 50, 5000):
            _check(final, rs, k, topn, seen)
    assert seen[0] > 0 and (seen[1] > 0 or k == D), seen


def test_one_cut_in_an_unexhausted_prefix_is_not_complete_past_it():
    """One cut point inside the prefix and none after it: the full list ends AT that cut (webui.py:74-75), so entries past it
    must not be emitted on the strength of the prefix alone -- only the indices below the cut are certain."""
    D, k = 200, 64
    rs = (1.0 - 3e-3 * np.arange(D)).astype(np.float32)
    rs[31] = np.nextafter(rs[30], np.float32(0))                   # the only near-tie: F index 30 (ranks 10.. are the rest)
    final = np.zeros(D)
    final[:10] = (10 - np.arange(10)) * 1e-200
    seen = [0, 0]
    assert _check(final, rs, k, 20, seen) == 0                     # 20 entries lie below the cut
    assert _check(final, rs, k, 40, seen) == 1                     # 40 do not; the full ranking gives 30
    assert len(osearch.rerank(final, 40, lambda ids, scores: rs)) == 30
