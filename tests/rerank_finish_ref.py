"""numpy model of hipts_rerank_finish (include/hip_tagsearch.h) and the planted score rows its tests share.

finish() maps a ranked prefix of  rf = 0.7 * final + 0.3 * rs  (hipts_topk: value descending, ties by ascending id), the first
stage's top-ten ids, topn and the corpus size to the emitted list and the status.  It is written for any prefix length k <= n, so
the CPU test can use short prefixes."""
import numpy as np

DIFF_FILTER_THRESH = 1e-6
PIN = 10


def ranked_prefix(row, k):
    """(ids int32 [k], vals float64 [k]) of one score row in hipts_topk's order."""
    row = np.asarray(row, dtype=np.float64)
    order = np.lexsort((np.arange(len(row)), -row))[:k]
    return order.astype(np.int32), row[order]


def finish(rids, rvals, top10, topn, n):
    """-> ([(id, score)], status).  status 0: the list is what the full ranking gives; 1: the ranks past the prefix decide it."""
    rids, rvals, top10 = np.asarray(rids), np.asarray(rvals, dtype=np.float64), np.asarray(top10)
    k = len(rids)
    assert len(top10) == PIN and 1 <= k <= n and n > PIN and topn >= 1
    mx = rvals[0]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        vals = rvals / mx if mx > 0 else rvals
        rest = ~np.isin(rids, top10)
        ids = np.concatenate([top10, rids[rest]])
        s = np.concatenate([np.ones(PIN), vals[rest]])
        L = len(ids)
        d = s[:-1] - s[1:]
        cuts = np.flatnonzero((d != 0) & (d < DIFF_FILTER_THRESH))         # NaN (-inf - -inf) compares false
    exhausted = k == n or rvals[k - 1] == -np.inf
    if len(cuts) >= 2:
        t = int(cuts[1])
    elif len(cuts) == 1:
        t = int(cuts[0])          # exhausted: the filter's single cut.  Not exhausted: the full list ends here or at a later second cut
    else:
        t = L if exhausted else L - 1                                       # the gap after the prefix's last entry is unknown
    sel = [i for i in range(t) if s[i] > 0]
    status = 0 if (len(cuts) >= 2 or exhausted or len(sel) >= topn) else 1
    return [(int(ids[i]), float(s[i])) for i in sel[:topn]], status


PLACEMENTS = ("first", "scattered", "one_beyond", "all_beyond")
CUTS = (0, 1, 2, 3, "index9", "one_exact", "last2")
VALUES = ("plain", "runs", "inf_tail", "rest_inf", "mx0", "mxneg", "scaled")


def planted_row(D, k, placement, cuts, values, rng, dtype=np.float64):
    """One score row of D documents (dtype: the number format the near-ties are one step apart in) and ten top ids, or None when
    the combination does not exist at this size.  Ranks are spaced 3e-4 apart, far more than the threshold, so the only cut
    points are the planted ones; `placement` puts the ten ids at the first ranks, scattered over the prefix with one at rank
    k - 1, nine inside and one beyond the prefix, or all beyond it."""
    one = dtype(1.0)
    by_rank = (1.0 - 3e-4 * np.arange(D)).astype(dtype)
    if placement == "first":
        top_ranks = np.arange(PIN)
    elif placement == "scattered":
        if k < PIN + 1:
            return None
        top_ranks = np.concatenate([rng.choice(k - 1, PIN - 1, replace=False), [k - 1]])
    elif placement == "one_beyond":
        if D - k < 1:
            return None
        top_ranks = np.concatenate([rng.choice(k, PIN - 1, replace=False), [k + rng.integers(D - k)]])
    else:
        if D - k < PIN:
            return None
        top_ranks = k + rng.choice(D - k, PIN, replace=False)
    top_ranks = rng.permutation(top_ranks)
    rest = np.setdiff1d(np.arange(k), top_ranks)                            # ranks of the rest inside the prefix, ascending
    m = len(rest)
    if values == "runs":
        for r0 in rng.choice(max(1, D - 6), 3):
            by_rank[r0:r0 + 6] = by_rank[r0]
    elif values == "inf_tail":
        by_rank[max(1, (2 * k) // 3):] = -np.inf
    elif values == "rest_inf":
        keep = by_rank[top_ranks].copy()
        by_rank[:] = -np.inf
        by_rank[top_ranks] = keep
    elif values == "mx0":
        by_rank -= one
    elif values == "mxneg":
        by_rank -= dtype(1.5)
    elif values == "scaled":
        by_rank *= dtype(3.7)
    if cuts in (1, 2, 3):
        if m < 2 * cuts + 1:
            return None
        for j in np.sort(rng.choice((m - 1) // 2, cuts, replace=False)) * 2:    # non-adjacent gaps of the rest
            by_rank[rest[j + 1]] = np.nextafter(by_rank[rest[j]], dtype(-np.inf))
    elif cuts in ("index9", "one_exact"):
        # F[9] = 1.0 against the first of the rest: one step below the maximum (a cut point at index 9) or equal to it (none)
        if placement != "first" or m < 1 or values not in ("plain", "runs", "inf_tail"):
            return None
        by_rank[rest[0]] = np.nextafter(by_rank[0], dtype(0)) if cuts == "index9" else by_rank[0]
    elif cuts == "last2":
        if m < 3:
            return None
        by_rank[rest[m - 2]] = np.nextafter(by_rank[rest[m - 3]], dtype(-np.inf))
        by_rank[rest[m - 1]] = np.nextafter(by_rank[rest[m - 2]], dtype(-np.inf))
    perm = rng.permutation(D)
    row = np.empty(D, dtype=dtype)
    row[perm] = by_rank                                                     # document perm[r] has rank r (equal values: by id)
    return row, perm[top_ranks].astype(np.int32)


def planted_rows(D, k, rng, dtype=np.float64):
    out = []
    for placement in PLACEMENTS:
        for cuts in CUTS:
            for values in VALUES:
                case = planted_row(D, k, placement, cuts, values, rng, dtype)
                if case is not None:
                    out.append(((placement, cuts, values),) + case)
    return out
