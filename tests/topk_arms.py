"""Which arm of topk_kernel (csrc/topk.h) a score row reaches: the kernel's decisions restated in numpy, and the table of rows the
top-k arm tests use.  The constants mirror topk.h; test_topk_arms_host.py asserts that every case still reaches the arm it is named
for, so a retuned constant cannot quietly turn a case into a duplicate of another."""
import math
import zlib

import numpy as np

CAP, SORT_TARGET, WSLOTS, OVCAP, FAST_MIN_N, COUNT_RANK_MAX = 2048, 256, 128, 1024, 8192, 640
NINF_KEY = np.uint64(0x000FFFFFFFFFFFFF)


def order_key(x):
    u = (np.asarray(x, np.float64) + 0.0).view(np.uint64)           # + 0.0: -0.0 and +0.0 share an image
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def value_digit(x):
    with np.errstate(invalid="ignore"):
        t = (np.asarray(x, np.float64) + 2.0) * 1024.0
        return np.where(t >= 4095.0, 4095, np.where(t > 0.0, np.minimum(t, 4095.0), 0.0)).astype(np.int64)


def _bin_from_top(hist, want):
    """(digit, count above it, its size) of the bin where the running count from the top first reaches `want`; None if it never does"""
    run = np.cumsum(hist[::-1])
    j = int(np.searchsorted(run, want))
    return None if j == len(hist) else (len(hist) - 1 - j, int(run[j] - hist[::-1][j]), int(hist[::-1][j]))


def predict(row, k):
    """The kernel's path for one row of hipts_topk (rows 16-byte aligned), as a dict of what it decides on the way."""
    n, k = len(row), min(k, len(row))
    key, i = order_key(row), np.arange(len(row))
    r = dict(fast_tried=n >= FAST_MIN_N, fast_ok=False, wide=n % 2 == 0, fill=0, passes=0, shortcut=False, tie_take=0)
    if r["fast_tried"]:
        d = value_digit(row)
        # the 1/8 sample: one histogram entry per thread, the largest digit among its samples
        sampled, thread = (i % 16384 < 2048, i % 16384 // 2) if r["wide"] else (i % 8192 < 1024, i % 8192)
        tmax = np.full(1024, -1)
        np.maximum.at(tmax, thread[sampled], d[sampled])
        want = k // 8 + 3 * math.ceil(math.sqrt(np.float32(k) / np.float32(8.0))) + 4
        hit = _bin_from_top(np.bincount(tmax[tmax >= 0], minlength=4096), want)
        r["dip"] = hit is None or hit[0] == 0
        cand = d >= (1 if r["dip"] else hit[0])
        wave = (i % 2048 // 128) if r["wide"] else (i % 1024 // 64)
        r["overflow"] = int(np.maximum(np.bincount(wave[cand], minlength=16) - WSLOTS, 0).sum())
        r["cnt"] = CAP + 1 if r["overflow"] > OVCAP else int(cand.sum())
        if r["dip"]:
            r["fast_ok"] = r["cnt"] <= CAP and (cand.all() or key[~cand].max() == NINF_KEY)
            r["fill"] = max(k - r["cnt"], 0) if r["fast_ok"] else 0
        else:
            r["fast_ok"] = k <= r["cnt"] <= CAP
    if not r["fast_ok"]:
        # exact radix select: 12-bit digits from the top (the last one 4 bits), until the survivors fit
        live, need, pbits, fits = np.ones(n, bool), k, 0, False
        for shift, dbits in ((52, 12), (40, 12), (28, 12), (16, 12), (4, 12), (0, 4)):
            dg = ((key >> np.uint64(shift)) & np.uint64((1 << dbits) - 1)).astype(np.int64)
            digit, above, size = _bin_from_top(np.bincount(dg[live], minlength=4096), need)
            live &= dg == digit
            need, pbits, r["passes"] = need - above, pbits + dbits, r["passes"] + 1
            fits = (k - need) + size <= (max(SORT_TARGET, k + 64) if pbits < 64 else CAP)
            if fits:
                break
            if pbits == 12 and size > CAP and key[live].min() == key[live].max():
                r["shortcut"] = True
                break
        r["cnt"] = (k - need) + size if fits else k
        r["tie_take"] = 0 if fits else need
    r["rank"] = "counting" if r["cnt"] <= COUNT_RANK_MAX else "bitonic"
    return r


def _sparse(rng, n, count, lo, hi, rest):
    v = np.full(n, rest, np.float64)
    v[rng.choice(n, count, replace=False)] = lo + (hi - lo) * rng.random(count)
    return v


def _uniform(rng, n):
    return rng.random(n)


def _three_kinds(rng, n):                 # the rows of test_topk_random
    v = rng.random((3, n))
    v[1, rng.integers(0, n, n // 3)] = -np.inf
    v[2] = np.round(v[2], 2)
    return v


def _skewed(rng, n):                      # one wave of the collect holds several times its 128 slots
    v = rng.random(n)
    hot = np.arange(n) % 2048 < 128
    v[hot] = v[hot] ** 0.25
    return v


# name -> (row builder, n, k, what predict() must say about every row)
CASES = {
    "below_floor_k100": (_uniform, 8191, 100, dict(fast_tried=False)),
    "below_floor_k1024": (_uniform, 8191, 1024, dict(fast_tried=False)),
    "fast_wide_counting": (_uniform, 8192, 100, dict(fast_ok=True, wide=True, dip=False, overflow=0, rank="counting")),
    "fast_short_of_k": (_uniform, 8192, 1024, dict(fast_tried=True, fast_ok=False, dip=False, overflow=0)),
    "fast_narrow_8193_k100": (_three_kinds, 8193, 100, dict(fast_ok=True, wide=False, rank="counting")),
    "fast_narrow_8193_k1024": (_three_kinds, 8193, 1024, dict(fast_ok=True, wide=False, rank="bitonic")),
    "fast_narrow_100001_k100": (_three_kinds, 100_001, 100, dict(fast_ok=True, wide=False, rank="counting")),
    "fast_narrow_100001_k1024": (_three_kinds, 100_001, 1024, dict(fast_ok=True, wide=False, rank="bitonic")),
    "overflow_list": (_skewed, 131_072, 1024, dict(fast_ok=True, wide=True, dip=False, overflow=lambda o: 0 < o <= OVCAP)),
    "dip_inf_fill": (lambda rng, n: _sparse(rng, n, 300, 0.0, 1.0, -np.inf), 100_000, 1024, dict(fast_ok=True, dip=True, cnt=300, fill=724)),
    "sparse_no_dip": (lambda rng, n: _sparse(rng, n, 300, 0.0, 1.0, -np.inf), 100_000, 100, dict(fast_ok=True, dip=False, fill=0)),
    "dip_refused_one_value": (lambda rng, n: _sparse(rng, n, 300, 0.0, 1.0, -5.0), 100_000, 1024,
                              dict(fast_tried=True, fast_ok=False, dip=True, passes=1, shortcut=True, tie_take=724)),
    "overflow_overflows_ties": (lambda rng, n: _sparse(rng, n, 500, 0.75, 1.0, 0.75), 50_000, 1024,
                                dict(fast_tried=True, fast_ok=False, overflow=lambda o: o > OVCAP, passes=6, shortcut=False, tie_take=524)),
    "ties_without_fast_path": (lambda rng, n: _sparse(rng, n, 500, 0.75, 1.0, 0.75), 5000, 1024,
                               dict(fast_tried=False, passes=6, shortcut=False, tie_take=524)),
}


def rows(name):
    """The case's score rows, [rows][n] float64: fixed by a seed made from the case's name."""
    build, n, _, _ = CASES[name]
    return np.atleast_2d(build(np.random.default_rng(zlib.crc32(name.encode())), n))
