#!/usr/bin/env python3
"""Grouping the character-feature index at the size the project is measured at: --rows x 768 unit rows (seed 47) around
--rows / 25 centres, noise scale 0.3, cut at 1 - cosine < 0.3 -- every group a clique of about 25, a few million neighbour pairs.

  (a) the new route      hipts_radius_create alone (both passes of the thresholded all-pairs product, the scan, the row sort),
                         and the whole CharacterFeatureIndex.cluster() call (that plus DBSCAN and the labels' copy back)
  (b) the parent's route Similarity.query over 256-row chunks into a device buffer, `1 - s < T` counted on the device by torch
                         (the count only: no lists are built, so (b) does LESS than (a))
Rows A B A B in one process: --warmup untimed rounds of both, then --repeats timed rounds, alternating.  Host clocks around calls
that end in a device synchronisation.  The pair counts of (a) and (b) are compared.  Algorithmic work of the product, printed with
the rates: (a) walks half the block pairs twice = 2 * (N^2 / 2) * K fused multiply-adds = 2 N^2 K flop over both passes; (b)
N^2 K fused multiply-adds once = 2 N^2 K flop.  Needs a GPU; there is no fallback."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "anime-illust-image-searcher_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from hiptagsearch import _lib, cfeatures  # noqa: E402

THRESHOLD = 0.3
SCALE = 0.3


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]), "n": len(a)}


def features(rows):
    rng = np.random.default_rng(47)
    centres = rng.standard_normal((max(1, rows // 25), 768)).astype(np.float32)
    feats = np.empty((rows, 768), dtype=np.float32)
    member = rng.integers(0, len(centres), rows)
    for s in range(0, rows, 20000):
        feats[s:s + 20000] = centres[member[s:s + 20000]] + SCALE * rng.standard_normal((min(20000, rows - s), 768)).astype(np.float32)
    return feats


def route_a_create(ci, t32):
    h = ctypes.c_void_p()
    t0 = time.perf_counter()
    _lib.call("hipts_radius_create", ci.index._h, ctypes.c_float(float(t32)), ctypes.c_int64(0), _lib.current_stream_ptr(), ctypes.byref(h))
    ms = (time.perf_counter() - t0) * 1e3                   # create ends in a stream synchronisation
    pairs = ctypes.c_int64()
    _lib.call("hipts_radius_info", h, None, ctypes.byref(pairs))
    _lib.call("hipts_radius_destroy", h)
    return ms, pairs.value


def route_b(ci, rows_host, t32, buf):
    n = len(rows_host)
    total = torch.zeros((), dtype=torch.int64, device=buf.device)
    one = torch.tensor(1.0, dtype=torch.float32, device=buf.device)
    thr = torch.tensor(float(t32), dtype=torch.float32, device=buf.device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(0, n, 256):
        q = rows_host[s:s + 256]
        out = buf[:len(q)]
        ci.index.query(q, out=out)
        total += ((one - out) < thr).sum()
    pairs = int(total.item())                               # synchronises
    return (time.perf_counter() - t0) * 1e3, pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cluster_bench needs a GPU")
    report = []

    def say(s):
        print(s, flush=True)
        report.append(s)

    N, K = args.rows, 768
    feats = features(N)
    ci = cfeatures.CharacterFeatureIndex(encoder=None)
    for s in range(0, N, 20000):
        ci.add_features(["img%06d.png" % i for i in range(s, min(N, s + 20000))], feats[s:s + 20000])
    rows_host = ci.index.matrix()
    t32 = np.float32(THRESHOLD)
    buf = torch.empty((256, N), dtype=torch.float32, device="cuda:0")
    say("cluster_bench: %d x %d rows, threshold %.2f, %d timed rounds after %d warm-up, rows A B A B" % (N, K, THRESHOLD, args.repeats, args.warmup))
    a_create, a_cluster, b_ms = [], [], []
    pairs_a = pairs_b = clusters = sweeps = None
    for it in range(args.warmup + args.repeats):
        ms_a, pairs_a = route_a_create(ci, t32)
        ms_b, pairs_b = route_b(ci, rows_host, t32, buf)
        t0 = time.perf_counter()
        labels = ci.cluster(t32, 2)
        ms_c = (time.perf_counter() - t0) * 1e3
        clusters, sweeps = ci.last_cluster_stats
        if it >= args.warmup:
            a_create.append(ms_a)
            a_cluster.append(ms_c)
            b_ms.append(ms_b)
        say("  round %d%s: (a) create %.1f ms, (b) chunked query + count %.1f ms, (a) cluster() %.1f ms"
            % (it, " (warm-up)" if it < args.warmup else "", ms_a, ms_b, ms_c))
    assert pairs_a == pairs_b, "pair counts differ: (a) %d, (b) %d" % (pairs_a, pairs_b)
    sa, sc, sb = stats(a_create), stats(a_cluster), stats(b_ms)
    flop = 2.0 * N * N * K                                  # both routes: see the docstring
    say("pairs under the threshold: %d (both routes agree); %d clusters, %d noise rows, %d sweeps" % (pairs_a, clusters, int((labels < 0).sum()), sweeps))
    say("(a) hipts_radius_create    median %9.2f ms  (min %.2f, max %.2f)  %.1f Tflop/s over 2 N^2 K flop (two passes of half the pairs)"
        % (sa["median_ms"], sa["min_ms"], sa["max_ms"], flop / sa["median_ms"] / 1e9))
    say("(a) cluster() whole call   median %9.2f ms  (min %.2f, max %.2f)" % (sc["median_ms"], sc["min_ms"], sc["max_ms"]))
    say("(b) chunked query + count  median %9.2f ms  (min %.2f, max %.2f)  %.1f Tflop/s over 2 N^2 K flop (every pair once, both orders)"
        % (sb["median_ms"], sb["min_ms"], sb["max_ms"], flop / sb["median_ms"] / 1e9))
    say(json.dumps({"cluster_bench": {"rows": N, "pairs": pairs_a, "clusters": clusters, "sweeps": sweeps, "a_create": sa, "a_cluster": sc, "b": sb}}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(report) + "\n")


if __name__ == "__main__":
    main()
