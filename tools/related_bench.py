#!/usr/bin/env python3
"""Related tags (BM25Index.related, csrc/related.hip) against what a user could do before it existed: the same answer on the host from
BM25Index.export() with numpy -- a boolean match mask from the postings, np.bincount over the matching rows' terms, the score and a
sort.  The corpus is the one of bench.py's query section (synth.tag_corpus: 100 000 documents, 10 000 tags).

Cases: one query on the most frequent term; one on a term with df ~ 100; a three-term conjunction; a batch of 256 one-term queries;
the full table (every term, k = 16).  Per case the rounds alternate host, device, host, device in one process on one box.  Device
figures are HIP-event times around whole calls (they end in a synchronisation) after a warm-up call; beside them the HIP-event time of
the count launches alone and the work items (workgroups) per arm of the count kernel (hiptsdbg_related_last).  The host's table is
timed on every --host-table-stride-th term and scaled.  A second part runs the short-list cases with the direct-arm limit
(HIPTS_RELATED_DIRECT_MAX) at 0 (every list through the LDS histogram), 256 (the default) and 4096, alternating.
Needs a GPU; there is no fallback."""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "anime-illust-image-searcher_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from hiptagsearch import _lib, synth  # noqa: E402
from hiptagsearch.bm25 import BM25Index  # noqa: E402


class HostIndex:
    """What the host answer needs, built once from export(): the postings (term-major) beside the rows"""
    def __init__(self, e):
        self.ptr, self.term, self.df = e["csr_ptr"], e["csr_term"], e["df"]
        self.D, self.V = len(self.ptr) - 1, len(self.df)
        self.doc_of = np.repeat(np.arange(self.D, dtype=np.int32), np.diff(self.ptr))
        order = np.argsort(self.term, kind="stable")
        self.tdoc = self.doc_of[order]
        self.tptr = np.concatenate([[0], np.cumsum(self.df)])

    def related(self, include, exclude, k, min_count=1):
        mask = np.ones(self.D, dtype=bool)
        for t in include:
            m = np.zeros(self.D, dtype=bool)
            m[self.tdoc[self.tptr[t]:self.tptr[t + 1]]] = True
            mask &= m
        for t in exclude:
            mask[self.tdoc[self.tptr[t]:self.tptr[t + 1]]] = False
        n = int(mask.sum())
        if len(include) == 1 and not exclude:                    # the rows of one posting list: no mask over all entries needed
            docs = self.tdoc[self.tptr[include[0]]:self.tptr[include[0] + 1]]
            lens = self.ptr[docs + 1] - self.ptr[docs]
            pos = np.repeat(self.ptr[docs] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(int(lens.sum()))
            c = np.bincount(self.term[pos], minlength=self.V)
        else:
            c = np.bincount(self.term[mask[self.doc_of]], minlength=self.V)
        c[list(include) + list(exclude)] = 0
        u = np.flatnonzero(c >= max(min_count, 1))
        s = c[u] / (n + self.df[u] - c[u]).astype(np.float64)
        top = np.lexsort((u, -s))[:k]
        return u[top], s[top], c[u][top], n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20, help="device calls per timed round (the table: 1)")
    ap.add_argument("--host-table-stride", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "related_tags.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("related_bench needs a GPU")
    report = []

    def say(s):
        print(s, flush=True)
        report.append(s)

    D, V = args.docs, 10_000
    ptr, terms = synth.tag_corpus(D, V, seed=42)
    bm = BM25Index(ptr, terms, V, 0)
    host = HostIndex(bm.export())
    last = _lib.load().hiptsdbg_related_last
    last.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]

    def arms():
        ms, a, b = ctypes.c_double(), ctypes.c_int64(), ctypes.c_int64()
        _lib.check(last(bm._h, ctypes.byref(ms), ctypes.byref(a), ctypes.byref(b)))
        return ms.value, a.value, b.value

    by_df = np.argsort(-host.df, kind="stable")
    t_top = int(by_df[0])
    t_100 = int(np.argmin(np.abs(host.df - 100)))
    used = by_df[:int((host.df > 0).sum())]
    batch = [int(t) for t in used[np.linspace(0, len(used) - 1, 256).astype(int)]]
    cases = [("most frequent term (df %d)" % host.df[t_top], [([t_top], [])], 20),
             ("term with df %d" % host.df[t_100], [([t_100], [])], 20),
             ("three-term conjunction (df %s)" % ", ".join(str(host.df[t]) for t in by_df[:3]), [([int(t) for t in by_df[:3]], [])], 20),
             ("256 one-term queries (df %d .. %d)" % (host.df[batch[-1]], host.df[batch[0]]), [([t], []) for t in batch], 20),
             ("table: all %d terms, k = 16" % V, [([t], []) for t in range(V)], 16)]
    say("related_bench: %d documents, %d terms, %d postings (mean row %.1f terms), jaccard, min_count 1; %d rounds host / device alternating"
        % (D, V, len(host.term), len(host.term) / D, args.rounds))

    def device_ms(queries, k, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            got = bm.related(queries, k, "jaccard", 1)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps, got

    for name, queries, k in cases:
        table = len(queries) == V
        reps = 1 if table else args.reps
        hq = queries[::args.host_table_stride] if table else queries
        _, got = device_ms(queries, k, 1)                        # warm-up (workspaces grow here)
        for (inc, exc), row_i, row_s, row_c, n in zip(hq, got[0][::args.host_table_stride] if table else got[0],
                                                      got[1][::args.host_table_stride] if table else got[1],
                                                      got[2][::args.host_table_stride] if table else got[2],
                                                      got[3][::args.host_table_stride] if table else got[3]):
            u, s, c, hn = host.related(inc, exc, k)
            m = len(u)
            assert hn == n and (row_i[:m] == u).all() and (row_s[:m] == s).all() and (row_c[:m] == c).all() and (row_i[m:] == -1).all(), name
        h_ms, d_ms, c_ms = [], [], []
        for r in range(args.rounds):
            t0 = time.perf_counter()
            for inc, exc in hq:
                host.related(inc, exc, k)
            h_ms.append(1e3 * (time.perf_counter() - t0) * (len(queries) / len(hq)))
            ms, _ = device_ms(queries, k, reps)
            d_ms.append(ms)
            c_ms.append(arms()[0])
        _, lds_items, direct_items = arms()
        say("%s" % name)
        say("  host numpy   ms per call: %s   median %.3f%s" % (" ".join("%.3f" % x for x in h_ms), float(np.median(h_ms)),
                                                                "  (timed on every %d-th term, scaled)" % args.host_table_stride if table else ""))
        say("  device       ms per call: %s   median %.3f   (%.1f x)" % (" ".join("%.3f" % x for x in d_ms), float(np.median(d_ms)),
                                                                        float(np.median(h_ms)) / float(np.median(d_ms))))
        say("  count launches alone, ms: %s   work items: %d LDS histogram arm, %d direct arm" % (" ".join("%.3f" % x for x in c_ms), lds_items, direct_items))

    say("direct-arm limit (HIPTS_RELATED_DIRECT_MAX): device ms per call / count launches alone ms, rounds alternating 0, 256, 4096")
    for name, queries, k in (cases[1], cases[3], cases[4]):
        reps = 1 if len(queries) == V else args.reps
        res = {lim: [] for lim in (0, 256, 4096)}
        for r in range(args.rounds):
            for lim in res:
                os.environ["HIPTS_RELATED_DIRECT_MAX"] = str(lim)
                if r == 0:
                    device_ms(queries, k, 1)
                ms, _ = device_ms(queries, k, reps)
                res[lim].append((ms, arms()))
        os.environ.pop("HIPTS_RELATED_DIRECT_MAX")
        say("%s" % name)
        for lim, rows in res.items():
            say("  limit %4d: %s   (%d LDS items, %d direct items)" % (lim, " ".join("%.3f/%.3f" % (ms, a[0]) for ms, a in rows), rows[-1][1][1], rows[-1][1][2]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(report) + "\n")


if __name__ == "__main__":
    main()
