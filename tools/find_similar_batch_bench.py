#!/usr/bin/env python3
"""The whole query function for a batch against a loop of single calls, at the size the project is measured at: the bench corpus of
bench.py's query section (100 000 documents, 10 000 tags, 300-d index rows, Doc2Vec inference with 100 epochs), the 24 query
strings of synth.queries(seed 47) repeated to --batch (256), topn = 800 as the web UI calls it (webui.py:586).

Per round, alternating on ONE engine in one process:
  (a) SearchEngine.find_similar_documents_batch(queries, 800)
  (b) [SearchEngine.find_similar_documents(q, 800) for q in queries]           (the only form before the batch entry point existed)
Host clocks around calls that return host lists (each ends in a device synchronisation).  Reports queries/s of both (median over the
rounds, with min and max), the single reruns of the batch, whether the results are equal, and where the batch call's time goes:
the two inference calls, the first-stage search, stage 4 (index pass, combine, ranking, finishing kernel) and the host
arithmetic that remains.  Needs a GPU; there is no fallback."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "anime-illust-image-searcher_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from hiptagsearch import synth  # noqa: E402
from hiptagsearch.bm25 import BM25Index  # noqa: E402
from hiptagsearch.d2v import Doc2VecInference  # noqa: E402
from hiptagsearch.index import Similarity  # noqa: E402
from hiptagsearch.search import SearchEngine  # noqa: E402


class Timed:
    """Wraps a bound method: sums the host time and the calls spent in it."""
    def __init__(self, fn):
        self.fn, self.s, self.n = fn, 0.0, 0

    def __call__(self, *a, **kw):
        t0 = time.perf_counter()
        try:
            return self.fn(*a, **kw)
        finally:
            self.s += time.perf_counter() - t0
            self.n += 1

    def take(self):
        s, n = self.s, self.n
        self.s, self.n = 0.0, 0
        return s, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--topn", type=int, default=800)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "find_similar_batch.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("find_similar_batch_bench needs a GPU")
    report = []

    def say(s):
        print(s, flush=True)
        report.append(s)

    D, V, K = args.docs, 10_000, 300
    ptr, terms = synth.tag_corpus(D, V, seed=42)
    rows = synth.index_vectors(D, K, seed=46)
    bm = BM25Index(ptr, terms, V, 0)
    idx = Similarity("bench", None, K, 0, capacity=D)
    idx.add_matrix(rows)
    toks = synth.vocab_tokens(V)
    token2id = {t: i for i, t in enumerate(toks)}
    m = synth.d2v_model(synth.term_counts(ptr, terms, V), dim=K, seed=44)
    model = Doc2VecInference(m["syn1neg"], m["cum_table"], m["sample_int"], token2id, epochs=args.epochs, device=0)
    lines = ["img%06d.png," % d + ",".join(toks[t] for t in terms[ptr[d]:ptr[d + 1]]) for d in range(D)]
    eng = SearchEngine(model, idx, token2id, bm, lines)
    base = [synth.query_string(q, toks) for q in synth.queries(24, V, seed=47)]
    queries = [base[i % len(base)] for i in range(args.batch)]
    say("find_similar_batch_bench: %d documents x %d-d, %d-epoch inference, %d queries (%d distinct strings), topn %d, %d rounds"
        % (D, K, args.epochs, len(queries), len(base), args.topn, args.rounds))
    # warm-up of every shape the timed window uses
    eng.find_similar_documents_batch(queries, args.topn)
    for q in base:
        eng.find_similar_documents(q, args.topn)
    infer = model.infer_vectors = Timed(model.infer_vectors)
    search = eng.score_topk = Timed(eng.score_topk)
    stage4 = eng._rerank_finish_batch = Timed(eng._rerank_finish_batch)
    batch_s, single_s, parts = [], [], []
    equal = True
    for r in range(args.rounds):
        reruns0 = eng.stats["batch_single_reruns"]
        for t in (infer, search, stage4):
            t.take()
        t0 = time.perf_counter()
        got = eng.find_similar_documents_batch(queries, args.topn)
        t1 = time.perf_counter()
        parts.append((infer.take(), search.take(), stage4.take()))
        reruns = eng.stats["batch_single_reruns"] - reruns0
        t2 = time.perf_counter()
        want = [eng.find_similar_documents(q, args.topn) for q in queries]
        t3 = time.perf_counter()
        batch_s.append(t1 - t0)
        single_s.append(t3 - t2)
        equal = equal and got == want
        say("round %d: batch %8.1f ms (%8.0f queries/s, %d single reruns)   loop of single calls %8.1f ms (%7.0f queries/s)"
            % (r, 1e3 * (t1 - t0), len(queries) / (t1 - t0), reruns, 1e3 * (t3 - t2), len(queries) / (t3 - t2)))
    nq = len(queries)
    bq, sq = sorted(nq / np.asarray(batch_s)), sorted(nq / np.asarray(single_s))
    say("batch call:            median %8.0f queries/s  (min %.0f, max %.0f)" % (float(np.median(bq)), bq[0], bq[-1]))
    say("loop of single calls:  median %8.0f queries/s  (min %.0f, max %.0f)" % (float(np.median(sq)), sq[0], sq[-1]))
    say("ratio of the medians:  %.2f x   results equal: %s   single reruns per batch: %d   mean result length %.0f"
        % (float(np.median(bq)) / float(np.median(sq)), equal, reruns, float(np.mean([len(g) for g in got]))))
    # where the batch call's time goes (median round by total time)
    mid = int(np.argsort(batch_s)[len(batch_s) // 2])
    (inf_s, inf_n), (se_s, se_n), (s4_s, s4_n) = parts[mid]
    total = batch_s[mid]
    say("batch call of round %d, %.1f ms:" % (mid, 1e3 * total))
    say("  model.infer_vectors        %2d calls %8.1f ms  (query tags once, top-ten documents once; + 2 per single rerun)" % (inf_n, 1e3 * inf_s))
    say("  score_topk (hipts_search)  %2d calls %8.1f ms  (+ 1 per single rerun)" % (se_n, 1e3 * se_s))
    say("  stage 4                    %2d calls %8.1f ms  (index pass, combine, hipts_topk, hipts_rerank_finish, lists)" % (s4_n, 1e3 * s4_s))
    say("  remaining host work                 %8.1f ms  (parsing, query vectors, rerank queries, single reruns' host part)"
        % (1e3 * (total - inf_s - se_s - s4_s)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(report) + "\n")
    if not equal:
        raise SystemExit("the batch call and the single calls returned different results")


if __name__ == "__main__":
    main()
