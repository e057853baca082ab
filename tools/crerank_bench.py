#!/usr/bin/env python3
"""Character-oriented rerank (webui.py:303-335) at the size the project is measured at: 100 000 x 768 unit rows (seed 45), planted
near-duplicate clusters of 10, 300 and 5000 rows, tag lists from the SURVEY section 8(d) document generator (synth.tag_corpus).

Per cluster size, median and spread (max - min; also p10 / p90) over --queries queries, after --warmup untimed ones, of
  (a) the host path      cfeatures.cfeatures_rerank                      (product on the device, threshold / tags / sort on the host)
  (b) the device path    cfeatures.DeviceReranker.rerank                 (the same list, every survivor read back)
  (c) for context        re-encoding the ten query images: gen_image_ndarray + CCIP encoder, one image at a time as
                         SearchEngine._cfeatures_rerank does
  (d) for comparison     ranking the same number of survivors with hipts_topk + hipts_topk_after, 1024 at a time
(a) and (b) alternate inside one loop and their results are compared.  Host clocks around calls that end in a device
synchronisation (both paths return host lists).  In a tree without DeviceReranker only (a) and (c) run, so the same file measures
the parent commit.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "anime-illust-image-searcher_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from hiptagsearch import _lib, cfeatures, synth  # noqa: E402

CLUSTERS = [(10, 20000), (300, 40000), (5000, 60000)]          # (size, first row); the centre is the row before the first
THRESHOLD = 0.2
EXCLUDE = ["t00005"]                                            # one popular tag, so that the survivors' tag lists are read


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "spread_ms": float(a[-1] - a[0]), "p10_ms": float(a[int(0.1 * (len(a) - 1))]),
            "p90_ms": float(a[int(round(0.9 * (len(a) - 1)))]), "min_ms": float(a[0]), "max_ms": float(a[-1]), "n": len(a)}


def corpus(R):
    rng = np.random.default_rng(45)
    feats = rng.standard_normal((R, 768)).astype(np.float32)
    for size, first in CLUSTERS:
        eps = rng.uniform(0.05, 0.3, (size, 1)).astype(np.float32)
        feats[first:first + size] = feats[first - 1] + eps * rng.standard_normal((size, 768)).astype(np.float32)
    ptr, terms = synth.tag_corpus(R, 10_000, seed=42)
    toks = synth.vocab_tokens(10_000)
    paths = ["img%06d.png" % i for i in range(R)]
    lines = [paths[d] + "," + ",".join(toks[t] for t in dict.fromkeys(terms[ptr[d]:ptr[d + 1]].tolist())) for d in range(R)]
    return feats, paths, lines


def topk_after_ms(n, R, scores, device=0):
    """(d): rank n finite float64 scores among R (the rest -inf) with the existing 1024-at-a-time continuation."""
    from ctypes import c_double, c_int64
    rng = np.random.default_rng(1)
    vals = np.full(R, -np.inf)
    vals[rng.permutation(R)[:n]] = scores
    dev = torch.from_numpy(vals).to("cuda:%d" % device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    k = min(1024, R)
    ids = np.empty((1, k), dtype=np.int32)
    out = np.empty((1, k), dtype=np.float64)
    _lib.call("hipts_topk", _lib.ptr(dev), 1, c_int64(R), k, _lib.ptr(ids), _lib.ptr(out), _lib.HOST, device, _lib.current_stream_ptr())
    ranked = k
    while ranked < n:
        _lib.call("hipts_topk_after", _lib.ptr(dev), c_int64(R), k, c_double(float(out[0, -1])), c_int64(int(ids[0, -1])), _lib.ptr(ids),
                  _lib.ptr(out), device, _lib.current_stream_ptr())
        ranked += k
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-encoder", action="store_true")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("crerank_bench needs a GPU")
    assert args.queries >= 20, "at least 20 timed queries"
    R = args.rows
    report = []

    def say(s):
        print(s, flush=True)
        report.append(s)

    feats, paths, lines = corpus(R)
    ci = cfeatures.CharacterFeatureIndex(encoder=lambda x: np.zeros((len(x), 768), np.float32))
    for s in range(0, R, 20000):
        ci.add_features(paths[s:s + 20000], feats[s:s + 20000])
    tags = {l.split(",")[0]: {t: True for t in l.split(",")[1:]} for l in lines}
    docid = {l.split(",")[0]: i for i, l in enumerate(lines)}
    have_dev = hasattr(cfeatures, "DeviceReranker")
    rr = cfeatures.DeviceReranker(ci, lines) if have_dev else None
    say("crerank_bench: %d x 768 rows, threshold %.2f, excluded %s, %d timed queries after %d warm-up, device path %s"
        % (R, THRESHOLD, EXCLUDE, args.queries, args.warmup, "present" if have_dev else "ABSENT (host path only)"))
    top10 = [(i, 1.0) for i in range(10)]
    rng = np.random.default_rng(7)
    results = {}
    for size, first in CLUSTERS:
        host_ms, dev_ms, after_ms, counts, mismatches = [], [], [], [], 0
        for it in range(args.warmup + args.queries):
            members = first + rng.choice(size, 10, replace=size < 10)
            qf = [feats[m] for m in members]
            t0 = time.perf_counter()
            host = cfeatures.cfeatures_rerank(top10, qf, ci, tags, docid, [], EXCLUDE, THRESHOLD)
            t1 = time.perf_counter()
            dev = rr.rerank(top10, qf, [], EXCLUDE, THRESHOLD) if have_dev else None
            t2 = time.perf_counter()
            if have_dev and dev != host:
                mismatches += 1
            if it >= args.warmup:
                host_ms.append((t1 - t0) * 1e3)
                dev_ms.append((t2 - t1) * 1e3)
                counts.append(len(host) - 10)
                if have_dev and len(host) > 10:
                    after_ms.append(topk_after_ms(len(host) - 10, R, [s for _, s in host[10:]]))
        r = {"cluster": size, "survivors_median": int(np.median(counts)), "host": stats(host_ms)}
        say("cluster %5d (survivors: median %d)" % (size, r["survivors_median"]))
        say("  (a) host path      median %9.3f ms  spread %8.3f ms  (p10 %.3f, p90 %.3f)" % tuple(r["host"][k] for k in ("median_ms", "spread_ms", "p10_ms", "p90_ms")))
        if have_dev:
            r["device"] = stats(dev_ms)
            r["mismatches"] = mismatches
            r["topk_after"] = stats(after_ms) if after_ms else None
            d = r["device"]
            say("  (b) device path    median %9.3f ms  spread %8.3f ms  (p10 %.3f, p90 %.3f)  results differ from (a): %d of %d"
                % (d["median_ms"], d["spread_ms"], d["p10_ms"], d["p90_ms"], mismatches, args.warmup + args.queries))
            margin = r["host"]["median_ms"] - d["median_ms"] - (r["host"]["spread_ms"] + d["spread_ms"])
            say("      host median - device median - (both spreads) = %.3f ms  -> %s" % (margin, "device path wins" if margin > 0 else "NOT beyond the spreads"))
            if after_ms:
                say("  (d) hipts_topk + hipts_topk_after over the same survivors (ranking only)  median %9.3f ms  spread %8.3f ms"
                    % (r["topk_after"]["median_ms"], r["topk_after"]["spread_ms"]))
            # algorithmic bytes of one device query: the index, sim and row_doc per row, the tag ids of the rows that pass the threshold
            tag_bytes = 4 * sum(len(tags[paths[i]]) for i in range(first - 1, first + size))
            r["algorithmic_bytes"] = R * 768 * 4 + R * 8 + tag_bytes
        results[size] = r
    if not args.skip_encoder:
        from PIL import Image
        cfg = dict(synth.CCIP_B36_384)
        enc = cfeatures.CCIPEncoder(cfg, synth.ccip_weights(cfg, seed=46), max_batch=1)
        ci.encoder = enc
        tmp = tempfile.mkdtemp(prefix="crerank_bench_")
        irng = np.random.default_rng(2)
        files = []
        for i in range(10):
            p = os.path.join(tmp, "q%02d.png" % i)
            Image.fromarray(irng.integers(0, 256, (768, 768, 3), dtype=np.uint8)).save(p)
            files.append(p)
        enc_ms = []
        for it in range(args.warmup + args.queries):
            t0 = time.perf_counter()
            for p in files:
                ci.ccip_batch_extract_features([cfeatures.gen_image_ndarray(p, ci.image_size)])[0]
            if it >= args.warmup:
                enc_ms.append((time.perf_counter() - t0) * 1e3)
        e = stats(enc_ms)
        results["encoder"] = e
        say("(c) re-encoding ten 768 x 768 PNG query images (gen_image_ndarray + CCIP CAFormer-B36 at 384, batch 1 each): median %.3f ms  spread %.3f ms"
            % (e["median_ms"], e["spread_ms"]))
        for size, _ in CLUSTERS:
            r = results[size]
            line = "    share of (c) in encode + rerank, cluster %5d: host path %.1f %%" % (size, 100 * e["median_ms"] / (e["median_ms"] + r["host"]["median_ms"]))
            if have_dev:
                line += ", device path %.1f %%" % (100 * e["median_ms"] / (e["median_ms"] + r["device"]["median_ms"]))
            say(line)
    say(json.dumps({"crerank_bench": {str(k): v for k, v in results.items()}, "rows": R, "device_path": have_dev}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(report) + "\n")


if __name__ == "__main__":
    main()
