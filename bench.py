#!/usr/bin/env python3
"""bench.py -- headline benchmark of the hot path (BASELINE.json):
images/sec tagged (ViT-B/16 @448 forward + sigmoid + MCut tag selection, bf16 MFMA, batch 64 per
GPU, inputs resident in HBM) on N GPUs of one node.  With --full, also the per-kernel breakdown and
roofline, an output self-check, a sustained run and -- on rank 0 at N=1 -- CCIP, EVA02, the input
pipeline, top-k queries/sec over a 100k-document index and the CPU restatement ("port") timed on the
host cores.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One step = one pass of the tagging path over one batch of 64 synthetic images per rank
(config.workload).  Rank 0 prints ONE JSON line on stdout; everything else goes to stderr.
--dump-outputs DIR writes what the last timed step returned (rank 0): DIR/probs.npy (float32
[64, classes]) and DIR/tag_rows.npy (the int32 tag rows as float64, [N * 64, 256]).  Inputs are
seeded, so two runs with the same arguments see the same images and weights.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "anime-illust-image-searcher_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

MFMA_BF16_PEAK_TFLOPS = 2500.0      # MI355X dense bf16 (MI355X_MICROARCH.md)
HBM_PEAK_GBS = 8000.0
BATCH = 64
ROW_WIDTH = 2 + 254                 # int32 {n_general, n_character, ids[254]} per image (1 KiB rows)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def cpu_baseline_vit(cfg, weights, n_images=4, budget_s=12.0, check_images=None):
    """The oracle (torch CPU float32 restatement of the same forward) on a bounded sample.  With check_images (uint8 NHWC) the
    sample starts with those images and their logits are returned as the second value: the checker of output_check.oracle."""
    from oracle import vit as ovit
    from hiptagsearch import synth
    # One GPU of the box comes with a 16-core CPU share; more intra-op threads than that
    # oversubscribe it (measured on the GPU box: 16 thr 3.9 img/s, 32 thr 3.1, 64 thr 1.9, 128 thr 0.8).
    threads = int(os.environ.get("HIPTS_CPU_THREADS", min(os.cpu_count() or 1, 16)))
    torch.set_num_threads(threads)
    w = ovit.to_torch(weights)
    imgs = synth.images_u8(n_images, cfg["image_size"], seed=99)
    x = ovit.preprocess_u8_nhwc(imgs)
    kw = dict(patch=cfg["patch"], heads=cfg["heads"], eps=cfg["ln_eps"], gelu_kind="tanh" if cfg["gelu_tanh"] else "erf")
    ovit.vit_forward(w, x[:1], **kw)      # warm-up
    t0 = time.perf_counter()
    done = 0
    check_logits = None
    if check_images is not None:
        xc = ovit.preprocess_u8_nhwc(check_images)
        check_logits = ovit.vit_forward(w, xc, **kw)
        torch.sigmoid(check_logits)
        check_logits = check_logits.numpy()
        done += len(check_images)
    while True:
        torch.sigmoid(ovit.vit_forward(w, x, **kw))
        done += n_images
        el = time.perf_counter() - t0
        if el > budget_s:
            break
    return {"value": done / el, "unit": "images/sec", "cores": threads, "kind": "port",
            "sample": "%d images (ViT-B/16@448 fp32 torch-CPU oracle forward+sigmoid, batch %d), %.1f s" % (done, n_images, el)}, check_logits


def pmc_traffic(kernel_name):
    """HBM bytes per launch of `kernel_name` as recorded in profiles/pmc_traffic_latest.json -- the committed result of
    separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this same command (gfx950 correction 2*FETCH_SIZE +
    WRITE_SIZE; tools/pmc_traffic.py).  Hardware counters cannot be read from inside the process, so this is a LOOK-UP of an
    earlier profiling run, not a measurement of this one: the bench line says so in roofline.traffic_source."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic_latest.json")
    # template indices of the category's kernels (EPI_RESID: the plain residual epilogue and EPI_RESID_XG, which also prepares the
    # next LayerNorm and is what 23 of the 24 residual GEMMs of a forward run)
    epi = {"EPI_PATCH": (0,), "EPI_QK": (1,), "EPI_VT": (2,), "EPI_RESID": (3, 13), "EPI_GELU": (4,), "EPI_HEAD": (5,)}
    try:
        k = json.load(open(path))["kernels"]
        for tag, idxs in epi.items():
            if tag in kernel_name:
                best = None      # the template instance (tile height, operand type) with the most launches
                for name, v in k.items():
                    if name.startswith("gemm") and any("<%d>" % idx in name or "<%d," % idx in name for idx in idxs):
                        if best is None or v.get("launches_fetch_pass", 0) > best.get("launches_fetch_pass", 0):
                            best = v
                if best:
                    return best["hbm_bytes_per_launch"]
        return k[kernel_name]["hbm_bytes_per_launch"]
    except Exception:
        return None


def query_section(device):
    """top-k queries/sec over a 100k-document index (config[2]) + its CPU port baseline."""
    from hiptagsearch import synth
    from hiptagsearch.bm25 import BM25Index
    from hiptagsearch.index import Similarity
    from hiptagsearch.search import SearchEngine
    from oracle import bm25 as obm25
    from oracle import search as osearch
    D, V, K, NQ, TOPK = 100_000, 10_000, 300, 1024, 100
    t0 = time.perf_counter()
    ptr, terms = synth.tag_corpus(D, V, seed=42)
    rows = synth.index_vectors(D, K, seed=46)
    bm = BM25Index(ptr, terms, V, device)
    idx = Similarity("bench", None, K, device, capacity=D)
    idx.add_matrix(rows)
    eng = SearchEngine(None, idx, {}, bm, [])
    qs = [dict(q) for q in synth.queries(NQ, V, seed=43)]
    rng = np.random.default_rng(5)
    qv = rng.standard_normal((NQ, K))
    qv = (qv / np.linalg.norm(qv, axis=1, keepdims=True)).astype(np.float32)
    log("query corpus built in %.1f s" % (time.perf_counter() - t0))
    chunk = 256
    eng.score_topk(qs[:chunk], qv[:chunk], TOPK)                        # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(0, NQ, chunk):
        ids, vals = eng.score_topk(qs[s:s + chunk], qv[s:s + chunk], TOPK)
    torch.cuda.synchronize()
    batched_sync = NQ / (time.perf_counter() - t0)            # one batch at a time: the host's packing / launching / unpacking is not hidden
    # The serving loop (round 4): two batches in flight -- the host prepares and launches batch i + 1 while the device runs batch i
    # (SearchEngine.submit_topk / collect_topk = hipts_search_submit / _collect); same kernels, same results (asserted below).
    reps = 4
    starts = [s for _ in range(reps) for s in range(0, NQ, chunk)]
    t0 = time.perf_counter()
    pending = eng.submit_topk(qs[starts[0]:starts[0] + chunk], qv[starts[0]:starts[0] + chunk], TOPK, slot=0)
    for j in range(1, len(starts)):
        s = starts[j]
        nxt = eng.submit_topk(qs[s:s + chunk], qv[s:s + chunk], TOPK, slot=j & 1)
        pids, pvals = eng.collect_topk(pending)
        pending = nxt
    pids, pvals = eng.collect_topk(pending)
    batched = len(starts) * chunk / (time.perf_counter() - t0)
    assert np.array_equal(pids, ids) and pvals.tobytes() == vals.tobytes(), "pipelined batches differ from the synchronous call"
    for i in range(8):
        eng.score_topk(qs[i:i + 1], qv[i:i + 1], TOPK)                # warm-up of the one-query path (first launch loads its kernels)
    n_single = 256
    t0 = time.perf_counter()
    for i in range(n_single):
        eng.score_topk(qs[i:i + 1], qv[i:i + 1], TOPK)
    torch.cuda.synchronize()
    single = n_single / (time.perf_counter() - t0)
    # the same calls through the C ABI alone (hipts_search, nq = 1; arguments marshalled once per query beforehand, so this is the
    # library's latency without the Python mirror's per-call work)
    import ctypes as _ct
    from hiptagsearch import _lib as _l
    _fn = _l.load().hipts_search
    _ids, _vals = np.empty((1, TOPK), np.int32), np.empty((1, TOPK), np.float64)
    _calls = []
    for i in range(n_single):
        q = qs[i]
        qt = np.asarray(list(q.keys()) or [0], np.int32); qw = np.asarray(list(q.values()) or [0.0], np.float64)
        qp = np.asarray([0, len(q)], np.int32); v = np.ascontiguousarray(qv[i:i + 1])
        _calls.append(((qt, qw, qp, v), (bm._h, idx._h, _l.ptr(qt), _l.ptr(qw), _l.ptr(qp), _l.ptr(v), 1, _ct.c_double(0.5), _ct.c_double(0.5), TOPK,
                                        _l.ptr(_ids), _l.ptr(_vals), None, None)))
    for _, a in _calls[:8]:
        _fn(*a)
    t0 = time.perf_counter()
    for _, a in _calls:
        rc = _fn(*a)
    single_c_abi = n_single / (time.perf_counter() - t0)
    assert rc == 0
    # CPU port on a bounded sample (vectorised numpy BM25 + fma-chain similarity + stable sort)
    e = bm.export()
    nq_cpu = 4
    t0 = time.perf_counter()
    for i in range(nq_cpu):
        q = qs[i]
        b = obm25.bm25_score_csr(e["csr_ptr"], e["csr_term"], e["csr_tf"], e["idf"], bm.avgdl, e["doc_len"], list(q.keys()), list(q.values()))
        s = osearch.similarity(rows, qv[i])
        f = osearch.combine(b, s)
        wi, wv = osearch.topk(f, TOPK)
    cpu_qps = nq_cpu / (time.perf_counter() - t0)
    gi, _ = eng.score_topk(qs[nq_cpu - 1:nq_cpu], qv[nq_cpu - 1:nq_cpu], TOPK)
    assert np.array_equal(gi[0], wi), "GPU/CPU top-k mismatch"
    # Doc2Vec PV-DBOW inference of every document (genmodel.py:168-169): 100 epochs, 300-d, negative 5
    from hiptagsearch.d2v import Doc2VecInference
    from oracle import d2v as od2v
    m = synth.d2v_model(synth.term_counts(ptr, terms, V), dim=K, seed=44)
    v0, seeds = synth.d2v_inputs(D, K, seed=44)
    model = Doc2VecInference(m["syn1neg"], m["cum_table"], m["sample_int"], {}, epochs=100, device=device)
    n_gpu = 20_000
    model.infer_batch(ptr[:257], terms[:ptr[256]], v0[:256], seeds[:256])               # warm-up
    t0 = time.perf_counter()
    got = model.infer_batch(ptr[:n_gpu + 1], terms[:ptr[n_gpu]], v0[:n_gpu], seeds[:n_gpu])
    d2v_gpu = n_gpu / (time.perf_counter() - t0)
    n_cpu = 24
    t0 = time.perf_counter()
    want = od2v.infer(m["syn1neg"], m["cum_table"], m["sample_int"], ptr[:n_cpu + 1], terms[:ptr[n_cpu]], v0[:n_cpu], seeds[:n_cpu], 100)
    d2v_cpu = n_cpu / (time.perf_counter() - t0)
    assert got[:n_cpu].tobytes() == want.tobytes(), "GPU/CPU Doc2Vec vectors differ"
    # per-kernel roofline of the query path: HIP events on the launch stream around every kernel (hipts_query_profile_*),
    # ALGORITHMIC bytes per launch / event time against the HBM peak
    import ctypes
    from hiptagsearch import _lib

    def read_query_profile():
        out = []
        for c in range(9):
            ms, n, by = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
            _lib.call("hipts_query_profile_read", bm._h, c, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(by))
            name = ctypes.create_string_buffer(64)
            _lib.call("hipts_query_profile_name", c, name, 64)
            if n.value:
                gbs = by.value / (ms.value * 1e6) if ms.value else 0.0
                out.append({"kernel": name.value.decode(), "launches": n.value, "avg_us": 1e3 * ms.value / n.value,
                            "bytes_per_launch": by.value / n.value, "achieved": gbs, "frac": gbs / HBM_PEAK_GBS})
        return out
    _lib.call("hipts_query_profile_enable", bm._h, 1)
    for s in range(0, NQ, chunk):
        eng.score_topk(qs[s:s + chunk], qv[s:s + chunk], TOPK)
    prof_batched = read_query_profile()
    _lib.call("hipts_query_profile_enable", bm._h, 1)
    for i in range(64):
        eng.score_topk(qs[i:i + 1], qv[i:i + 1], TOPK)
    prof_single = read_query_profile()
    _lib.call("hipts_query_profile_enable", bm._h, 0)
    for c in prof_batched + prof_single:
        log("query %-26s n=%4d  avg %8.1f us  %8.1f GB/s  (%.3f of HBM peak)" % (c["kernel"], c["launches"], c["avg_us"], c["achieved"], c["frac"]))

    def dominant(prof):
        return max(prof, key=lambda c: c["avg_us"] * c["launches"]) if prof else None
    roof = {"bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "note": "achieved = algorithmic bytes per launch / HIP-event time of that launch, on the launch stream. Batched: the index product "
                    "(sim_mfma_wide_kernel, round 3) serves up to 256 queries with ONE pass over the index -- its bytes are the index once plus "
                    "the %d x D score rows, and at that many queries per pass it is bound by the exact-f32 MFMA rate (2 D K nq flop against "
                    "157 TFLOP/s: see 'sim_mfma'), not by HBM; bm25_postings_kernel / topk_kernel / rowmax / combine one launch per batch. "
                    "Single: the one-query path's four launches per query" % chunk,
            "batched": {"kernels": prof_batched}, "single": {"kernels": prof_single}}
    for c in prof_batched:
        if c["kernel"] == "sim_mfma_kernel":
            fl = 2.0 * D * K * chunk
            roof["sim_mfma"] = {"bound": "mfma (exact f32, v_mfma_f32_32x32x2_f32)", "flops_per_launch": fl, "avg_launch_us": c["avg_us"],
                                "achieved": fl / (c["avg_us"] * 1e6), "peak": 157.0, "unit": "TFLOP/s", "frac": fl / (c["avg_us"] * 1e6) / 157.0}
    for tag, prof in (("batched", prof_batched), ("single", prof_single)):
        d = dominant(prof)
        if d:
            roof[tag].update({"dominant_kernel": d["kernel"], "achieved": d["achieved"], "frac": d["frac"], "avg_launch_us": d["avg_us"],
                              "kernel_time_per_query_us": sum(c["avg_us"] * c["launches"] for c in prof) / (NQ if tag == "batched" else 64)})
    # bytes one query costs on each path (for the batched path the index pass is shared by 32 queries)
    # The whole query function as the web UI calls it (webui.py:586: find_similar_documents(query, topn=800)): parse, per-tag Doc2Vec
    # inference, fused scoring with top-1024, re-inference of the top-10 documents, rerank product, combine, rank, gap filter.
    toks = synth.vocab_tokens(V)
    lines = ["img%06d.png," % d_ + ",".join(toks[t] for t in terms[ptr[d_]:ptr[d_ + 1]]) for d_ in range(D)]
    full = SearchEngine(model, idx, {t: i for i, t in enumerate(toks)}, bm, lines)
    model.key_to_index = full.token2id
    qstrings = [synth.query_string(q, toks) for q in synth.queries(24, V, seed=47)]
    full.find_similar_documents(qstrings[0], topn=800)
    fs_ms = []
    for qs_ in qstrings[:20]:
        t0 = time.perf_counter()
        full.find_similar_documents(qs_, topn=800)
        fs_ms.append(1e3 * (time.perf_counter() - t0))
    fs_ms.sort()
    # Doc2Vec PV-DBOW training (genmodel.py:159-162), parallel schedule: 20k documents x 5 epochs of the bench corpus
    from hiptagsearch.d2v import Doc2Vec
    n_tr, ep_tr = 20_000, 5
    tr_docs = [[str(t) for t in terms[ptr[d]:ptr[d + 1]]] for d in range(n_tr)]
    tm = Doc2Vec(vector_size=K, window=50, min_count=1, workers=1, dm=0, device=device)
    tm.build_vocab(tr_docs)
    tm.train(tr_docs[:256] + [[]] * (n_tr - 256), epochs=1, mode="parallel")               # warm-up (kernel load)
    t0 = time.perf_counter()
    tm.train(tr_docs, total_examples=n_tr, epochs=ep_tr, mode="parallel")
    d2v_train = n_tr * ep_tr / (time.perf_counter() - t0)
    n_trc, ep_trc = 200, 2
    k2i, _, cum_c, si_c = od2v.build_vocab(tr_docs[:n_trc])
    p_c = np.cumsum([0] + [len(d) for d in tr_docs[:n_trc]]).astype(np.int64)
    i_c = np.array([k2i[t] for d in tr_docs[:n_trc] for t in d], dtype=np.int32)
    syn_c, dv_c = np.zeros((len(k2i), K), np.float32), od2v.init_doc_vectors(n_trc, K)
    t0 = time.perf_counter()
    od2v.train(syn_c, dv_c, cum_c, si_c, p_c, i_c, epochs=ep_trc)
    d2v_train_cpu = n_trc * ep_trc / (time.perf_counter() - t0)
    bytes_single = D * K * 4 + bm.nnz * 8 + D * (8 + 4 + 8 + 4) + D * 20 + D * 8
    bytes_batched = D * K * 4 / 32.0 + D * (8 * 3 + 4 + 4 + 20 + 8)
    return {"metric": "top-100 queries/sec over 100k-doc index (BM25 + 300-d index product, fused)",
            "batched_qps": batched_sync, "batched_pipelined_qps": batched, "metric_version": 2,
            "batched_note": "batched_qps: every call waits for its own result (the definition of rounds 1-3; round 4's lines printed the "
                            "pipelined figure under this key and this one as batched_one_at_a_time_qps); batched_pipelined_qps: two batches of "
                            "256 in flight (submit / collect: the host prepares batch i + 1 while the device runs batch i)",
            "single_query_qps": single, "single_query_c_abi_qps": single_c_abi, "batch": chunk,
            "roofline": roof,
            "algorithmic_bytes_per_query": {"single": bytes_single, "batched": bytes_batched,
                                            "note": "batched: one 120 MB index pass per 32 queries + per-query score rows (posting lists counted per launch in roofline)"},
            "cpu_port_qps": cpu_qps, "cpu_port_sample": "%d queries, numpy CSR BM25 + C fma-chain + lexsort, 1 thread" % nq_cpu,
            "d2v_infer_docs_per_s": d2v_gpu, "d2v_sample": "%d docs x 100 epochs, host buffers in/out" % n_gpu,
            "find_similar_documents_ms": {"median": fs_ms[len(fs_ms) // 2], "min": fs_ms[0], "max": fs_ms[-1],
                                          "sample": "20 queries of 1-4 tags, topn=800, 100-epoch inference of the query tags and of the top-10 documents",
                                          "full_rank_fallbacks": full.stats["full_rank_fallbacks"], "rank_continuations": full.stats["rank_continuations"]},
            "d2v_train_doc_epochs_per_s": d2v_train, "d2v_train_sample": "%d docs x %d epochs, parallel schedule, host arrays in/out" % (n_tr, ep_tr),
            "d2v_train_cpu_port_doc_epochs_per_s": d2v_train_cpu, "d2v_train_cpu_sample": "%d docs x %d epochs, C oracle, 1 thread (reference: workers=1)" % (n_trc, ep_trc),
            "d2v_cpu_port_docs_per_s": d2v_cpu, "d2v_cpu_sample": "%d docs, C oracle, 1 thread (reference: workers=1)" % n_cpu}


def ccip_section(device):
    """BASELINE.json configs[4]: CCIP encoder images/sec (CAFormer-B36 widths @384, bf16 MFMA) + rerank
    cosine queries/sec over 100k x 768 feature rows, with the CPU port of the encoder beside it."""
    from hiptagsearch import synth
    from hiptagsearch.cfeatures import CCIPEncoder
    from hiptagsearch.index import Similarity
    from oracle import ccip as occip
    cfg = dict(synth.CCIP_B36_384)
    w = synth.ccip_weights(cfg, seed=46)
    out = {"metric": "CCIP encoder images/sec (CAFormer-B36 @384, 16-bit MFMA operands) + rerank cosine queries/sec over 100k x 768"}
    # 20 = the reference's batch (gen_cfeatures.py:50); operands: IEEE half, the encoder's default (same matrix rate as bf16)
    for B, mode in ((20, 1), (64, 1)):
        enc = CCIPEncoder(dict(cfg, operand_f16=mode), w, max_batch=B, device=device)
        imgs = torch.randint(0, 256, (B, 384, 384, 3), dtype=torch.uint8, device="cuda")
        feats = torch.empty((B, 768), dtype=torch.float32, device="cuda")
        for _ in range(2):
            enc.forward_u8(imgs, out=feats)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 5
        for _ in range(n):
            enc.forward_u8(imgs, out=feats)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
        fl = enc.flops_per_image()
        tag = "batch%d" % B
        out["images_per_s_" + tag] = B / dt
        out["tflops_" + tag] = B * fl / dt / 1e12
        out["flops_per_image"] = fl
        del enc
    out["operands"] = "f16"
    out["e4m3_note"] = ("the e4m3 operand mode of rounds 1-3 (configs[4]'s fp8 leg) was withdrawn in round 4: cosine 0.968 to the float32 oracle, "
                        "1 % slower than 16-bit operands (2766 vs 2799 images/s), and no scaling scheme of the scaled MFMA lifts it above 0.995 "
                        "(tools/ccip_fp8_emulation.py; DESIGN.md section 6)")
    # CPU port: the float32 torch oracle on a bounded sample
    threads = int(os.environ.get("HIPTS_CPU_THREADS", min(os.cpu_count() or 1, 16)))
    torch.set_num_threads(threads)
    x = occip.preprocess_u8_nhwc(synth.images_u8(2, 384, seed=47))
    tw = occip.to_torch(w)
    occip.metaformer_forward(tw, x[:1], dims=cfg["dims"], depths=cfg["depths"])
    t0 = time.perf_counter()
    done = 0
    while time.perf_counter() - t0 < 8.0:
        occip.metaformer_forward(tw, x, dims=cfg["dims"], depths=cfg["depths"])
        done += 2
    out["cpu_port_images_per_s"] = done / (time.perf_counter() - t0)
    out["cpu_port_sample"] = "%d images, torch-CPU float32 oracle, %d threads" % (done, threads)
    # rerank: cosine of a query feature against 100k unit rows (webui.py:303-335 restated, configs[4])
    D = 100_000
    rng = np.random.default_rng(45)
    rows = rng.standard_normal((D, 768)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    idx = Similarity("ccip-bench", None, 768, device, capacity=D)
    idx.add_matrix(rows)
    q = rows[:64].copy()
    idx.query(q)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        sims = idx.query(q)
    torch.cuda.synchronize()
    out["rerank_queries_per_s_batch64"] = 640 / (time.perf_counter() - t0)
    t0 = time.perf_counter()
    for i in range(32):
        idx.query(q[i])
    out["rerank_queries_per_s_single"] = 32 / (time.perf_counter() - t0)
    assert int(np.argmax(sims[5])) == 5
    out["rerank_algorithmic_bytes_per_query"] = D * 768 * 4
    return out


def input_pipeline_section(device):
    """what one host core spends per image on decode alone and on decode + the transform's Resize(bicubic), and what the device
    resize (hipts_resize_u8, Pillow-exact) sustains -- 1024 x 768 JPEGs, the padded 1024^2 square resized to 448^2 (tagging.py:100-120,241)."""
    import io
    from PIL import Image
    from hiptagsearch.tagger import Predictor, device_resize_u8
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    blobs = []
    for i in range(24):
        buf = io.BytesIO()
        Image.fromarray(np.roll(base, i, axis=0)).resize((1024, 768), Image.BICUBIC).save(buf, format="JPEG", quality=90)
        blobs.append(buf.getvalue())
    pr = Predictor(device=device)

    def decode(b):
        img = Image.open(io.BytesIO(b))
        img.load()
        return pr.prepare_image(img)
    decode(blobs[0])
    t0 = time.perf_counter()
    padded = [decode(b) for b in blobs]
    t_dec = (time.perf_counter() - t0) / len(blobs)
    t0 = time.perf_counter()
    for im in padded:
        np.asarray(im.resize((448, 448), Image.BICUBIC), dtype=np.uint8)
    t_res = (time.perf_counter() - t0) / len(blobs)
    arrs = [torch.from_numpy(np.asarray(im, dtype=np.uint8)).cuda() for im in padded]
    out = torch.empty((448, 448, 3), dtype=torch.uint8, device="cuda:%d" % device)
    for a in arrs[:4]:
        device_resize_u8(a, 448, 448, 3, device, out=out)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(4):
        for a in arrs:
            device_resize_u8(a, 448, 448, 3, device, out=out)
    torch.cuda.synchronize()
    t_gpu = (time.perf_counter() - t0) / (4 * len(arrs))
    res = {"sample": "%d JPEGs 1024x768 (quality 90), padded to 1024^2, resized to 448^2 bicubic; one host core" % len(blobs),
           "host_decode_only_images_per_s_per_core": 1.0 / t_dec, "host_decode_plus_resize_images_per_s_per_core": 1.0 / (t_dec + t_res),
           "host_resize_share_of_decode_plus_resize": t_res / (t_dec + t_res),
           "device_resize_images_per_s": 1.0 / t_gpu, "device_resize_note": "hipts_resize_u8, source already on the device, one call per image"}
    # hybrid JPEG decode (round 4): the host keeps the Huffman decoding (per core), the device does the rest of libjpeg + pad + resize (per batch)
    from hiptagsearch import _lib
    lib = _lib.load()
    n = len(blobs)
    stride = int(lib.hipts_jpeg_slot_bytes(1024, 768))
    slots = torch.empty((n, stride), dtype=torch.uint8).pin_memory()
    srcs = [np.frombuffer(b, dtype=np.uint8) for b in blobs]

    def entropy_all():
        for i, a in enumerate(srcs):
            if lib.hipts_jpeg_entropy_decode(a.ctypes.data, len(a), slots[i].numpy().ctypes.data, stride) != 0:
                raise RuntimeError("bench: the entropy decoder refused a file Pillow wrote")
    entropy_all()
    t0 = time.perf_counter()
    for _ in range(3):
        entropy_all()
    t_ent = (time.perf_counter() - t0) / (3 * n)
    kinds = np.ones(n, np.int32)
    hw = np.ascontiguousarray(np.tile(np.asarray([[768, 1024]], np.int32), (n, 1)))
    outb = torch.empty((n, 448, 448, 3), dtype=torch.uint8, device="cuda:%d" % device)
    st = torch.cuda.current_stream(device).cuda_stream

    def batch():
        _lib.call("hipts_jpeg_batch_u8", slots.data_ptr(), stride, _lib.ptr(kinds), _lib.ptr(hw), n, 1, _lib.ptr(outb), 448, 3, device, st)
    batch()
    torch.cuda.synchronize()
    want = np.stack([np.asarray(im.resize((448, 448), Image.BICUBIC), dtype=np.uint8) for im in padded])
    if not np.array_equal(outb.cpu().numpy(), want):
        raise AssertionError("bench: hybrid JPEG decode + device resize differ from Pillow's decode + resize")
    t0 = time.perf_counter()
    for _ in range(5):
        batch()
    torch.cuda.synchronize()
    t_dev = (time.perf_counter() - t0) / (5 * n)
    res["hybrid_jpeg"] = {"host_entropy_decode_images_per_s_per_core": 1.0 / t_ent, "host_speedup_over_pillow_decode": t_dec / t_ent,
                          "device_idct_upsample_rgb_pad_resize_images_per_s": 1.0 / t_dev,
                          "note": "csrc/jpeg_host.c (Huffman decoding, in the worker processes) + csrc/jpeg.hip (libjpeg's IDCT, fancy upsampling, colour "
                                  "conversion) + resize.hip; device rate includes the pinned host -> device copies of the coefficient slots; "
                                  "output checked equal to Pillow's decode + resize in this run; end to end: profiles/r04_pipeline_e2e.txt"}
    return res


def eva_section(device, oracle_check=False):
    """The model the reference really loads (tagging.py:45): EVA02-L/14 @448, 723.5 GFLOP/image.  oracle_check (the cpu_baseline leg): the
    trained-like checkpoint's logits on a noise and a flat image against the float32 CPU oracle, absolute and rms-relative."""
    from hiptagsearch import synth
    from hiptagsearch.tagger import EvaTagger
    cfg = dict(synth.EVA02_L14_448)
    w = synth.eva_weights(cfg, seed=0)
    out = {"metric": "images/sec tagged, EVA02-L/14 @448 forward + sigmoid (IEEE-half MFMA operands: EvaTagger's default, same matrix rate as bf16)"}
    for B in (10, 32):                                   # 10 = the reference's batch (tagging.py:49)
        m = EvaTagger(cfg, w, max_batch=B, device=device)
        imgs = torch.randint(0, 256, (B, 448, 448, 3), dtype=torch.uint8, device="cuda")
        probs = torch.empty((B, cfg["num_classes"]), dtype=torch.float32, device="cuda")
        for _ in range(2):
            m.forward_u8(imgs, probs=probs, want="probs")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 4
        for _ in range(n):
            m.forward_u8(imgs, probs=probs, want="probs")
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
        fl = m.flops_per_image()
        out["images_per_s_batch%d" % B] = B / dt
        out["tflops_batch%d" % B] = B * fl / dt / 1e12
        out["flops_per_image"] = fl
        m.close()
    out["published_reference"] = "0.59 images/sec CPU (Ryzen 7 5700X), ~2 images/sec GTX 1660 SUPER (reference README, this model)"
    if oracle_check:
        from oracle import eva as oeva
        wt = synth.eva_weights(cfg, seed=0, trained_like=True)
        chk = np.concatenate([synth.images_u8(1, 448, seed=5), synth.structured_images_u8(448, seed=77, kinds=("flat",))])
        m = EvaTagger(cfg, wt, max_batch=2, device=device)
        got, _ = m.forward_u8(chk, want="logits")
        m.close()
        t0 = time.perf_counter()
        from oracle import vit as ovit
        want = oeva.eva_forward(oeva.to_torch(wt), ovit.preprocess_u8_nhwc(chk), patch=cfg["patch"], heads=cfg["heads"], eps=cfg["ln_eps"],
                                ref_grid=cfg["rope_ref_grid"]).numpy()
        if want is not None:
            d = got.astype(np.float64) - want.astype(np.float64)
            rms_l = np.sqrt((want.astype(np.float64) ** 2).mean(axis=1))
            out["oracle_check"] = {"checkpoint": "trained-like", "images": ["noise", "flat"], "logit_rms": float(rms_l.mean()),
                                   "max_abs_logit_error": [float(v) for v in np.abs(d).max(axis=1)],
                                   "rms_relative_logit_error": [float(v) for v in np.sqrt((d ** 2).mean(axis=1)) / rms_l],
                                   "cpu_oracle_seconds": time.perf_counter() - t0}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: per-kernel breakdown and roofline (HIP events in the timed region), output "
                         "self-check, sustained run, kernel-alone pass, CCIP / EVA02 / input pipeline / query sections, CPU baselines, --precise")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (rank 0) as DIR/probs.npy and DIR/tag_rows.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines, the oracle check and --precise")
    ap.add_argument("--no-query", action="store_true", help="with --full: skip the CCIP, EVA02, input pipeline and query sections")
    ap.add_argument("--no-exclusive", action="store_true",
                    help="with --full: skip the kernel-alone pass after the timed region (profiler runs: keeps per-launch averages to the "
                         "timed launches)")
    ap.add_argument("--operands", choices=["bf16", "f16"], default="f16",
                    help="16-bit MFMA operand type: f16 (default, the product's: IEEE half, same MFMA rate as bf16, 8x smaller activation "
                         "rounding -- inside the 1e-3 logit tolerance on flat images too) or bf16 (BASELINE.json configs[1]'s wording)")
    ap.add_argument("--checkpoint", choices=["trained-like", "random-init"], default="trained-like",
                    help="synthetic checkpoint: trained-like (peaked attention with a heavy tail, logit rms ~10, sparse probabilities, tens "
                         "of labels per image) or the plain random init of rounds 1-2 (logit rms 0.35, ~3000 labels 'selected')")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        log("warning: WORLD_SIZE=%d but --gpus %d; using WORLD_SIZE" % (world, args.gpus))
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("HIPTS_BENCH_BACKEND", "nccl")      # "gloo": rehearsal of the N > 1 control flow on a one-GPU box
        if backend == "nccl":
            dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            local_rank = 0                                            # every rank shares the one GPU
            dist.init_process_group(backend=backend, rank=rank, world_size=world)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    import hiptagsearch  # noqa: F401  (raises if libhip_tagsearch.so is missing: no CPU fallback)
    from hiptagsearch import synth
    from hiptagsearch.tagger import TagSelector, ViTTagger
    from hiptagsearch import _lib
    import ctypes

    cfg = dict(synth.VIT_B16_448)
    cfg["operand_f16"] = 1 if args.operands == "f16" else 0
    weights = synth.vit_weights(cfg, seed=0, trained_like=args.checkpoint == "trained-like")
    model = ViTTagger(cfg, weights, max_batch=BATCH, device=local_rank)
    names, cat = synth.label_table(cfg["num_classes"])
    selector = TagSelector(cat, max_batch=BATCH, device=local_rank)

    # the synthetic corpus is generated ON THE DEVICE by a counter-based generator keyed by the GLOBAL image
    # index (hipts_synth_images_u8) -- rank r holds images r * 64 .. r * 64 + 63 of corpus 1234, and any rank can reproduce any image
    # (the order check of the gathered rows below does).
    CORPUS_SEED = 1234

    def corpus_images(first, count):
        buf = torch.empty((count, cfg["image_size"], cfg["image_size"], 3), dtype=torch.uint8, device=dev)
        _lib.call("hipts_synth_images_u8", _lib.ptr(buf), ctypes.c_int64(first), ctypes.c_int64(count), cfg["image_size"], ctypes.c_uint64(CORPUS_SEED),
                  local_rank, _lib.current_stream_ptr())
        return buf
    images = corpus_images(rank * BATCH, BATCH)
    probs = torch.empty((BATCH, cfg["num_classes"]), dtype=torch.float32, device=dev)
    rows = torch.zeros((BATCH, ROW_WIDTH), dtype=torch.int32, device=dev)
    gathered = torch.empty((world * BATCH, ROW_WIDTH), dtype=torch.int32, device=dev) if world > 1 else None

    # One step = forward + tag selection (+ all-gather).  The selection of step i (64 workgroups, ~0.25 ms, LDS sorts)
    # runs on a side stream while the forward of step i+1 already occupies the main stream, as a tagging loop
    # over many batches does; probabilities and rows are double-buffered and every hand-over is an event, so
    # nothing is skipped: all K selections and gathers have completed at the final synchronize.
    side = torch.cuda.Stream(device=dev)
    probs2 = [probs, torch.empty_like(probs)]
    rows2 = [rows, torch.zeros_like(rows)]
    ev_fwd = [torch.cuda.Event(), torch.cuda.Event()]
    ev_sel = [torch.cuda.Event(), torch.cuda.Event()]
    counter = [0]
    deferred = not os.environ.get("HIPTS_BENCH_SERIAL_SELECT") and not os.environ.get("HIPTS_BENCH_JOIN")
    _lib.call("hipts_vit_set_deferred_join", model._h, 1 if deferred else 0)

    def step():
        b = counter[0] & 1
        counter[0] += 1
        main = torch.cuda.current_stream()
        main.wait_event(ev_sel[b])                                        # step i-2's selection has released buffer b
        model.forward_u8(images, probs=probs2[b], want="probs")          # patchify ... head + sigmoid
        ev_fwd[b].record(main)
        with torch.cuda.stream(main if os.environ.get("HIPTS_BENCH_SERIAL_SELECT") else side):     # A/B switch
            torch.cuda.current_stream().wait_event(ev_fwd[b])
            if deferred:                                                  # the forward's two halves join HERE, not on main
                _lib.call("hipts_vit_join", model._h, _lib.current_stream_ptr())
            selector.run_device(probs2[b], rows2[b])                      # MCut selection -> fixed-width tag rows
            if world > 1:
                dist.all_gather_into_tensor(gathered, rows2[b])           # RCCL: rank order == file order
            ev_sel[b].record(torch.cuda.current_stream())

    def step_local():
        b = counter[0] & 1
        counter[0] += 1
        main = torch.cuda.current_stream()
        main.wait_event(ev_sel[b])
        model.forward_u8(images, probs=probs2[b], want="probs")
        ev_fwd[b].record(main)
        with torch.cuda.stream(side):
            side.wait_event(ev_fwd[b])
            if deferred:
                _lib.call("hipts_vit_join", model._h, _lib.current_stream_ptr())
            selector.run_device(probs2[b], rows2[b])
            ev_sel[b].record(side)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    # --full: HIP events inside the timed region, around the launches of the DOMINANT kernel only (the residual GEMM: 48 of a step's
    # ~130 launches), every 3rd step -- events around every launch cost 0.7 % of the step time (HIPTS_BENCH_PROFILE_ALL=1: as before).
    # The per-kernel breakdown (`kernels`) comes from three extra steps after the timed region, run the same way.  A plain run records
    # no events.
    if args.full:
        DOM_NAME = "gemm_kernel<EPI_RESID>"
        dom_cat = -1
        for c in range(11):
            nm = ctypes.create_string_buffer(64)
            _lib.call("hipts_vit_profile_name", c, nm, 64)
            if nm.value.decode() == DOM_NAME:
                dom_cat = c
        profile_all = bool(os.environ.get("HIPTS_BENCH_PROFILE_ALL")) or dom_cat < 0
        _lib.call("hipts_vit_profile_select", model._h, ctypes.c_uint32(0xffffffff if profile_all else (1 << dom_cat)))
        _lib.call("hipts_vit_profile_enable", model._h, int(os.environ.get("HIPTS_BENCH_PROFILE_EVERY", "3")))
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # what the last timed step returned to its caller: the probabilities and the tag rows (all ranks' rows, gathered, at N > 1)
    if rank == 0 and args.dump_outputs:
        b_last = (counter[0] - 1) & 1
        out_rows = gathered if world > 1 else rows2[b_last]
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "probs.npy"), probs2[b_last].cpu().numpy().astype(np.float32))
        np.save(os.path.join(args.dump_outputs, "tag_rows.npy"), out_rows.cpu().numpy().astype(np.float64))

    imgs_per_s = world * BATCH * args.steps / elapsed
    flops_img = model.flops_per_image()
    result = {
        "metric": "images/sec tagged (ViT fwd)", "value": imgs_per_s, "unit": "images/sec", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.operands,
        "dtype_note": ("IEEE-half MFMA operands (v_mfma_f32_16x16x32_f16), fp32 accumulation / residual stream / LayerNorm / softmax "
                       "statistics; the bf16 checkpoint's matrices are exact in half.  Same matrix rate as the bf16 operands BASELINE.json "
                       "names (--operands bf16 runs those: outside the 1e-3 logit tolerance on flat images)") if args.operands == "f16"
                      else "bf16 MFMA operands, fp32 accumulation",
        "data": "synthetic (%s checkpoint, uniform-noise u8 images)" % args.checkpoint,
        "config": {"workload": "wd-tagger ViT-B/16 448px 16-bit-operand forward + sigmoid + MCut tag selection, batch 64 per GPU, "
                               "u8 NHWC images resident in HBM (BASELINE.json configs[1])",
                   "batch_per_gpu": BATCH, "image": "448x448x3 u8", "classes": cfg["num_classes"],
                   "parallelism": "dp%d (images sharded by rank, RCCL all-gather of tag rows)" % world if world > 1 else "single GPU",
                   "flops_per_image": flops_img},
        "model_tflops": imgs_per_s * flops_img / 1e12 / world,
        "model_mfma_frac": imgs_per_s * flops_img / 1e12 / world / MFMA_BF16_PEAK_TFLOPS,
        "full": args.full,
    }
    if not args.full:
        if world > 1:
            dist.destroy_process_group()
        if rank == 0:
            print(json.dumps(result), flush=True)
        return

    # per-kernel device time from the HIP events recorded on the launch stream during the timed steps
    def read_categories():
        out = []
        for c in range(11):
            ms, n, fl, by = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
            _lib.call("hipts_vit_profile_read", model._h, c, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl), ctypes.byref(by))
            name = ctypes.create_string_buffer(64)
            _lib.call("hipts_vit_profile_name", c, name, 64)
            if n.value:
                out.append({"kernel": name.value.decode(), "launches": n.value, "total_ms": ms.value,
                            "avg_us": 1e3 * ms.value / n.value, "tflops": fl.value / (ms.value * 1e9) if ms.value else 0.0,
                            "gbs": by.value / (ms.value * 1e6) if ms.value else 0.0, "flops": fl.value, "bytes": by.value})
        return out

    cats_timed = read_categories()
    _lib.call("hipts_vit_profile_enable", model._h, 0)
    if profile_all:
        cats = cats_timed
        breakdown_steps = (args.steps + 2) // 3
    else:       # the full breakdown: three more steps, every launch bracketed (outside the timed region; same streams, same deferred join)
        _lib.call("hipts_vit_profile_select", model._h, ctypes.c_uint32(0xffffffff))
        _lib.call("hipts_vit_profile_enable", model._h, 1)
        breakdown_steps = 3
        for _ in range(breakdown_steps):
            step_local()
        torch.cuda.synchronize()
        cats = read_categories()
        _lib.call("hipts_vit_profile_enable", model._h, 0)

    # What the timed steps produced is checked AFTER the clock stopped: the tag rows of the last step (two sub-batch streams,
    # deferred join, side-stream selection) must equal those of a fresh single-stream, joined forward + selection of the same images.
    last_rows = rows2[(counter[0] - 1) & 1].clone()
    check = {}
    if rank == 0:
        _lib.call("hipts_vit_set_deferred_join", model._h, 0)
        _lib.call("hipts_vit_set_sub_batches", model._h, 1)
        ref_probs = torch.empty_like(probs)
        ref_rows = torch.zeros_like(rows)
        model.forward_u8(images, probs=ref_probs, want="probs")
        selector.run_device(ref_probs, ref_rows)
        torch.cuda.synchronize()
        same_rows = bool(torch.equal(ref_rows, last_rows))
        same_probs = bool(torch.equal(ref_probs, probs2[(counter[0] - 1) & 1]))
        # (HIPTS_GEMM_SPLITK >= 2, an opt-in A/B mode, gives up exactly this property: which tiles are summed as partial chains depends on
        # the launch's size, so the two-stream and the one-stream forward differ in low bits.  Rows still have to agree.)
        if int(os.environ.get("HIPTS_GEMM_SPLITK", "0")) >= 2:
            assert same_rows, "timed-region tag rows differ from a fresh single-stream forward"
        else:
            assert same_rows and same_probs, "timed-region outputs differ from a fresh single-stream forward"
        check = {"rows_equal_single_stream_forward": same_rows, "probs_bit_equal": same_probs,
                 "tags_selected_per_image_mean": float((last_rows[:, 0] + last_rows[:, 1]).float().mean().item())}
        if world > 1:
            # ORDER of the all-gathered rows: rank 0 regenerates images that OTHER ranks tagged (first and last image of every rank's batch:
            # global indices r * 64 and r * 64 + 63), tags them itself and compares with the rows at those positions of `gathered`
            idx = sorted({r * BATCH + o for r in range(world) for o in (0, BATCH - 1)})
            spot = torch.cat([corpus_images(i, 1) for i in idx])
            sp_probs = torch.empty((len(idx), cfg["num_classes"]), dtype=torch.float32, device=dev)
            sp_rows = torch.zeros((len(idx), ROW_WIDTH), dtype=torch.int32, device=dev)
            model.forward_u8(spot, probs=sp_probs, want="probs")
            selector.run_device(sp_probs, sp_rows)
            torch.cuda.synchronize()
            got = gathered[torch.as_tensor(idx, device=dev)]
            order_ok = bool(torch.equal(got, sp_rows))
            assert order_ok, "all-gathered tag rows are not in rank order == corpus order"
            check["gathered_rows_in_corpus_order"] = {"ok": order_ok, "global_indices_recomputed_on_rank0": idx}
        _lib.call("hipts_vit_set_sub_batches", model._h, 0)
        _lib.call("hipts_vit_set_deferred_join", model._h, 1 if deferred else 0)

    # Sustained rate: the driver-timed window above is short (K steps of ~12 ms); dense MFMA work is power-limited and the clock sags
    # under sustained load, so the same step is run for >= 300 more steps (outside the timed region) and reported beside `value`.
    sustained = {}
    if rank == 0 and not os.environ.get("HIPTS_BENCH_NO_SUSTAINED"):
        n_sus = int(os.environ.get("HIPTS_BENCH_SUSTAINED_STEPS", "300"))
        marks = []
        torch.cuda.synchronize()
        ts = time.perf_counter()
        for i in range(n_sus):
            step_local()
            if (i + 1) % 100 == 0:
                torch.cuda.synchronize()
                marks.append(time.perf_counter())
        torch.cuda.synchronize()
        te = time.perf_counter()
        prev = ts
        per100 = []
        for m in marks:
            per100.append(BATCH * 100 / (m - prev))
            prev = m
        sustained = {"steps": n_sus, "images_per_s": BATCH * n_sus / (te - ts), "ms_per_step": 1e3 * (te - ts) / n_sus,
                     "images_per_s_per_100_steps": per100, "seconds": te - ts,
                     "note": "same step as the timed region, forward + selection only (no collective), run after it on rank 0"}
    # After the timed region: the same kernels with the chip to themselves (one sub-batch = the whole batch on
    # one stream).  In the timed region two sub-batch streams run concurrently, so a launch's duration there
    # includes the time it shares CUs with the other stream's kernel; this pass gives the kernel-alone figure.
    excl = []
    _lib.call("hipts_vit_set_deferred_join", model._h, 0)
    if rank == 0 and not args.no_exclusive:
        _lib.call("hipts_vit_set_sub_batches", model._h, 1)
        model.forward_u8(images, probs=probs, want="probs")      # forward only: no collective outside the timed region
        torch.cuda.synchronize()
        _lib.call("hipts_vit_profile_enable", model._h, 1)
        for _ in range(3):
            model.forward_u8(images, probs=probs, want="probs")
        torch.cuda.synchronize()
        excl = read_categories()
        _lib.call("hipts_vit_set_sub_batches", model._h, 0)
    _lib.call("hipts_vit_profile_enable", model._h, 0)

    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return

    for c in cats:
        log("%-26s n=%5d  avg %9.1f us  %8.1f TFLOP/s  %8.1f GB/s  (%.1f%% of step time)" % (
            c["kernel"], c["launches"], c["avg_us"], c["tflops"], c["gbs"],
            100 * c["total_ms"] / breakdown_steps / (elapsed * 1e3 / args.steps)))
    gemms = [c for c in cats if c["kernel"].startswith("gemm_kernel")]
    dom = max(gemms, key=lambda c: c["total_ms"])
    if not profile_all:          # the roofline's launch time is the one measured INSIDE the timed region
        timed_dom = [c for c in cats_timed if c["kernel"] == dom["kernel"]]
        assert timed_dom, "the dominant kernel (%s) is not the one recorded in the timed region (%s)" % (dom["kernel"], DOM_NAME)
        dom = timed_dom[0]
    roofline = {"bound": "mfma", "kernel": dom["kernel"], "achieved": dom["tflops"], "peak": MFMA_BF16_PEAK_TFLOPS,
                "unit": "TFLOP/s", "frac": dom["tflops"] / MFMA_BF16_PEAK_TFLOPS, "traffic": pmc_traffic(dom["kernel"]),
                "traffic_source": "profiles/pmc_traffic_latest.json (committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command; "
                                  "looked up, not measured in this run)",
                "avg_launch_us": dom["avg_us"], "launches": dom["launches"],
                "all_gemm_tflops": sum(c["flops"] for c in gemms) / (sum(c["total_ms"] for c in gemms) * 1e9),
                "measured": "HIP events on the launch streams around this kernel's launches of every 3rd step of the timed region; the other "
                            "kernels of `kernels` in three extra steps after it",
                "note": "timed region: 2 sub-batch streams, each launch (32 images) shares the chip with the other stream's "
                        "kernel, so achieved/frac are per launch UNDER that concurrency (rocprofv3 durations agree); "
                        "'exclusive' = the same kernel over the whole batch with the chip to itself, measured after the timed region. "
                        "The LayerNorms are folded into the GEMM epilogues (+3.4 % images/s): this kernel (EPI_RESID_XG, 23 of the 24 "
                        "residual GEMMs of a forward) also writes the next LayerNorm's 16-bit gamma*x operand and row sums, work that "
                        "used to be 47 separate HBM-bound launches per forward, so its own launch takes 207 instead of 174 us for the "
                        "same algorithmic flops while the forward is faster; HIPTS_LN_FOLD=0 restores the separate kernels"}
    # the shader clock the chip sustains inside the GEMM main loop (in-kernel cycle counter against the 100 MHz wall clock): the
    # nominal peak assumes 2.4 GHz, dense MFMA work runs power-limited well below it
    try:
        lib = _lib.load()
        lib.hiptsdbg_gemm_clock.argtypes = [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_float)] * 2
        clocks = {}
        for tag, (gm, gn, gk, ge) in {"resid_k768": (BATCH * 784, 768, 768, 3), "resid_k3072": (BATCH * 784, 768, 3072, 3),
                                      "gelu_k768": (BATCH * 784, 3072, 768, 4)}.items():
            ms_, ghz = ctypes.c_float(), ctypes.c_float()
            if lib.hiptsdbg_gemm_clock(gm, gn, gk, ge, 20, ctypes.byref(ms_), ctypes.byref(ghz)) == 0 and ghz.value > 0:
                clocks[tag] = round(ghz.value, 3)
        if clocks:
            lo = min(clocks.values())
            roofline["clock"] = {"nominal_ghz": 2.4, "main_loop_ghz": clocks,
                                 "peak_at_measured_clock_tflops": MFMA_BF16_PEAK_TFLOPS * lo / 2.4,
                                 "note": "20 back-to-back launches per shape, standalone; peak_at_measured_clock scales the 2.5 PF "
                                         "nominal peak by the lowest of these clocks"}
    except Exception as e:
        roofline["clock"] = {"error": repr(e)}
    ex = [c for c in excl if c["kernel"] == dom["kernel"]]
    if ex:
        egemms = [c for c in excl if c["kernel"].startswith("gemm_kernel")]
        roofline["exclusive"] = {"achieved": ex[0]["tflops"], "frac": ex[0]["tflops"] / MFMA_BF16_PEAK_TFLOPS,
                                 "avg_launch_us": ex[0]["avg_us"], "launches": ex[0]["launches"],
                                 "all_gemm_tflops": sum(c["flops"] for c in egemms) / (sum(c["total_ms"] for c in egemms) * 1e9),
                                 "kernels": [{k: c[k] for k in ("kernel", "launches", "avg_us", "tflops", "gbs")} for c in excl]}
    result.update({
        "roofline": roofline,
        "output_check": check,
        "sustained": sustained,
        "kernels": [{k: c[k] for k in ("kernel", "launches", "avg_us", "tflops", "gbs")} for c in cats],
    })
    if world == 1 and not args.no_query:
        # before the CPU baselines: their 16 spinning intra-op threads slow the ~600 launches of a two-stream CCIP forward
        try:
            result["ccip"] = ccip_section(local_rank)
        except Exception as e:
            result["ccip"] = {"error": repr(e)}
        try:
            result["eva02_large"] = eva_section(local_rank, oracle_check=not args.no_cpu_baseline)
        except Exception as e:
            result["eva02_large"] = {"error": repr(e)}
    if world == 1 and not args.no_query:
        try:
            result["input_pipeline"] = input_pipeline_section(local_rank)
        except Exception as e:
            result["input_pipeline"] = {"error": repr(e)}
    if world == 1 and not args.no_cpu_baseline:
        # the oracle as the CHECKER of what the benched configuration computes on structured images (flat, posterised, gradient, line
        # art, half flat, flat tiles) and two noise images -- its forward over them is also the first part of the CPU sample
        kinds = list(synth.STRUCTURED_KINDS) + ["noise", "noise"]
        chk = np.concatenate([synth.structured_images_u8(cfg["image_size"], seed=77), synth.images_u8(2, cfg["image_size"], seed=5)])
        got, _ = model.forward_u8(chk, want="logits")
        result["cpu_baseline"], want = cpu_baseline_vit(cfg, weights, check_images=chk)
        result["cpu_baseline"]["published_reference"] = "0.59 images/sec (README: EVA02-L tagger on Ryzen 7 5700X; different model and hardware)"
        d = got.astype(np.float64) - want.astype(np.float64)
        rms_l = np.sqrt((want.astype(np.float64) ** 2).mean(axis=1))
        result["output_check"]["oracle"] = {
            "images": kinds, "logit_rms": float(np.sqrt((want.astype(np.float64) ** 2).mean())),
            "max_abs_logit_error": [float(v) for v in np.abs(d).max(axis=1)],
            "rms_logit_error": [float(v) for v in np.sqrt((d ** 2).mean(axis=1))],
            "rms_relative_logit_error": [float(v) for v in np.sqrt((d ** 2).mean(axis=1)) / rms_l],
            "note": "GPU logits of the benched model (same handle, operands and checkpoint) against the float32 CPU oracle"}
        # the product's --precise mode (tagging.py --precise, Predictor(precise=True): operand_f16 |= 16, the attention output as a hi | lo
        # pair of halves): the same oracle check and the same loop as the timed region, so the record carries what the 1e-3 tolerance costs
        try:
            cfg_p = dict(cfg, operand_f16=cfg["operand_f16"] | 16)
            model_p = ViTTagger(cfg_p, weights, max_batch=BATCH, device=local_rank)
            got_p, _ = model_p.forward_u8(chk, want="logits")
            d_p = got_p.astype(np.float64) - want.astype(np.float64)

            def loop_rate(m, n=20):
                for _ in range(3):
                    m.forward_u8(images, probs=probs, want="probs")
                    selector.run_device(probs, rows)
                torch.cuda.synchronize()
                t0_ = time.perf_counter()
                for _ in range(n):
                    m.forward_u8(images, probs=probs, want="probs")
                    selector.run_device(probs, rows)
                torch.cuda.synchronize()
                return BATCH * n / (time.perf_counter() - t0_)
            r_def = loop_rate(model)
            r_pre = loop_rate(model_p)
            result["precise"] = {
                "switch": "tagging.py --precise / Predictor(precise=True) / hipts_vit_config_t.operand_f16 |= 16 (HIPTS_OPERAND_SPLIT_ATT)",
                "images_per_s": r_pre, "images_per_s_default_same_loop": r_def, "relative": r_pre / r_def,
                "loop": "20 steps of forward + selection on one stream, after the timed region (the default mode measured the same way beside it)",
                "oracle": {"images": kinds, "max_abs_logit_error": [float(v) for v in np.abs(d_p).max(axis=1)],
                           "rms_relative_logit_error": [float(v) for v in np.sqrt((d_p ** 2).mean(axis=1)) / rms_l]}}
            del model_p
        except Exception as e:
            result["precise"] = {"error": repr(e)}
    if world == 1 and not args.no_query:
        try:
            result["query"] = query_section(local_rank)
        except Exception as e:   # the headline line must still be printed
            result["query"] = {"error": repr(e)}
    if world > 1:
        dist.destroy_process_group()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
