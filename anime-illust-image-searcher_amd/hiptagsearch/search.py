"""Query function: host-side mirror of webui.py:63-390 over the device kernels.

  filter_searched_result                webui.py:63-80
  normalize_and_apply_weight_doc2vec    webui.py:82-117
  find_similar_documents                webui.py:345-390   (same name / arguments / return value)
  get_doc2vec_based_reranked_scores     webui.py:189-253

The reference keeps model, index, dictionary and the BM25 statistics in module globals that
`load_model()` fills (webui.py:649-689); here they live in a SearchEngine, and the module-level
functions of the same names operate on the engine installed with `set_engine()`.
Scoring (BM25, index product, normalise, combine, top-k) runs in libhip_tagsearch.so; parsing,
the 10-document pseudo-relevance bookkeeping and the gap filter are host logic on the one-query path; for a batch
(find_similar_documents_batch) the bookkeeping after the second ranking and the gap filter are one kernel, hipts_rerank_finish.
"""
import ctypes
import itertools
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import c_double, c_int64
from .bm25 import BM25Index
from .d2v import Doc2VecInference
from .index import Similarity

BM25_WEIGHT: float = 0.5               # webui.py:51
DOC2VEC_WEIGHT: float = 0.5            # webui.py:52
ORIGINAL_SCORE_WEIGHT: float = 0.7     # webui.py:55
RERANKED_SCORE_WEIGHT: float = 0.3     # webui.py:56
DIFF_FILTER_THRESH = 1e-6              # webui.py:58
REQUIRE_TAG_MAGIC_NUMBER = 1000        # webui.py:60
TOPK_MAX = 1024                        # hipts_topk limit
BATCH_MAX = 256                        # queries per device pass of find_similar_documents_batch: what hipts_search is tuned for


def filter_searched_result(ranked: List[Tuple[int, float]]) -> List[Tuple[int, float]]:
    """The result filter of webui.py:63-80 on a list ranked by descending score: the list ends at the SECOND place where two neighbours
    are closer than 1e-6 without being equal (at the first if there is only one), entries with a non-positive score are dropped, and
    the scores are divided by the largest one.  Pinned by tests/golden/g5_filter.json (vectors produced by the reference's function)."""
    vals = np.fromiter((score for _, score in ranked), dtype=np.float64, count=len(ranked))
    gaps = vals[:-1] - vals[1:]
    close = np.flatnonzero((gaps != 0) & (gaps < DIFF_FILTER_THRESH))      # equal neighbours (gap 0) do not count; NaN gaps neither
    cut = len(ranked) if close.size == 0 else int(close[min(1, close.size - 1)])
    top = float(vals.max())
    return [(doc, score / top) for doc, score in ranked[:cut] if score > 0]


def _split_weight(tag: str):
    sp = tag.split(":")
    if len(sp) >= 2 and (sp[-1].startswith("+") or sp[-1].startswith("-") or sp[-1].isdigit()):
        return ":".join(sp[:-1]), sp[-1]
    return ":".join(sp), None


def parse_related_query(query: str, token2id: Dict[str, int]) -> Tuple[List[int], List[int]]:
    """(include ids, exclude ids) of a related-tags query, in the grammar of the search box (_split_weight): a weight that starts with
    '-' excludes its tag, every other term is included, the weight's value is ignored.  Tags are looked up as typed, like
    parse_bm25_query (no parenthesis escaping); an unknown tag raises KeyError; ids are kept once, in order.  A query without any term
    is the empty query, which matches every document."""
    include: List[int] = []
    exclude: List[int] = []
    for term in query.split(" ") if query.strip() else []:
        name, w = _split_weight(term)
        side = exclude if w is not None and w.startswith("-") else include
        t = token2id[name]
        if t not in side:
            side.append(t)
    return include, exclude


class SearchEngine:
    def __init__(self, model: Doc2VecInference, index: Similarity, token2id: Dict[str, int], bm25: BM25Index,
                 image_files_name_tags_arr: Sequence[str], search_mode: str = "normal", compat_rerank: bool = False):
        self.model, self.index, self.token2id, self.bm25 = model, index, token2id, bm25
        self.image_files_name_tags_arr = list(image_files_name_tags_arr)
        self.search_mode = search_mode
        self.compat_rerank = compat_rerank
        self.cindex = None                     # cfeatures.CharacterFeatureIndex for 'character oriented' mode
        self.crerank = None                    # cfeatures.DeviceReranker once enable_device_crerank() was called (default: the host loop)
        self.stats = {"queries": 0, "full_rank_fallbacks": 0, "rank_continuations": 0,       # full_rank_fallbacks: always 0 since round 3
                      "batch_single_reruns": 0}
        self._search_fn = _lib.load().hipts_search
        self._w_bm25, self._w_sim = c_double(BM25_WEIGHT), c_double(DOC2VEC_WEIGHT)
        # webui.py:623-646: path -> {tag: True} and path -> doc id, built from the same index file
        self.file_tag_index_dict = {l.split(",")[0]: {t: True for t in l.split(",")[1:]} for l in self.image_files_name_tags_arr}
        self.filepath_docid_dict = {l.split(",")[0]: i for i, l in enumerate(self.image_files_name_tags_arr)}

    # ---- webui.py:82-117 ------------------------------------------------------------------------
    def normalize_and_apply_weight_doc2vec(self, new_doc: str) -> np.ndarray:
        tag_and_weight, all_weight = self._parse_doc2vec_query(new_doc)
        vecs = self.model.infer_vectors([[t] for t, _ in tag_and_weight])            # :106, batched
        return self._weighted_query_vector(tag_and_weight, all_weight, vecs)

    @staticmethod
    def _parse_doc2vec_query(new_doc: str) -> Tuple[List[Tuple[str, int]], int]:
        tag_and_weight: List[Tuple[str, int]] = []
        all_weight = 0
        for tag in new_doc.split(" "):
            name, w = _split_weight(tag)
            name = name.replace("\\(", "(").replace("\\)", ")").replace("(", "\\(").replace(")", "\\)")   # :92-98
            wi = int(w) if w is not None else 1
            tag_and_weight.append((name, wi))
            all_weight += wi
        if all_weight == 0:
            all_weight = 1
        return tag_and_weight, all_weight

    def _weighted_query_vector(self, tag_and_weight: List[Tuple[str, int]], all_weight: int, vecs) -> np.ndarray:
        """webui.py:104-117 on the inferred vectors of the query's tags (one per entry of tag_and_weight, in order)."""
        got = np.zeros(self.model.vector_size)
        for (tag, weight), v in zip(tag_and_weight, vecs):
            v = v / np.linalg.norm(v)                                                # :107
            got += weight * v                                                        # :108
        got = got / all_weight
        norm = np.linalg.norm(got)
        if math.isinf(norm) or norm == 0:
            norm = 1.0
        return got / norm

    # ---- webui.py:354-371 -----------------------------------------------------------------------
    def parse_bm25_query(self, new_doc: str):
        qw: Dict[int, float] = {}
        required: List[str] = []
        exclude: List[str] = []
        for term in new_doc.split(" "):
            name, w = _split_weight(term)
            if w is not None:
                if w.startswith("+"):
                    qw[self.token2id[name]] = REQUIRE_TAG_MAGIC_NUMBER + int(w)      # KeyError like :364
                    required.append(name)
                else:
                    qw[self.token2id[name]] = int(w)
                    exclude.append(name)
            else:
                qw[self.token2id[name]] = 1
        return qw, required, exclude

    # ---- related tags (no counterpart in the reference: its README sends the user to the tag file with grep) -------------------
    def related_tags(self, query: str, topn: int = 20, measure: str = "jaccard", min_count: int = 1) -> List[Tuple[str, float, int]]:
        """The tags that co-occur most with the documents `query` matches: (tag, score, count), best first.  `query` is parsed by
        parse_related_query; counting, scoring and ranking are BM25Index.related."""
        include, exclude = parse_related_query(query, self.token2id)
        ids, scores, counts, _ = self.bm25.related([(include, exclude)], topn, measure, min_count)
        id2token = self._id2token()
        return [(id2token[int(t)], float(s), int(c)) for t, s, c in zip(ids[0], scores[0], counts[0]) if t >= 0]

    def related_tags_table(self, k: int, measure: str = "jaccard", min_count: int = 1) -> Tuple[np.ndarray, np.ndarray]:
        """related_tags for every dictionary term at once: row t answers the one-tag query ([t], []).  ids int32 [V, k] and scores
        float64 [V, k], rows padded with (-1, -inf).  One call; the library takes the queries in passes of 256."""
        ids, scores, _, _ = self.bm25.related([((t,), ()) for t in range(self.bm25.vocab)], k, measure, min_count)
        return ids, scores

    def _id2token(self) -> Dict[int, str]:
        if getattr(self, "_id2token_map", None) is None or len(self._id2token_map) != len(self.token2id):
            self._id2token_map = {i: t for t, i in self.token2id.items()}
        return self._id2token_map

    # ---- device scoring -------------------------------------------------------------------------
    def score_topk(self, query_weights: Sequence[Dict[int, float]], query_vectors: np.ndarray, k: int,
                   final_out=None) -> Tuple[np.ndarray, np.ndarray]:
        """Fused webui.py:352-383 for a batch: returns (ids int32 [nq,k], scores float64 [nq,k]) in
        rank order; `final_out` (device float64 tensor [nq, D]) receives all combined scores."""
        nq = len(query_weights)
        if nq == 1 and final_out is None:                       # the reference's usage (webui.py:586): keep the host side short
            q = query_weights[0]
            n = len(q)
            qt_a = np.fromiter(q.keys(), dtype=np.int32, count=n) if n else np.zeros(1, np.int32)
            qw_a = np.fromiter(q.values(), dtype=np.float64, count=n) if n else np.zeros(1, np.float64)
            qp = np.array((0, n), dtype=np.int32)
            qv = np.ascontiguousarray(query_vectors, dtype=np.float32).reshape(1, -1)
            ids = np.empty((1, k), dtype=np.int32)
            vals = np.empty((1, k), dtype=np.float64)
            _lib.check(self._search_fn(self.bm25._h, self.index._h, qt_a.ctypes.data, qw_a.ctypes.data, qp.ctypes.data, qv.ctypes.data, 1,
                                       self._w_bm25, self._w_sim, k, ids.ctypes.data, vals.ctypes.data, None, _lib.current_stream_ptr()))
            return ids, vals
        # the CSR of the batch without a Python-level loop over terms (that loop was ~1/5 of a 256-query call)
        qp = np.zeros(nq + 1, dtype=np.int32)
        np.cumsum(np.fromiter(map(len, query_weights), dtype=np.int32, count=nq), out=qp[1:])
        nt = int(qp[nq])
        if nt:
            qt_a = np.fromiter(itertools.chain.from_iterable(query_weights), dtype=np.int32, count=nt)                   # dict iteration = keys
            qw_a = np.fromiter(itertools.chain.from_iterable(map(dict.values, query_weights)), dtype=np.float64, count=nt)
        else:
            qt_a = np.zeros(1, dtype=np.int32)
            qw_a = np.zeros(1, dtype=np.float64)
        qv = np.ascontiguousarray(np.atleast_2d(query_vectors), dtype=np.float32)
        ids = np.empty((nq, k), dtype=np.int32)
        vals = np.empty((nq, k), dtype=np.float64)
        _lib.call("hipts_search", self.bm25._h, self.index._h, _lib.ptr(qt_a), _lib.ptr(qw_a), _lib.ptr(qp), _lib.ptr(qv), nq,
                  c_double(BM25_WEIGHT), c_double(DOC2VEC_WEIGHT), k, _lib.ptr(ids), _lib.ptr(vals),
                  _lib.ptr(final_out) if final_out is not None else None, _lib.current_stream_ptr())
        return ids, vals

    def submit_topk(self, query_weights: Sequence[Dict[int, float]], query_vectors: np.ndarray, k: int, slot: int = 0):
        """First half of score_topk for a host that serves a stream of batches: packs and launches the batch into `slot` (0 or 1) and returns
        a ticket without waiting; `collect_topk(ticket)` returns what score_topk would have.  With the two slots used alternately the host
        prepares batch i + 1 while the device runs batch i (hipts_search_submit / hipts_search_collect)."""
        nq = len(query_weights)
        qp = np.zeros(nq + 1, dtype=np.int32)
        np.cumsum(np.fromiter(map(len, query_weights), dtype=np.int32, count=nq), out=qp[1:])
        nt = int(qp[nq])
        if nt:
            qt_a = np.fromiter(itertools.chain.from_iterable(query_weights), dtype=np.int32, count=nt)
            qw_a = np.fromiter(itertools.chain.from_iterable(map(dict.values, query_weights)), dtype=np.float64, count=nt)
        else:
            qt_a = np.zeros(1, dtype=np.int32)
            qw_a = np.zeros(1, dtype=np.float64)
        qv = np.ascontiguousarray(np.atleast_2d(query_vectors), dtype=np.float32)
        _lib.call("hipts_search_submit", self.bm25._h, self.index._h, _lib.ptr(qt_a), _lib.ptr(qw_a), _lib.ptr(qp), _lib.ptr(qv), nq,
                  c_double(BM25_WEIGHT), c_double(DOC2VEC_WEIGHT), k, slot, _lib.current_stream_ptr())
        return (slot, nq, k)

    def collect_topk(self, ticket) -> Tuple[np.ndarray, np.ndarray]:
        slot, nq, k = ticket
        ids = np.empty((nq, k), dtype=np.int32)
        vals = np.empty((nq, k), dtype=np.float64)
        _lib.call("hipts_search_collect", self.bm25._h, slot, _lib.ptr(ids), _lib.ptr(vals))
        return ids, vals

    # ---- webui.py:345-390 -----------------------------------------------------------------------
    def find_similar_documents(self, new_doc: str, topn: int = 50) -> List[Tuple[int, float]]:
        self.stats["queries"] += 1
        return self._find_one(new_doc, topn)

    def _find_one(self, new_doc: str, topn: int) -> List[Tuple[int, float]]:
        import torch
        vec = self.normalize_and_apply_weight_doc2vec(new_doc)                        # :349
        qw, required, exclude = self.parse_bm25_query(new_doc)                        # :354-371
        D = len(self.index)
        final_dev = torch.empty((1, D), dtype=torch.float64, device="cuda:%d" % self.index.device)
        k = min(TOPK_MAX, D)
        ids, vals = self.score_topk([qw], vec[None, :], k, final_out=final_dev)       # :352,374-383
        if self.search_mode == "character oriented":                                  # :386-388
            return self._cfeatures_rerank(ids[0], vals[0], topn, required, exclude)
        return self._doc2vec_rerank(final_dev, ids[0], vals[0], topn)                 # :390

    def find_similar_documents_batch(self, queries: Sequence[str], topn: int = 50) -> List[List[Tuple[int, float]]]:
        """find_similar_documents for a batch of queries as a front end accumulates them: per query the same list, ids and float bits.
        Every device stage runs once per chunk of BATCH_MAX queries (first-stage search, one inference of the distinct top-ten
        documents, second index pass, combine, ranking, hipts_rerank_finish); the query vectors and the ten-document rerank queries
        are built on the host with the single path's own arithmetic (numpy's reduction order and BLAS are part of those bits).
        A query whose result the ranks past TOPK_MAX decide (status 1 of hipts_rerank_finish) is answered by the one-query path and
        counted in stats["batch_single_reruns"]."""
        queries = list(queries)
        if not queries or topn < 1 or len(self.index) <= 10 or self.search_mode == "character oriented":
            return [self.find_similar_documents(q, topn) for q in queries]
        parsed = [(self._parse_doc2vec_query(q), self.parse_bm25_query(q)[0]) for q in queries]       # KeyError before any launch
        out: List[List[Tuple[int, float]]] = []
        for c0 in range(0, len(queries), BATCH_MAX):
            out += self._find_chunk(queries[c0:c0 + BATCH_MAX], parsed[c0:c0 + BATCH_MAX], topn)
        return out

    def _find_chunk(self, queries: List[str], parsed, topn: int) -> List[List[Tuple[int, float]]]:
        import torch
        nq, D = len(queries), len(self.index)
        self.stats["queries"] += nq
        # 1. query vectors: the distinct tags of the chunk in one inference (webui.py:106)
        tags = list(dict.fromkeys(t for (tw, _), _ in parsed for t, _ in tw))
        tag_vec = dict(zip(tags, self.model.infer_vectors([[t] for t in tags])))
        qvecs = np.stack([self._weighted_query_vector(tw, allw, [tag_vec[t] for t, _ in tw]) for (tw, allw), _ in parsed])
        # 2. first stage (webui.py:352,374-383)
        k = min(TOPK_MAX, D)
        final_dev = torch.empty((nq, D), dtype=torch.float64, device="cuda:%d" % self.index.device)
        ids, vals = self.score_topk([qw for _, qw in parsed], qvecs, k, final_out=final_dev)
        # 3. rerank queries: the distinct top-ten documents in one inference (webui.py:198-203)
        top10 = np.ascontiguousarray(ids[:, :10])
        docs = list(dict.fromkeys(top10.ravel().tolist()))
        doc_vec = dict(zip(docs, self.model.infer_vectors([self._doc_tags(d) for d in docs])))
        rq = np.stack([self._rerank_query_of(np.stack([doc_vec[d] for d in top10[q].tolist()]), [float(v) for v in vals[q, :10]])
                       for q in range(nq)]).astype(np.float32)
        lists, status = self._rerank_finish_batch(final_dev, rq, top10, topn)
        # 5. the ranks past TOPK_MAX decide: the one-query path continues the ranking
        for q in np.flatnonzero(status).tolist():
            self.stats["batch_single_reruns"] += 1
            lists[q] = self._find_one(queries[q], topn)
        return lists

    def _rerank_finish_batch(self, final_dev, rerank_queries: np.ndarray, top10: np.ndarray, topn: int):
        """Stage 4 of the batch: second index pass (webui.py:205), 0.7 / 0.3 combine (:208, written over final_dev), ranking and the
        finishing kernel.  Returns (lists, status int32 [nq]); lists[q] is the result where status[q] == 0."""
        import torch
        nq, D = final_dev.shape
        dev = final_dev.device
        rs_dev = torch.empty((nq, D), dtype=torch.float32, device=dev)
        self.index.query(rerank_queries, out=rs_dev)
        _lib.call("hipts_combine", _lib.ptr(final_dev), _lib.ptr(rs_dev), nq, c_int64(D), c_double(ORIGINAL_SCORE_WEIGHT),
                  c_double(RERANKED_SCORE_WEIGHT), 0, 0, _lib.ptr(final_dev), self.index.device, _lib.current_stream_ptr())
        k = min(TOPK_MAX, D)
        rids_dev = torch.empty((nq, k), dtype=torch.int32, device=dev)
        rvals_dev = torch.empty((nq, k), dtype=torch.float64, device=dev)
        _lib.call("hipts_topk", _lib.ptr(final_dev), nq, c_int64(D), k, _lib.ptr(rids_dev), _lib.ptr(rvals_dev), _lib.DEVICE, self.index.device,
                  _lib.current_stream_ptr())
        cap = min(topn, 10 + k)
        docs = np.empty((nq, cap), dtype=np.int32)
        scores = np.empty((nq, cap), dtype=np.float64)
        counts = np.empty(nq, dtype=np.int32)
        status = np.empty(nq, dtype=np.int32)
        _lib.call("hipts_rerank_finish", _lib.ptr(rids_dev), _lib.ptr(rvals_dev), nq, k, c_int64(D), _lib.ptr(np.ascontiguousarray(top10, dtype=np.int32)),
                  topn, _lib.ptr(docs), _lib.ptr(scores), _lib.ptr(counts), _lib.ptr(status), self.index.device, _lib.current_stream_ptr())
        lists = [list(zip(docs[q, :c].tolist(), scores[q, :c].tolist())) if st == 0 else None
                 for q, (c, st) in enumerate(zip(counts.tolist(), status.tolist()))]
        return lists, status

    # ---- webui.py:255-342 -----------------------------------------------------------------------
    def enable_device_crerank(self, enable: bool = True):
        """Character-oriented mode: threshold, tag filter and ranking (webui.py:311-335) on the device instead of the host loop of
        cfeatures_rerank -- the same list, bit for bit (cfeatures.DeviceReranker, built from this engine's lines and cindex)."""
        from .cfeatures import DeviceReranker
        if not enable:
            self.crerank = None
            return None
        if self.cindex is None:
            raise RuntimeError("enable_device_crerank needs engine.cindex (a cfeatures.CharacterFeatureIndex)")
        self.crerank = DeviceReranker(self.cindex, self.image_files_name_tags_arr, self.cindex.index.device, self.file_tag_index_dict,
                                      self.filepath_docid_dict)
        return self.crerank

    def _cfeatures_rerank(self, ids: np.ndarray, vals: np.ndarray, topn: int, required: List[str], exclude: List[str]):
        from .cfeatures import cfeatures_rerank, gen_image_ndarray
        if self.cindex is None:
            raise RuntimeError("character oriented mode needs engine.cindex (a cfeatures.CharacterFeatureIndex with an encoder)")
        D = len(self.index)
        if D <= 10:                                                                   # :336-342
            sims = filter_searched_result([(int(i), float(v)) for i, v in zip(ids[:D], vals[:D])])
            return sims[:min(topn, len(sims))]
        top10 = [(int(i), float(v)) for i, v in zip(ids[:10], vals[:10])]
        feats = []
        for doc_id, _ in top10:                                                       # :292-301
            path = self.image_files_name_tags_arr[doc_id].split(",")[0]
            arr = gen_image_ndarray(path, self.cindex.image_size)
            if arr is None:
                continue
            feats.append(self.cindex.ccip_batch_extract_features([arr])[0])
        if not feats:
            return top10
        if self.crerank is not None and self.crerank.cindex is self.cindex:
            return self.crerank.rerank(top10, feats, required, exclude, self.cindex.cosine_diff_threshold)
        return cfeatures_rerank(top10, feats, self.cindex, self.file_tag_index_dict, self.filepath_docid_dict, required, exclude,
                                self.cindex.cosine_diff_threshold)        # own parameter: gen_cfeatures.py:298-299's constant is the metric model's

    # ---- webui.py:189-253 -----------------------------------------------------------------------
    def _doc_tags(self, doc_id: int) -> List[str]:
        return self.image_files_name_tags_arr[doc_id].split(",")[1:]                  # :183 (doc_id+1-1)

    def _rerank_query(self, top10_ids: Sequence[int], top10_scores: Sequence[float]) -> np.ndarray:
        vecs = self.model.infer_vectors([self._doc_tags(int(d)) for d in top10_ids])  # :198-199
        return self._rerank_query_of(vecs, top10_scores)

    def _rerank_query_of(self, vecs: np.ndarray, top10_scores: Sequence[float]) -> np.ndarray:
        mean = np.average(vecs.astype(np.float64), axis=0, weights=np.asarray(top10_scores, dtype=np.float64))   # :200 (value column)
        if self.compat_rerank:
            # webui.py:200-203 divides the (index, value) pairs by the Frobenius norm of the whole
            # [300,2] array and rounds the indices: every index becomes 0, so the sparse query is
            # sum(values) * e0, which gensim then unit-normalises  [analysis; gensim unavailable].
            q = np.zeros_like(mean)
            s = mean.sum()
            q[0] = 1.0 if s >= 0 else -1.0
            return q
        n = np.linalg.norm(mean)
        return mean / n if n > 0 else mean

    def _ranked_prefix(self, scores_dev, k: int) -> Tuple[np.ndarray, np.ndarray]:
        ids = np.empty((1, k), dtype=np.int32)
        vals = np.empty((1, k), dtype=np.float64)
        _lib.call("hipts_topk", _lib.ptr(scores_dev), 1, c_int64(scores_dev.shape[-1]), k, _lib.ptr(ids), _lib.ptr(vals),
                  _lib.HOST, self.index.device, _lib.current_stream_ptr())
        return ids[0], vals[0]

    def _doc2vec_rerank(self, final_dev, ids: np.ndarray, vals: np.ndarray, topn: int) -> List[Tuple[int, float]]:
        import torch
        D = final_dev.shape[-1]
        if D <= 10:                                                                   # :247-253
            sims = filter_searched_result([(int(i), float(v)) for i, v in zip(ids[:D], vals[:D])])
            return sims[:min(topn, len(sims))]
        top10_ids = [int(i) for i in ids[:10]]
        top10_scores = [float(v) for v in vals[:10]]
        q = self._rerank_query(top10_ids, top10_scores).astype(np.float32)
        rs_dev = torch.empty((1, D), dtype=torch.float32, device=final_dev.device)
        self.index.query(q, out=rs_dev)                                               # :205
        rf_dev = torch.empty_like(final_dev)
        _lib.call("hipts_combine", _lib.ptr(final_dev), _lib.ptr(rs_dev), 1, c_int64(D), c_double(ORIGINAL_SCORE_WEIGHT),
                  c_double(RERANKED_SCORE_WEIGHT), 0, 0, _lib.ptr(rf_dev), self.index.device, _lib.current_stream_ptr())   # :208
        k = min(TOPK_MAX, D)
        rids, rvals = self._ranked_prefix(rf_dev, k)
        last_id, last_val = int(rids[-1]), float(rvals[-1])                          # the last ranked entry as the device holds it
        mx = rvals[0]
        if mx > 0:
            rvals = rvals / mx                                                        # :210-211
        top10_set = set(top10_ids)
        final = [(d, 1.0) for d in top10_ids]                                         # :219-222
        final += [(int(i), float(v)) for i, v in zip(rids, rvals) if int(i) not in top10_set]   # :217,225-237
        # The gap filter (webui.py:63-80) cuts at the SECOND near-tie of the whole ranked list, wherever that is.  Almost always it lies
        # inside the first 1024 ranks; while it does not, the ranking is continued on the device 1024 entries at a time
        # (hipts_topk_after) -- until two cut points are in hand or only -inf scores remain (they produce no cut point: inf - inf is
        # nan).  Round 2 ranked all D scores on the host in that case (27 ms, one query in 20 on the bench corpus).
        n_ranked = k
        while n_ranked < D and last_val > -math.inf and not self._two_cut_points(final):
            self.stats["rank_continuations"] = self.stats.get("rank_continuations", 0) + 1
            kk = min(TOPK_MAX, D - n_ranked)
            mids = np.empty((1, kk), dtype=np.int32)
            mvals = np.empty((1, kk), dtype=np.float64)
            _lib.call("hipts_topk_after", _lib.ptr(rf_dev), c_int64(D), kk, c_double(last_val), c_int64(last_id), _lib.ptr(mids), _lib.ptr(mvals),
                      self.index.device, _lib.current_stream_ptr())
            last_id, last_val = int(mids[0, -1]), float(mvals[0, -1])
            more = mvals[0] / mx if mx > 0 else mvals[0]
            final += [(int(i), float(v)) for i, v in zip(mids[0], more) if int(i) not in top10_set]
            n_ranked += kk
        final = filter_searched_result(final)                                         # :240
        return final[:min(topn, len(final))]

    @staticmethod
    def _two_cut_points(ranked: List[Tuple[int, float]]) -> bool:
        s = np.array([v for _, v in ranked])
        d = s[:-1] - s[1:]
        d = np.where(d == 0, np.inf, d)
        return int((d < DIFF_FILTER_THRESH).sum()) >= 2


_engine: Optional[SearchEngine] = None


def set_engine(engine: SearchEngine):
    global _engine
    _engine = engine


def find_similar_documents(new_doc: str, topn: int = 50) -> List[Tuple[int, float]]:
    """webui.py:345 -- module-level entry point with the reference's signature."""
    if _engine is None:
        raise RuntimeError("no SearchEngine installed: call set_engine(load_engine()) first (webui.py:585 load_model)")
    return _engine.find_similar_documents(new_doc, topn)


def find_similar_documents_batch(queries: Sequence[str], topn: int = 50) -> List[List[Tuple[int, float]]]:
    """find_similar_documents for a batch of queries on the installed engine."""
    if _engine is None:
        raise RuntimeError("no SearchEngine installed: call set_engine(load_engine()) first (webui.py:585 load_model)")
    return _engine.find_similar_documents_batch(queries, topn)


def related_tags(query: str, topn: int = 20, measure: str = "jaccard", min_count: int = 1) -> List[Tuple[str, float, int]]:
    """SearchEngine.related_tags on the installed engine."""
    if _engine is None:
        raise RuntimeError("no SearchEngine installed: call set_engine(load_engine()) first (webui.py:585 load_model)")
    return _engine.related_tags(query, topn, measure, min_count)


def load_engine(device: int = 0, d2v_model: str = "doc2vec_model", compat_rerank: bool = False) -> SearchEngine:
    """webui.py:649-689 load_model(): everything the query function needs, from the files
    genmodel.py writes into the current directory."""
    import pickle
    from .bm25 import load_bm25_index
    tag_file_path = 'tags-wd-tagger_doc2vec_idx.csv'
    with open(tag_file_path, 'r', encoding='utf-8') as f:
        lines = [line.strip() for line in f.readlines()]
    model = Doc2VecInference.load(d2v_model, device)
    index = Similarity.load("doc2vec_index", device)
    dictionary = pickle.load(open("doc2vec_dictionary", "rb"))
    bm25 = load_bm25_index(device)
    return SearchEngine(model, index, dictionary.token2id, bm25, lines, compat_rerank=compat_rerank)
