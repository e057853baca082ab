#!/usr/bin/env python3
"""python query.py "1girl blue_eyes:+2 hat:-1" [--topn 50]     -- the webui.py query function
(find_similar_documents, webui.py:345) without the Streamlit UI.
python query.py --batch-file queries.txt [--topn 50]           -- one query per line, answered as one batch
(find_similar_documents_batch); per query a "# query" header line, then the same lines."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("query", nargs="?")
    ap.add_argument("--batch-file", help="file with one query per line (empty lines are skipped); replaces the positional query")
    ap.add_argument("--topn", type=int, default=50)
    ap.add_argument("--compat-rerank", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if (a.query is None) == (a.batch_file is None):
        ap.error("give either a query or --batch-file")
    from hiptagsearch import search
    eng = search.load_engine(a.device, compat_rerank=a.compat_rerank)
    search.set_engine(eng)
    if a.batch_file is not None:
        with open(a.batch_file, encoding="utf-8") as f:
            queries = [line.strip() for line in f if line.strip()]
        results = search.find_similar_documents_batch(queries, a.topn)
    else:
        queries, results = None, [search.find_similar_documents(a.query, a.topn)]
    for i, res in enumerate(results):
        if queries is not None:
            print("# %s" % queries[i])
        for doc_id, score in res:
            print("%.6f\t%s" % (score, eng.image_files_name_tags_arr[doc_id].split(",")[0]))


if __name__ == "__main__":
    main(sys.argv[1:])
