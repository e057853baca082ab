#!/usr/bin/env python3
"""python query.py "1girl blue_eyes:+2 hat:-1" [--topn 50]     -- the webui.py query function
(find_similar_documents, webui.py:345) without the Streamlit UI.
python query.py --batch-file queries.txt [--topn 50]           -- one query per line, answered as one batch
(find_similar_documents_batch); per query a "# query" header line, then the same lines.
python query.py --related "1girl hat:-1" [--topn 20] [--measure count|jaccard|lift] [--min-count N]
-- the tags that co-occur most with the documents that carry 1girl and not hat (SearchEngine.related_tags): score<TAB>count<TAB>tag lines.
Needs only doc2vec_dictionary and the BM25 pickles.
python query.py QUERY --contact-sheet FILE --thumbnails DIR [--columns 8]
-- also writes the ranked results as ONE JPEG, in result order, from the thumbnail cache DIR (make_thumbnails.py, tagging.py --thumbnails);
a result without a thumbnail leaves its cell white."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("query", nargs="?")
    ap.add_argument("--batch-file", help="file with one query per line (empty lines are skipped); replaces the positional query")
    ap.add_argument("--related", metavar="QUERY", help="list the tags related to this query instead of searching")
    ap.add_argument("--measure", choices=["count", "jaccard", "lift"], default="jaccard", help="--related: how co-occurrence is scored")
    ap.add_argument("--min-count", type=int, default=1, help="--related: drop tags that co-occur in fewer matching documents")
    ap.add_argument("--topn", type=int, default=None, help="default 50; 20 with --related")
    ap.add_argument("--compat-rerank", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--contact-sheet", metavar="FILE", help="write the results of the (single) query as one JPEG of thumbnails; needs --thumbnails")
    ap.add_argument("--thumbnails", metavar="DIR", help="the thumbnail cache (the directory that holds thumbnails.csv)")
    ap.add_argument("--columns", type=int, default=8, help="--contact-sheet: thumbnails per row (default 8)")
    a = ap.parse_args(argv)
    if a.contact_sheet is not None and (a.thumbnails is None or a.query is None or a.related is not None or a.columns < 1):
        ap.error("--contact-sheet needs a single query, --thumbnails DIR and --columns >= 1")
    if a.related is not None:
        if a.query is not None or a.batch_file is not None:
            ap.error("--related replaces the query and --batch-file")
        return related(a)
    if a.topn is None:
        a.topn = 50
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
    if a.contact_sheet is not None:
        write_contact_sheet([eng.image_files_name_tags_arr[doc_id].split(",")[0] for doc_id, _ in results[0]], a.thumbnails, a.contact_sheet,
                            a.columns, a.device)


def write_contact_sheet(paths, thumb_dir, out_file, columns=8, device=0):
    """the thumbnails of `paths`, in order, as one JPEG of quality 85; the cell size is the cache's (read from the first thumbnail found)"""
    import io
    from PIL import Image
    from hiptagsearch import thumbs
    index = thumbs.read_index(thumb_dir)
    found = [index.get(p) for p in paths]
    size, quality = 256, 85
    for f in found:
        if f and os.path.exists(f):
            with open(f, "rb") as fh:
                im = Image.open(io.BytesIO(fh.read()))
            size = im.size[0]
            break
    data = thumbs.contact_sheet(found, columns, size, quality, device)
    with open(out_file, "wb") as f:
        f.write(data)
    print("%d of %d results have a thumbnail -> %s" % (sum(1 for f in found if f and os.path.exists(f)), len(found), out_file))


def related(a):
    import pickle
    from hiptagsearch import search
    from hiptagsearch.bm25 import load_bm25_index
    token2id = pickle.load(open("doc2vec_dictionary", "rb")).token2id
    eng = search.SearchEngine(None, None, token2id, load_bm25_index(a.device), [])
    for tag, score, count in eng.related_tags(a.related, 20 if a.topn is None else a.topn, a.measure, a.min_count):
        print("%.6f\t%d\t%s" % (score, count, tag))


if __name__ == "__main__":
    main(sys.argv[1:])
