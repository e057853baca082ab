"""Group the character-feature index by character: which pictures show the same one?

Reads the latest `charactor-featues-idx*` revision and `charactor-featues-idx.csv` that gen_cfeatures.py leaves in the
current directory, clusters the features on the device (CharacterFeatureIndex.cluster: DBSCAN over
`1 - cosine < threshold`) and writes one `path,label` line per feature row, in index order; label -1 = in no group.

    python cluster_cfeatures.py [--threshold T] [--min-samples M] [--out charactor-clusters.csv] [--max-pairs P] [--device D]
"""
import argparse

import numpy as np

from hiptagsearch.cfeatures import CharacterFeatureIndex


def _no_encoder(_images):
    raise RuntimeError("cluster_cfeatures.py encodes no image")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--threshold", type=float, default=None, help="cut on 1 - cosine (default: the index's cosine_diff_threshold)")
    ap.add_argument("--min-samples", type=int, default=2, help="neighbours (itself included) that make a row a core row (default 2)")
    ap.add_argument("--out", default="charactor-clusters.csv")
    ap.add_argument("--max-pairs", type=int, default=0, help="refuse when more neighbour pairs lie under the threshold (0: by free device memory)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)

    cindex = CharacterFeatureIndex.load_latest(_no_encoder, args.device)
    labels = cindex.cluster(args.threshold, args.min_samples, args.max_pairs)
    with open(args.out, "w", encoding="utf-8") as f:
        for path, label in zip(cindex.paths, labels.tolist()):
            f.write("%s,%d\n" % (path, label))
    clusters = int(labels.max()) + 1 if len(labels) else 0
    noise = int(np.count_nonzero(labels < 0))
    print("%d clusters, %d clustered rows, %d noise rows -> %s" % (clusters, len(labels) - noise, noise, args.out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
