"""Find the files that hold the same picture: a re-save at another size, a JPEG of a PNG, a second download.

Every image goes through the tagger's own input pipeline (composite over white, centred pad to a square, bicubic resize to 448: the
hash sees exactly what the tagger sees), is hashed on the device (hiptagsearch.dedup.image_hashes: a 128-bit gradient hash) and the
hashes are grouped on the device (ImageHashIndex.groups: files whose hashes differ in at most --max-distance bits, chained).  Writes one
`path,label` line per file, in input order; label -1 = the file has no duplicate.  A file that cannot be decoded is left out, as the
tagger leaves it out.

    python find_duplicates.py (--dir D | --shards DIR | --hashes PREFIX) [--max-distance 10] [--min-set-bits 8]
                              [--workers 8] [--gpu-resize] [--gpu-jpeg] [--gpu-png] [--batch 64] [--save-hashes PREFIX]
                              [--out duplicates.csv] [--max-pairs 0] [--device 0]
"""
import argparse

import numpy as np

from hiptagsearch import pipeline
from hiptagsearch.dedup import ImageHashIndex, image_hashes, set_bits

SIZE = 448                   # the tagger's input


def _hash_batches(index: ImageHashIndex, batches, device: int) -> None:
    for paths, images in batches:
        index.add(paths, image_hashes(images, device))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--dir", help="hash the image files under this directory (the files tagging.py would tag)")
    src.add_argument("--shards", help="hash the pre-decoded shards in this directory (written by tagging.py --write-shards)")
    src.add_argument("--hashes", metavar="PREFIX", help="group a saved index (PREFIX.npy + PREFIX.csv); no image is touched")
    ap.add_argument("--max-distance", type=int, default=10, help="hashes that differ in at most this many of their 128 bits are duplicates (default 10)")
    ap.add_argument("--min-set-bits", type=int, default=8,
                    help="files whose hash has fewer set bits are flat pictures (an all-white page): left out, label -1 (default 8; 0: none)")
    ap.add_argument("--workers", type=int, default=8, help="decode processes (default 8)")
    ap.add_argument("--gpu-resize", action="store_true", help="pad and resize on the device (as tagging.py --gpu-resize)")
    ap.add_argument("--gpu-jpeg", action="store_true", help="the per-block half of the JPEG decode on the device (implies --gpu-resize)")
    ap.add_argument("--gpu-png", action="store_true", help="unfilter and composite PNG files on the device (implies --gpu-resize)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--save-hashes", metavar="PREFIX", default=None, help="also write the index: PREFIX.npy and PREFIX.csv")
    ap.add_argument("--out", default="duplicates.csv")
    ap.add_argument("--max-pairs", type=int, default=0, help="refuse when more pairs lie within the distance (0: by free device memory)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)

    if args.hashes:
        index = ImageHashIndex.load(args.hashes, args.device)
    else:
        index = ImageHashIndex(args.device)
        if args.shards:
            _hash_batches(index, pipeline.iter_shards(args.shards, args.batch), args.device)
        else:
            from hiptagsearch.tagger import Predictor
            files = Predictor.list_files_recursive(None, args.dir)         # (uses nothing of a Predictor: no model is loaded here)
            print("%d files found" % len(files))
            gpu = args.gpu_resize or args.gpu_jpeg or args.gpu_png
            with pipeline.DecodePool(args.workers, SIZE, args.batch, pipeline.TAGGER, device_resize=gpu, device=args.device,
                                     device_jpeg=args.gpu_jpeg, device_png=args.gpu_png) as pool:
                _hash_batches(index, pool.batches(files), args.device)
    if args.save_hashes:
        index.save(args.save_hashes)

    labels = index.groups(args.max_distance, args.min_set_bits, args.max_pairs)
    with open(args.out, "w", encoding="utf-8") as f:
        for path, label in zip(index.paths, labels.tolist()):
            f.write("%s,%d\n" % (path, label))
    groups = int(labels.max()) + 1 if len(labels) else 0
    flat = int(np.count_nonzero(set_bits(index.hashes) < args.min_set_bits))
    print("%d files, %d groups, %d files in groups, %d flat files -> %s" % (len(labels), groups, int(np.count_nonzero(labels >= 0)), flat, args.out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
