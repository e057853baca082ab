"""Build the thumbnail cache of a collection: one small JPEG per image, encoded on the device.

Every image goes through the tagger's own input pipeline (composite over white, centred pad to a square, bicubic resize to 448), so a
thumbnail shows exactly what the tagger sees and find_duplicates.py hashes, and every input mode gives the same bytes for the same
picture.  The 448 square is resized to --size (Pillow's bicubic) and encoded (hiptagsearch.thumbs.ThumbnailWriter: the file
PIL.Image.save(..., "JPEG", quality=Q) would write).  Files go to OUT/<two hex digits>/<sha1 of the path>.jpg; OUT/thumbnails.csv lists
`path,thumbnail` in input order.  A file that cannot be decoded is left out, as the tagger leaves it out.  query.py --contact-sheet reads
the cache.

    python make_thumbnails.py (--dir D | --shards DIR) --out thumbs [--size 256] [--quality 85] [--workers 8] [--gpu-resize] [--gpu-jpeg]
                              [--gpu-png] [--batch 64] [--device 0]
"""
import argparse

from hiptagsearch import pipeline
from hiptagsearch.thumbs import ThumbnailWriter

SIZE = 448                   # the tagger's input


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--dir", help="the image files under this directory (the files tagging.py would tag)")
    src.add_argument("--shards", help="the pre-decoded shards in this directory (written by tagging.py --write-shards)")
    ap.add_argument("--out", required=True, help="the cache directory")
    ap.add_argument("--size", type=int, default=256, help="thumbnail edge: a multiple of 16 in 64..512 (default 256)")
    ap.add_argument("--quality", type=int, default=85, help="JPEG quality, 1..100 (default 85)")
    ap.add_argument("--workers", type=int, default=8, help="decode processes (default 8)")
    ap.add_argument("--gpu-resize", action="store_true", help="pad and resize on the device (as tagging.py --gpu-resize)")
    ap.add_argument("--gpu-jpeg", action="store_true", help="the per-block half of the JPEG decode on the device (implies --gpu-resize)")
    ap.add_argument("--gpu-png", action="store_true", help="unfilter and composite PNG files on the device (implies --gpu-resize)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--threads", type=int, default=8, help="host threads of the Huffman coder (default 8, at most 16)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--input-size", type=int, default=SIZE,
                    help="--dir: the model input the thumbnails are made from (default 448, the wd taggers'; 64 for tagging.py --model vit-tiny)")
    args = ap.parse_args(argv)
    if args.size % 16 != 0 or not 64 <= args.size <= 512:
        ap.error("--size must be a multiple of 16 in 64..512")
    if not 1 <= args.quality <= 100:
        ap.error("--quality must be in 1..100")

    with ThumbnailWriter(args.out, args.size, args.quality, args.device, args.threads) as writer:
        if args.shards:
            for paths, images in pipeline.iter_shards(args.shards, args.batch):
                writer.add(paths, images)
        else:
            from hiptagsearch.tagger import Predictor
            files = Predictor.list_files_recursive(None, args.dir)         # (uses nothing of a Predictor: no model is loaded here)
            print("%d files found" % len(files))
            gpu = args.gpu_resize or args.gpu_jpeg or args.gpu_png
            with pipeline.DecodePool(args.workers, args.input_size, args.batch, pipeline.TAGGER, device_resize=gpu, device=args.device,
                                     device_jpeg=args.gpu_jpeg, device_png=args.gpu_png) as pool:
                for paths, images in pool.batches(files):
                    writer.add(paths, images)
    print("%d thumbnails -> %s" % (writer.count, args.out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
