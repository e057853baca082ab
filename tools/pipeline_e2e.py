#!/usr/bin/env python3
"""Development aid (needs the GPU): end-to-end images/s of the tagging loop over a directory of images, by input pipeline --
the reference's 8 decode threads, the same with the resize on the device, N decode processes, N decode-only processes + device resize,
N entropy-decode-only processes + the rest of the JPEG decode and the resize on the device (hybrid decode, round 4), N inflate-only
processes + the rest of the PNG decode and the resize on the device (hybrid PNG decode).
usage: pipeline_e2e.py [n_images] [workers[,workers]] [--format jpeg|png|png-rgba|mixed]
  --format jpeg      (default) the rows above but the PNG one, over JPEGs
  --format png       RGB PNGs:  --gpu-resize against --gpu-resize --gpu-png
  --format png-rgba  RGBA PNGs: the same two rows
  --format mixed     JPEG, RGB PNG and RGBA PNG in turn: --gpu-resize, + --gpu-png, + --gpu-jpeg, + both
The tag file must be the same in every row."""
import argparse, concurrent.futures, io, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "anime-illust-image-searcher_amd")
ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=2048)
ap.add_argument("workers", nargs="?", default=str(os.cpu_count() or 8), help="worker processes; a,b: every row once per count, over the same files")
ap.add_argument("--format", choices=["jpeg", "png", "png-rgba", "mixed"], default="jpeg")
ARGS = ap.parse_args()
N, FORMAT = ARGS.n, ARGS.format
WORKERS = [int(v) for v in ARGS.workers.split(",")]
W = max(WORKERS)
import numpy as np
from PIL import Image


def kind_of(i):
    return {"jpeg": "jpeg", "png": "png", "png-rgba": "png-rgba"}.get(FORMAT) or ("jpeg", "png", "png-rgba")[i % 3]


def make(args):
    d, i = args
    rng = np.random.default_rng(i)
    kind = kind_of(i)
    c = 4 if kind == "png-rgba" else 3
    small = rng.integers(0, 256, (24, 32, c), dtype=np.uint8)
    big = np.stack([np.asarray(Image.fromarray(small[:, :, k]).resize((1024, 768), Image.BICUBIC)) for k in range(c)], axis=2) if c == 4 else \
        np.asarray(Image.fromarray(small).resize((1024, 768), Image.BICUBIC))
    if kind == "jpeg":
        a = big.astype(np.int16) + rng.integers(-6, 7, (768, 1024, 3), dtype=np.int16)
        Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(os.path.join(d, "img%05d.jpg" % i), quality=90,
                                                                   progressive=bool(int(os.environ.get("E2E_PROGRESSIVE", "0"))))
    else:       # a gradient with +- 8 noise: Pillow's adaptive filter mixes the row filter types, inflate has real work
        a = big.astype(np.int16) + rng.integers(-8, 9, (768, 1024, c), dtype=np.int16)
        Image.fromarray(np.clip(a, 0, 255).astype(np.uint8), "RGBA" if c == 4 else "RGB").save(os.path.join(d, "img%05d.png" % i))


def rows(W):
    w = ["--workers", str(W)]
    if FORMAT == "jpeg":
        return [("8 threads, host resize (the reference's structure)", []), ("8 threads, device resize", ["--gpu-resize"]),
                ("%d processes, host resize" % W, w), ("%d decode-only processes, device resize" % W, w + ["--gpu-resize"]),
                ("%d entropy-decode processes, device IDCT + resize" % W, w + ["--gpu-resize", "--gpu-jpeg"])]
    out = [("%d decode-only processes, device resize" % W, w + ["--gpu-resize"]),
           ("%d inflate-only processes, device unfilter + resize" % W, w + ["--gpu-resize", "--gpu-png"])]
    if FORMAT == "mixed":
        out += [("%d processes, device IDCT + resize (JPEG only)" % W, w + ["--gpu-resize", "--gpu-jpeg"]),
                ("%d processes, device IDCT + unfilter + resize" % W, w + ["--gpu-resize", "--gpu-jpeg", "--gpu-png"])]
    return out


with tempfile.TemporaryDirectory() as tmp:
    d = os.path.join(tmp, "imgs")
    os.makedirs(d)
    import shutil
    per_file = {"jpeg": 0.4e6, "png": 1.6e6, "png-rgba": 2.1e6, "mixed": 1.4e6}[FORMAT]
    free = shutil.disk_usage(tmp).free
    if N * per_file > 0.6 * free:           # a PNG corpus is several times the JPEG one: never fill the disk
        fit = int(0.6 * free / per_file) // 64 * 64
        print("only %.1f GB free under %s: %d files instead of %d" % (free / 1e9, tmp, fit, N), flush=True)
        N = fit
    t0 = time.perf_counter()
    with concurrent.futures.ProcessPoolExecutor(W) as ex:
        list(ex.map(make, [(d, i) for i in range(N)], chunksize=16))
    what = {"jpeg": "%sJPEGs 1024x768 q90" % ("progressive " if int(os.environ.get("E2E_PROGRESSIVE", "0")) else ""), "png": "RGB PNGs 1024x768",
            "png-rgba": "RGBA PNGs 1024x768", "mixed": "JPEGs / RGB PNGs / RGBA PNGs 1024x768"}[FORMAT]
    size = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
    print("%d %s (%.2f MB each) written in %.1f s (%d processes)" % (N, what, size / N / 1e6, time.perf_counter() - t0, W), flush=True)
    ref = None
    only = os.environ.get("E2E_MODES")          # e.g. "3,4": run only those rows (0-based)
    repeat = int(os.environ.get("E2E_REPEAT", "1"))       # e.g. 2: the rows in the order A B A B
    for mode_i, (name, extra) in [(i, r) for nw in WORKERS for _ in range(repeat) for i, r in enumerate(rows(nw))]:
        if only and str(mode_i) not in only.split(","):
            continue
        out = os.path.join(tmp, "tags-wd-tagger.txt")
        if os.path.exists(out):
            os.remove(out)
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, os.path.join(PKG, "tagging.py"), "--dir", "imgs", "--batch", "64"] + extra, cwd=tmp, capture_output=True, text=True)
        dt = time.perf_counter() - t0
        if r.returncode != 0:       # nothing more is started on the GPU after a run that failed
            print(name, "FAILED (exit %d)" % r.returncode, r.stderr[-1500:], flush=True)
            sys.exit(1)
        # the CLI prints "<n> files processed / <t> seconds elapsed" from inside the loop: the last pair = loop time without model load
        lines = r.stdout.splitlines()
        el = [float(l.split()[0]) for l in lines if l.endswith("seconds elapsed")]
        cnt = [int(l.split()[0]) for l in lines if l.endswith("files processed")]
        for l in lines:
            if l.startswith("pipeline timing"):
                print("    " + l, flush=True)
        text = open(out, encoding="utf-8").read()
        same = ref is None or text == ref
        ref = ref or text
        # steady state: between the first and the last progress print (pool start-up, first-use allocations and the model's warm-up lie before the first)
        loop = ("%.0f images/s steady (images %d..%d in %.2f s), %.0f incl. start-up" % ((cnt[-1] - cnt[0]) / (el[-1] - el[0]), cnt[0], cnt[-1], el[-1] - el[0], cnt[-1] / el[-1])
                if len(el) >= 2 else "n/a")
        print("%-58s %s; whole process %.1f s; output identical: %s" % (name, loop, dt, same), flush=True)
