#!/usr/bin/env python3
"""Thumbnails at the sizes the project is measured at (hiptagsearch/thumbs.py; csrc/jpegenc.hip, csrc/jpeg_host.c).

  kernel     hipts_jpeg_encode_batch_u8 on a batch of 64 images at 256 x 256, quality 85, device memory in and out: HIP events around
             --calls calls per repetition, after warm-up.  Content: the bicubic reduction of noisy gradients (what a thumbnail of a
             picture looks like) -- the kernel's time does not depend on it.  Floor: 3 B read + 3 B written per pixel over the HBM rate.
  coder      the host coder (hipts_jpeg_entropy_encode through ctypes, as jpeg_encode drives it) over the slots of 1024 such thumbnails
             that sit in host memory: thumbnails/s at 1, 8 and 16 threads.  Its time does depend on the content.
  whole      ThumbnailWriter.add over 16 batches of 64 model-input images at 448 in device memory (resize to 256, encode, copy, code,
             write the files), 8 and 16 threads: thumbnails/s from a host clock around add() ... close().
  reference  what the device path is compared against, NOT the code under test: Image.fromarray(x).resize((256, 256), BICUBIC) and
             save(quality=85) into memory, on 1 and on 16 host processes of the same box.
  tagging    tagging.py --workers 16 --gpu-resize --gpu-jpeg over --files JPEG files of 1024 x 768 with and without --thumbnails, rows
             A B A B over the same files: a host clock around each child process (start-up and model set-up included), and the
             difference between the rows of THIS run.  The tag files must be equal.

Without --step the steps run one after the other, each as a child process of its own under its own time limit; the first one that
fails, faults or runs out of time ends the run.  Needs a GPU; there is no fallback."""
import argparse
import concurrent.futures
import io
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "anime-illust-image-searcher_amd")
sys.path.insert(0, ROOT)
sys.path.insert(0, PKG)
import numpy as np  # noqa: E402

B, SIZE, QUALITY, INPUT = 64, 256, 85, 448
STEPS = ("kernel", "coder", "whole", "reference", "tagging")
LIMITS = {"kernel": 120, "coder": 180, "whole": 180, "reference": 240, "tagging": 540}      # seconds per step


def stats(v):
    a = np.sort(np.asarray(v, dtype=np.float64))
    return {"median": float(np.median(a)), "min": float(a[0]), "max": float(a[-1]), "n": len(a)}


def picture(i, size):
    """uint8 [size, size, 3]: a smooth random field with a little noise, like a reduced photograph or drawing"""
    from PIL import Image
    rng = np.random.default_rng(i)
    small = rng.integers(0, 256, (max(2, size // 32), max(2, size // 32), 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(small).resize((size, size), Image.BICUBIC), dtype=np.int16) + rng.integers(-6, 7, (size, size, 3), dtype=np.int16)
    return np.clip(a, 0, 255).astype(np.uint8)


def pictures(n, size):
    base = np.stack([picture(i, size) for i in range(16)])
    return np.stack([np.roll(base[i % 16], 7 * (i // 16), axis=1) for i in range(n)])


def step_kernel(args, say):
    import ctypes
    import torch
    from hiptagsearch import _lib
    if not torch.cuda.is_available():
        raise SystemExit("thumbs_bench needs a GPU")
    images = torch.from_numpy(pictures(B, SIZE)).cuda()
    stride = int(_lib.load().hipts_jpeg_slot_bytes(SIZE, SIZE))
    slots = torch.empty((B, stride), dtype=torch.uint8, device="cuda")
    stream = _lib.current_stream_ptr()
    ms = []
    for it in range(args.warmup + args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            _lib.call("hipts_jpeg_encode_batch_u8", _lib.ptr(images), _lib.DEVICE, B, SIZE, SIZE, QUALITY, _lib.ptr(slots), _lib.DEVICE,
                      ctypes.c_int64(stride), 0, stream)
        e1.record()
        e1.synchronize()
        if it >= args.warmup:
            ms.append(e0.elapsed_time(e1) / args.calls)
    st = stats(ms)
    moved = B * SIZE * SIZE * 6
    say("kernel: %d images at %d x %d, quality %d, %d calls per repetition, %d repetitions after %d warm-up" % (B, SIZE, SIZE, QUALITY, args.calls,
                                                                                                            args.repeats, args.warmup))
    say("  per batch  median %.4f ms  (min %.4f, max %.4f, n %d)  = %.2f TB/s of the %.1f MB read + written; the forward it runs next to "
        "takes 11.8 ms per batch" % (st["median"], st["min"], st["max"], st["n"], moved / st["median"] / 1e9, moved / 1e6))
    say(json.dumps({"thumbs_bench_kernel": {"batch": B, "size": SIZE, "per_batch_ms": st}}))


def step_coder(args, say):
    import torch
    from hiptagsearch import thumbs
    if not torch.cuda.is_available():
        raise SystemExit("thumbs_bench needs a GPU")
    n = 1024
    launched = [thumbs._launch(torch.from_numpy(pictures(n, SIZE)[s:s + B]).cuda(), QUALITY, 0) for s in range(0, n, B)]
    torch.cuda.synchronize()
    say("coder: the slots of %d thumbnails of %d x %d in pinned host memory, %d repetitions after 1 warm-up" % (n, SIZE, SIZE, args.repeats))
    res = {}
    for threads in (1, 8, 16):
        rate, size = [], 0
        with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as ex:
            for it in range(1 + args.repeats):
                t0 = time.perf_counter()
                files = [f for L in launched for f in thumbs._code(L, ex)]
                dt = time.perf_counter() - t0
                size = sum(len(f) for f in files) / len(files)
                if it >= 1:
                    rate.append(n / dt)
        st = stats(rate)
        res[str(threads)] = st
        say("  %2d threads  median %8.0f thumbnails/s  (min %.0f, max %.0f, n %d); %.1f kB per file" % (threads, st["median"], st["min"], st["max"],
                                                                                                     st["n"], size / 1e3))
    say(json.dumps({"thumbs_bench_coder": {"size": SIZE, "thumbnails_per_s_by_threads": res}}))


def step_whole(args, say):
    import torch
    from hiptagsearch.thumbs import ThumbnailWriter
    if not torch.cuda.is_available():
        raise SystemExit("thumbs_bench needs a GPU")
    batches = 16
    images = torch.from_numpy(pictures(B, INPUT)).cuda()
    paths = [["b%02d/img%03d.jpg" % (k, i) for i in range(B)] for k in range(batches)]
    say("whole: ThumbnailWriter over %d batches of %d model inputs at %d in device memory -> %d x %d files, %d repetitions after 1 warm-up"
        % (batches, B, INPUT, SIZE, SIZE, args.repeats))
    res = {}
    for threads in (8, 16):
        rate = []
        for it in range(1 + args.repeats):
            with tempfile.TemporaryDirectory() as tmp:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with ThumbnailWriter(tmp, SIZE, QUALITY, 0, threads) as tw:
                    for k in range(batches):
                        tw.add(paths[k], images)
                dt = time.perf_counter() - t0
            if it >= 1:
                rate.append(batches * B / dt)
        st = stats(rate)
        res[str(threads)] = st
        say("  %2d threads  median %8.0f thumbnails/s  (min %.0f, max %.0f, n %d)" % (threads, st["median"], st["min"], st["max"], st["n"]))
    say(json.dumps({"thumbs_bench_whole": {"thumbnails_per_s_by_threads": res}}))


def _pillow_thumbnails(args):
    from PIL import Image
    first, count = args
    x = picture(first, INPUT)
    t0 = time.perf_counter()
    for _ in range(count):
        buf = io.BytesIO()
        Image.fromarray(x).resize((SIZE, SIZE), Image.BICUBIC).save(buf, "JPEG", quality=QUALITY)
    return time.perf_counter() - t0


def step_reference(args, say):
    per = 256
    say("reference (Pillow on the host, not the code under test): resize %d -> %d (BICUBIC) + save(quality=%d) into memory, %d per process"
        % (INPUT, SIZE, QUALITY, per))
    res = {}
    for procs in (1, 16):
        rate = []
        with concurrent.futures.ProcessPoolExecutor(procs) as ex:
            for it in range(1 + args.repeats):
                t0 = time.perf_counter()
                list(ex.map(_pillow_thumbnails, [(p, per) for p in range(procs)]))
                dt = time.perf_counter() - t0
                if it >= 1:
                    rate.append(procs * per / dt)
        st = stats(rate)
        res[str(procs)] = st
        say("  %2d processes  median %8.0f thumbnails/s  (min %.0f, max %.0f, n %d)" % (procs, st["median"], st["min"], st["max"], st["n"]))
    say(json.dumps({"thumbs_bench_reference": {"thumbnails_per_s_by_processes": res}}))


def _make_file(a):
    from PIL import Image
    d, i = a
    rng = np.random.default_rng(i)
    small = rng.integers(0, 256, (24, 32, 3), dtype=np.uint8)
    big = np.asarray(Image.fromarray(small).resize((1024, 768), Image.BICUBIC)).astype(np.int16) + rng.integers(-6, 7, (768, 1024, 3), dtype=np.int16)
    Image.fromarray(np.clip(big, 0, 255).astype(np.uint8)).save(os.path.join(d, "img%05d.jpg" % i), quality=90)


def step_tagging(args, say):
    n = args.files
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "imgs")
        os.makedirs(d)
        with concurrent.futures.ProcessPoolExecutor(16) as ex:
            list(ex.map(_make_file, [(d, i) for i in range(n)], chunksize=16))
        say("tagging: tagging.py --workers 16 --gpu-resize --gpu-jpeg over %d JPEGs of 1024 x 768 (vit-b16, seeded weights), rows A B A B; "
            "seconds of the whole child process, start-up and model set-up included" % n)
        base = [sys.executable, os.path.join(PKG, "tagging.py"), "--dir", d, "--workers", "16", "--gpu-resize", "--gpu-jpeg"]
        secs = {"A": [], "B": []}
        tags = None
        for k in range(2 * args.tagging_pairs):
            row = "AB"[k & 1]
            cwd = os.path.join(tmp, "run%d" % k)
            os.makedirs(cwd)
            cmd = base + (["--thumbnails", "thumbs"] if row == "B" else [])
            t0 = time.perf_counter()
            r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=200)
            dt = time.perf_counter() - t0
            if r.returncode != 0:
                say(r.stderr[-2000:])
                raise SystemExit("tagging.py ended with status %d; nothing more is started" % r.returncode)
            text = open(os.path.join(cwd, "tags-wd-tagger.txt"), "rb").read()
            assert tags is None or text == tags, "the tag file differs between the rows"
            tags = text
            made = sum(len(f) for _, _, f in os.walk(os.path.join(cwd, "thumbs"))) - 1 if row == "B" else 0
            secs[row].append(dt)
            say("  %s %-22s %7.2f s  = %6.0f images/s%s" % (row, "with --thumbnails" if row == "B" else "without", dt, n / dt,
                                                          "  (%d thumbnails)" % made if row == "B" else ""))
        a, b = float(np.median(secs["A"])), float(np.median(secs["B"]))
        say("  medians: %.2f s without, %.2f s with: %+.2f s (%+.1f %%) for %d thumbnails; the tag files are equal" % (a, b, b - a, 100 * (b - a) / a, n))
        say(json.dumps({"thumbs_bench_tagging": {"files": n, "seconds_without": secs["A"], "seconds_with": secs["B"]}}))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--step", choices=STEPS, default=None, help="run one step in this process (default: all, one child process each)")
    ap.add_argument("--steps", nargs="+", choices=STEPS, default=list(STEPS), help="the steps to run as child processes")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=2000, help="kernel step: calls between two events")
    ap.add_argument("--files", type=int, default=4096, help="tagging step: JPEG files")
    ap.add_argument("--tagging-pairs", type=int, default=2, help="tagging step: A B pairs")
    ap.add_argument("--out", default=None, help="also append the report to this file")
    args = ap.parse_args()
    report = []

    def say(s):
        print(s, flush=True)
        report.append(s)

    if args.step:
        {"kernel": step_kernel, "coder": step_coder, "whole": step_whole, "reference": step_reference, "tagging": step_tagging}[args.step](args, say)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write("\n".join(report) + "\n")
        return 0
    if args.out and os.path.exists(args.out):
        os.remove(args.out)
    common = ["--repeats", str(args.repeats), "--warmup", str(args.warmup), "--calls", str(args.calls), "--files", str(args.files),
              "--tagging-pairs", str(args.tagging_pairs)]
    for step in args.steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + common + (["--out", args.out] if args.out else [])
        try:
            rc = subprocess.run(cmd, timeout=LIMITS[step]).returncode
        except subprocess.TimeoutExpired:
            print("thumbs_bench: step %s ran out of its %d s; nothing more is started" % (step, LIMITS[step]), flush=True)
            return 124
        if rc != 0:
            print("thumbs_bench: step %s ended with status %d; nothing more is started" % (step, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
