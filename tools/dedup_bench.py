#!/usr/bin/env python3
"""Near-duplicate detection at the sizes the project is measured at (hiptagsearch/dedup.py; csrc/imghash.hip, csrc/radius.hip).

  hash    hipts_image_hash_u8 on a batch of 64 uniform-noise images at 448, device memory in and out: HIP events around --calls calls
          per repetition, for the library's own choice of workgroups per image and for HIPTS_IMGHASH_SPLIT = 1, 2, 4, 8, 16, 32, 64,
          A B ... A B ...; the hashes of every setting are compared.  Floor: the 38.5 MB of the batch over the HBM rate.
  pairs   ImageHashIndex over --rows random 128-bit rows, 1 % of them copies of another row with at most 10 bits flipped, T = 10:
          hipts_radius_create_hamming alone -- pass 1 and pass 2 from the library's HIP events (hiptsdbg_radius_passes), the whole call
          from a host clock (it ends synchronised) -- and the whole groups() call.  Floor per pass: rows^2 / 2 pairs x nine vector
          instructions over 256 CUs x 4 SIMDs x 16 lanes per cycle; printed as cycles, and as seconds at the clock --clock-ghz names.
  host    the numpy statement of the same lists (float32 products of the unpacked bits, exact below 2^24) at --host-rows rows.

Without --step the three steps run one after the other, each as a child process of its own under its own time limit; the first one
that fails, faults or runs out of time ends the run.  Needs a GPU; there is no fallback."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "anime-illust-image-searcher_amd"))
import numpy as np  # noqa: E402

T = 10
SPLITS = [0, 1, 2, 4, 8, 16, 32, 64]        # 0: the library's choice
LIMITS = {"hash": 240, "pairs": 420, "host": 300}      # seconds per step


def stats(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]), "n": len(a)}


def fmt(s):
    return "median %9.3f ms  (min %.3f, max %.3f, n %d)" % (s["median_ms"], s["min_ms"], s["max_ms"], s["n"])


def rows_with_copies(n, seed=47):
    rng = np.random.default_rng(seed)
    H = rng.integers(0, 1 << 64, (n, 2), dtype=np.uint64)
    k = n // 100
    dst = rng.choice(n, k, replace=False)
    src = rng.integers(0, n, k)
    flips = np.zeros((k, 2), dtype=np.uint64)
    for _ in range(T):                          # ten single bits, which may coincide: at most ten differ
        bit = rng.integers(0, 128, k)
        flips[np.arange(k), bit // 64] ^= np.uint64(1) << (bit % 64).astype(np.uint64)
    keep = rng.random(k) < 0.7                  # some copies are exact
    H[dst] = H[src] ^ np.where(keep[:, None], flips, np.uint64(0))
    return H


def step_hash(args, say):
    import torch
    from hiptagsearch import _lib
    if not torch.cuda.is_available():
        raise SystemExit("dedup_bench needs a GPU")
    B, S = 64, 448
    gen = torch.Generator(device="cuda").manual_seed(5)
    images = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device="cuda", generator=gen)
    out = torch.zeros((B, 2), dtype=torch.int64, device="cuda")
    stream = _lib.current_stream_ptr()

    def run(split, calls):
        if split:
            os.environ["HIPTS_IMGHASH_SPLIT"] = str(split)
        else:
            os.environ.pop("HIPTS_IMGHASH_SPLIT", None)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            _lib.call("hipts_image_hash_u8", _lib.ptr(images), _lib.DEVICE, B, S, _lib.ptr(out), _lib.DEVICE, 0, stream)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls, out.cpu().numpy().copy()
    say("hash: %d images at %d (%.1f MB), %d calls per repetition, %d repetitions after %d warm-up, settings interleaved"
        % (B, S, B * S * S * 3 / 1e6, args.calls, args.repeats, args.warmup))
    ms = {s: [] for s in args.splits}
    ref = None
    for it in range(args.warmup + args.repeats):
        for s in args.splits:
            t, h = run(s, args.calls)
            ref = h if ref is None else ref
            assert (h == ref).all(), "HIPTS_IMGHASH_SPLIT=%d changes the hashes" % s
            if it >= args.warmup:
                ms[s].append(t)
    os.environ.pop("HIPTS_IMGHASH_SPLIT", None)
    res = {}
    for s in args.splits:
        st = stats(ms[s])
        res[str(s)] = st
        say("  %-28s %s  %.2f TB/s of the batch's bytes" % ("library's choice" if s == 0 else "%d workgroups per image" % s, fmt(st),
                                                            B * S * S * 3 / st["median_ms"] / 1e9))
    say("  all settings give the same hashes; floor: %.1f MB per batch; the forward it would run next to takes 11.8 ms per batch" % (B * S * S * 3 / 1e6))
    say(json.dumps({"dedup_bench_hash": {"batch": B, "size": S, "per_call_ms_by_split": res}}))


def step_pairs(args, say):
    import torch
    from hiptagsearch import _lib
    from hiptagsearch.dedup import ImageHashIndex
    if not torch.cuda.is_available():
        raise SystemExit("dedup_bench needs a GPU")
    lib = _lib.load()
    for n in args.rows:
        H = rows_with_copies(n)
        index = ImageHashIndex()
        index.add(["img%07d.png" % i for i in range(n)], H)
        say("pairs: %d rows, %d of them copies, T = %d; %d repetitions after %d warm-up" % (n, n // 100, T, args.repeats, args.warmup))
        p1, p2, srt, whole, grp = [], [], [], [], []
        pairs = labels = None
        for it in range(args.warmup + args.repeats):
            h = ctypes.c_void_p()
            t0 = time.perf_counter()
            _lib.call("hipts_radius_create_hamming", _lib.ptr(H), _lib.HOST, ctypes.c_int64(n), T, ctypes.c_int64(0), 0, _lib.current_stream_ptr(),
                      ctypes.byref(h))
            w = (time.perf_counter() - t0) * 1e3                # create ends in a stream synchronisation
            a, b, c, np_ = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
            assert lib.hiptsdbg_radius_passes(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
            _lib.call("hipts_radius_info", h, None, ctypes.byref(np_))
            _lib.call("hipts_radius_destroy", h)
            assert pairs is None or pairs == np_.value
            pairs = np_.value
            t0 = time.perf_counter()
            labels = index.groups(T)
            g = (time.perf_counter() - t0) * 1e3                # ends with the labels on the host
            if it >= args.warmup:
                p1.append(a.value), p2.append(b.value), srt.append(c.value), whole.append(w), grp.append(g)
        cycles = (n * n / 2.0) * 9 / (256 * 4 * 16)
        say("  pass 1 (degrees)             %s" % fmt(stats(p1)))
        say("  pass 2 (ids)                 %s" % fmt(stats(p2)))
        say("  row sort                     %s" % fmt(stats(srt)))
        say("  create, whole call           %s  (the copy of the rows, both passes, scan, sort)" % fmt(stats(whole)))
        say("  groups(), whole call         %s  (set-bit filter on the host, create, DBSCAN, labels back)" % fmt(stats(grp)))
        say("  %d neighbour pairs (the %d rows themselves included); %d groups, %d rows in groups" % (pairs, n, int(labels.max()) + 1, int((labels >= 0).sum())))
        say("  floor per pass: %.3g pairs x 9 vector instructions / (256 CUs x 4 SIMDs x 16 lanes) = %.3g cycles = %.1f ms at %.1f GHz "
            "(the clock under this load was not measured: arithmetic, not a target)" % (n * n / 2.0, cycles, cycles / args.clock_ghz / 1e6, args.clock_ghz))
        say(json.dumps({"dedup_bench_pairs": {"rows": n, "pairs": pairs, "pass1": stats(p1), "pass2": stats(p2), "sort": stats(srt),
                                              "create": stats(whole), "groups": stats(grp)}}))


def host_lists(H, chunk=2000):
    """(ptr, ids) of the relation by numpy: float32 products of the unpacked bits (sums of at most 128 ones: exact)"""
    bits = np.unpackbits(H.view(np.uint8).reshape(len(H), 16), axis=1).astype(np.float32)
    ones = bits.sum(axis=1)
    counts, ids = [], []
    for s in range(0, len(H), chunk):
        d = ones[s:s + chunk, None] + ones[None, :] - 2.0 * (bits[s:s + chunk] @ bits.T)
        r, c = np.nonzero(d <= T)
        counts.append(np.bincount(r, minlength=len(d)))
        ids.append(c.astype(np.int32))
    ptr = np.zeros(len(H) + 1, dtype=np.int64)
    np.cumsum(np.concatenate(counts), out=ptr[1:])
    return ptr, np.concatenate(ids)


def step_host(args, say):
    from hiptagsearch.dedup import ImageHashIndex
    n = args.host_rows
    H = rows_with_copies(n)
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        ptr, ids = host_lists(H)
        ms.append((time.perf_counter() - t0) * 1e3)
    index = ImageHashIndex()
    index.add([""] * n, H)
    dptr, dids = index.neighbors(T)
    assert (ptr == dptr).all() and (ids == dids).all(), "the device lists differ from numpy's"
    st = stats(ms)
    say("host: numpy lists at %d rows (float32 products of the unpacked bits, the BLAS's threads)  %s; equal to the device's lists"
        % (n, fmt(st)))
    say("  SCALED by (100000 / %d)^2 to 100 000 rows, not measured there: %.0f ms" % (n, st["median_ms"] * (100000.0 / n) ** 2))
    say(json.dumps({"dedup_bench_host": {"rows": n, "lists": st}}))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--step", choices=["hash", "pairs", "host"], default=None, help="run one step in this process (default: all, one child process each)")
    ap.add_argument("--rows", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--host-rows", type=int, default=20_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=2000, help="hash step: calls between two events")
    ap.add_argument("--splits", type=int, nargs="+", default=SPLITS, help="hash step: the HIPTS_IMGHASH_SPLIT settings (0: the library's choice)")
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="the clock the floor is turned into seconds with")
    ap.add_argument("--out", default=None, help="also append the report to this file")
    args = ap.parse_args()
    report = []

    def say(s):
        print(s, flush=True)
        report.append(s)

    if args.step:
        {"hash": step_hash, "pairs": step_pairs, "host": step_host}[args.step](args, say)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write("\n".join(report) + "\n")
        return 0
    if args.out and os.path.exists(args.out):
        os.remove(args.out)
    common = ["--repeats", str(args.repeats), "--warmup", str(args.warmup), "--calls", str(args.calls), "--clock-ghz", str(args.clock_ghz),
              "--host-rows", str(args.host_rows), "--splits"] + [str(x) for x in args.splits] + ["--rows"] + [str(r) for r in args.rows]
    for step in ("hash", "pairs", "host"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + common + (["--out", args.out] if args.out else [])
        try:
            rc = subprocess.run(cmd, timeout=LIMITS[step]).returncode
        except subprocess.TimeoutExpired:
            print("dedup_bench: step %s ran out of its %d s; nothing more is started" % (step, LIMITS[step]), flush=True)
            return 124
        if rc != 0:
            print("dedup_bench: step %s ended with status %d; nothing more is started" % (step, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
