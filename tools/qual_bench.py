#!/usr/bin/env python3
"""Quality-coder timing and size, files -> files: `xz -6 -T16` against `bin/mcomz e --qual L` on the host twin and on GPU 0, on one
quality matrix, both directions.

  python tools/qual_bench.py --rows 2000000 --len 150 [--binned] [--fastq FILE] [--repeats 3] [--dir DIR] [--out FILE]

The matrix is the synthetic generator of the tests (a first-order walk; --binned: four values) or, with --fastq, the quality lines of a
four-line FASTQ file of one read length -- the way to learn what real instrument qualities gain.  Every route runs once to warm up (page
cache included) and `--repeats` times measured: wall clock around the child process, median and spread (max - min).  Also reported:
the `.rans` member and bz2 -9 of the same bytes (sizes only), the model the coder chose, whether the host twin and the GPU wrote the
same member and whether every route gave the bytes back.  One JSON line (also written to --out).  Exit status 1 when a route fails, a
decoded file differs from its source, or the two routes' members differ.  Nothing is retried."""
import argparse
import bz2
import filecmp
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MCOMZ = os.path.join(ROOT, "bin", "mcomz")


def synth_quals(seed, n, L, binned=False):
    """the generator of tests/qual_cases.py"""
    rng = np.random.default_rng(seed); q = np.empty((n, L), np.int64)
    base = rng.choice(np.array([38, 34, 28]), size=n, p=[.6, .3, .1]); cur = base.copy()
    for j in range(L):
        drop = rng.random(n) < (0.01 + 0.10 * j / L); rec = rng.random(n) < 0.5
        down = np.maximum(2, cur - rng.integers(5, 25, n)); up = np.minimum(base, cur + rng.integers(1, 8, n))
        cur = np.where(drop, down, np.where(rec, up, cur)); q[:, j] = cur
    if binned: q = np.array([2, 12, 23, 37])[np.digitize(q, [10, 20, 30])]
    return (q + 33).astype(np.uint8)


def timed(cmd, stdout=None):
    t0 = time.perf_counter()
    p = subprocess.run(cmd, stdout=stdout, stderr=subprocess.PIPE)
    ms = (time.perf_counter() - t0) * 1e3
    if p.returncode:
        raise RuntimeError("%s failed: %s" % (" ".join(cmd), p.stderr.decode(errors="replace")[-500:]))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150, dest="L")
    ap.add_argument("--binned", action="store_true")
    ap.add_argument("--fastq", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from minicom_amd import pipeline
    work = tempfile.mkdtemp(prefix="qual_bench_", dir=a.dir)
    try:
        src = os.path.join(work, "qual.raw")
        if a.fastq:
            with open(a.fastq, "rb") as f:
                lines = f.read().split(b"\n")[3::4]
            L = len(lines[0])
            lines = [l for l in lines if l]
            if any(len(l) != L for l in lines):
                print("qual_bench: quality lines of more than one length", file=sys.stderr)
                return 1
            raw = b"".join(lines)
            rows = len(lines)
        else:
            L, rows = a.L, a.rows
            raw = synth_quals(5, rows, L, a.binned).tobytes()
        with open(src, "wb") as f:
            f.write(raw)
        xz, mh, mg, back = src + ".xz", src + ".h.mcq", src + ".g.mcq", src + ".back"

        def xz_e():
            with open(xz, "wb") as f:
                return timed(["xz", "-6", "-T16", "-c", src], stdout=f)

        def xz_d():
            with open(back, "wb") as f:
                return timed(["xz", "-d", "-T16", "-c", xz], stdout=f)
        routes = {"xz": (xz_e, xz_d, xz),
                  "host": (lambda: timed([MCOMZ, "e", "--qual", str(L), src, mh]), lambda: timed([MCOMZ, "d", mh, back]), mh),
                  "gpu": (lambda: timed([MCOMZ, "e", "--qual", str(L), "--gpu", src, mg]), lambda: timed([MCOMZ, "d", "--gpu", mg, back]), mg)}
        res = {"rows": rows, "L": L, "source": a.fastq or ("synthetic, binned" if a.binned else "synthetic"), "repeats": a.repeats, "raw_bytes": len(raw)}
        same = True
        for r, (enc, dec, coded) in routes.items():
            enc(); dec()                                                   # warm-up
            e = [enc() for _ in range(a.repeats)]
            d = [dec() for _ in range(a.repeats)]
            same = same and filecmp.cmp(src, back, shallow=False)
            res[r] = {"bytes": os.path.getsize(coded), "enc_ms": round(statistics.median(e), 1), "enc_spread_ms": round(max(e) - min(e), 1),
                      "dec_ms": round(statistics.median(d), 1), "dec_spread_ms": round(max(d) - min(d), 1)}
        same = same and filecmp.cmp(mh, mg, shallow=False)
        with open(mg, "rb") as f:
            head = f.read(8)
        res["kind"], res["model"] = head[5], pipeline.QUAL_MODELS[head[6]]
        res["rans_bytes"] = len(pipeline.rans_encode(raw))
        res["bz2_9_bytes"] = len(bz2.compress(raw, 9))
        res["same_bytes"] = same
        for k in ("enc", "dec"):
            res[k + "_gpu_faster_than_xz_by_ms"] = round(res["xz"][k + "_ms"] - res["gpu"][k + "_ms"], 1)
        res["ok"] = same
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return 0 if same else 1
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
