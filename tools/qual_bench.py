#!/usr/bin/env python3
"""Quality-coder timing and size, files -> files: `xz -6 -T16` against `bin/mcomz e --qual L` on the host twin and on GPU 0, on one
quality matrix, both directions.

  python tools/qual_bench.py --rows 2000000 --len 150 [--binned] [--fastq FILE] [--repeats 3] [--dir DIR] [--out FILE]

The matrix is the synthetic generator of the tests (a first-order walk; --binned: four values) or, with --fastq, the quality lines of a
four-line FASTQ file of one read length -- the way to learn what real instrument qualities gain.  Every route runs once to warm up (page
cache included) and `--repeats` times measured: wall clock around the child process, median and spread (max - min).  Also reported:
the `.rans` member and bz2 -9 of the same bytes (sizes only), the model the coder chose, whether the host twin and the GPU wrote the
same member and whether every route gave the bytes back.  One JSON line (also written to --out).  Exit status 1 when a route fails, a
decoded file differs from its source, or the two routes' members differ.  Nothing is retried.

  python tools/qual_bench.py --rows 2000000 --len 150 --lossy ill8 pblock:2 [--repeats 3] [--dir DIR] [--out FILE]

measures the lossy transform instead (`minicom -b`), per SPEC: mcom_qual_transform on GPU 0 over the matrix in HBM
(wall clock around the synchronous call -- its fill, its launch, the 32 bytes of the report coming back and the wait -- against the byte
model of 2 n L bytes moved), the report, and the member step `mcomz e --fastq-qual L --gpu` over a FASTQ file of the same qualities with
and without `--lossy SPEC` (wall clock around the child process, sizes of the members, whether the host twin writes the same member
where --host-check is given).  Median and spread (max - min) of --repeats runs after one warm-up.

  python tools/qual_bench.py --rows 2000000 --len 150 --agree 40:3 40:2 [--lossy ill8] [--repeats 3] [--dir DIR] [--out FILE] [--sizes FILE]

measures the consensus-guided transform (`minicom -a Q[:C]`) on a -p archive of synthetic reads (coverage 30,
substitution rate 0.5 %) with the synthetic qualities: per Q:C the share of mask bits set, the time of the mask step (`decompress
--agree-mask --gpu`) against the plain stream-files -> rows decode of the same folder (`decompress --gpu`), the time of the quality-member
step with and without `--agree`, and the size of `qual.mcq` against the member made without it; with --lossy also Q:C of the first --agree
argument followed by SPEC.  Wall clock around the child processes.  The generator's qualities are independent of its base errors: the
sizes say nothing about real instrument data.  --sizes: the sizes alone as JSON."""
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


def fastq_file(path, quals):
    """four-line records of one width (names @0000001 ..., reads of A) around the quality rows, built as one matrix"""
    n, L = quals.shape
    rec = np.empty((n, 2 * L + 13), np.uint8)
    rec[:, 0] = ord("@")
    idx = np.arange(1, n + 1)
    for k in range(7):
        rec[:, 7 - k] = 48 + idx // 10 ** k % 10
    rec[:, 8] = 10; rec[:, 9:9 + L] = ord("A"); rec[:, 9 + L] = 10; rec[:, 10 + L] = ord("+"); rec[:, 11 + L] = 10
    rec[:, 12 + L:12 + 2 * L] = quals; rec[:, 12 + 2 * L] = 10
    with open(path, "wb") as f:
        f.write(rec.tobytes())


def lossy_main(a):
    import torch
    import minicom_amd
    from minicom_amd import pipeline
    work = tempfile.mkdtemp(prefix="qual_bench_", dir=a.dir)
    try:
        L, rows = a.L, a.rows
        q = synth_quals(5, rows, L, a.binned)
        fq = os.path.join(work, "q.fastq")
        fastq_file(fq, q)
        ctx = minicom_amd.Context(0)
        d = torch.from_numpy(q).cuda()
        res = {"rows": rows, "L": L, "repeats": a.repeats, "bytes_moved_model": 2 * rows * L, "specs": {}}

        def member(extra, out):
            return timed([MCOMZ, "e", "--fastq-qual", str(L)] + extra + ["--gpu", fq, out], stdout=subprocess.DEVNULL)
        plain = os.path.join(work, "plain.mcq")
        member([], plain)
        t = [member([], plain) for _ in range(a.repeats)]
        res["member_plain"] = {"bytes": os.path.getsize(plain), "ms": round(statistics.median(t), 1), "spread_ms": round(max(t) - min(t), 1)}
        ok = True
        for spec in a.lossy:
            work_rows = d.clone()
            ctx.qual_transform(work_rows, spec, in_place=True)             # warm-up
            ms = []
            for _ in range(max(a.repeats, 3)):
                work_rows.copy_(d); torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, report = ctx.qual_transform(work_rows, spec, in_place=True)
                ms.append((time.perf_counter() - t0) * 1e3)
            med = statistics.median(ms)
            out = os.path.join(work, "lossy.mcq")
            member(["--lossy", spec], out)
            t = [member(["--lossy", spec], out) for _ in range(a.repeats)]
            r = {"transform_call_ms": round(med, 3), "transform_call_spread_ms": round(max(ms) - min(ms), 3), "model_GB_per_s": round(2 * rows * L / med / 1e6, 1),
                 "report": report, "member_bytes": os.path.getsize(out), "member_ms": round(statistics.median(t), 1), "member_spread_ms": round(max(t) - min(t), 1)}
            if a.host_check:
                host = os.path.join(work, "host.mcq")
                timed([MCOMZ, "e", "--fastq-qual", str(L), "--lossy", spec, fq, host], stdout=subprocess.DEVNULL)
                r["same_bytes_as_host"] = filecmp.cmp(out, host, shallow=False)
                ok = ok and r["same_bytes_as_host"]
            res["specs"][spec] = r
        res["ok"] = ok
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return 0 if ok else 1
    finally:
        shutil.rmtree(work, ignore_errors=True)


def agree_main(a):
    from minicom_amd import synth
    from minicom_amd.pipeline import Pipeline
    DECOMPRESS = os.path.join(ROOT, "bin", "decompress")
    work = tempfile.mkdtemp(prefix="qual_bench_", dir=a.dir)
    try:
        L, rows = a.L, a.rows
        reads = synth.synth_reads(1002, rows, L)
        q = synth_quals(5, rows, L, a.binned)
        fq = os.path.join(work, "q.fastq")
        fastq_file(fq, q)                                                  # (the member step reads the quality lines only)
        folder = os.path.join(work, "streams")
        os.mkdir(folder)
        p = Pipeline(reads, host_threads=16); p.pre_process()
        try:
            p.cluster_dump(folder, order=True, paired=False)
        finally:
            p.close()

        def runs(cmd):
            timed(cmd, stdout=subprocess.DEVNULL)                          # warm-up
            t = [timed(cmd, stdout=subprocess.DEVNULL) for _ in range(a.repeats)]
            return {"ms": round(statistics.median(t), 1), "spread_ms": round(max(t) - min(t), 1)}
        res = {"rows": rows, "L": L, "repeats": a.repeats, "what": "synthetic reads (coverage 30, 0.5 % substitutions) and synthetic qualities, independent of each other", "agree": {}}
        res["decode_rows"] = runs([DECOMPRESS, "--gpu", folder, os.path.join(work, "reads.out"), "false", "true", "1"])
        plain = os.path.join(work, "plain.mcq")
        res["member_plain"] = dict(runs([MCOMZ, "e", "--fastq-qual", str(L), "--gpu", fq, plain]), bytes=os.path.getsize(plain))
        sizes = {"rows": rows, "L": L, "qual.mcq": os.path.getsize(plain)}
        legs = [(s, None) for s in a.agree] + ([(a.agree[0], spec) for spec in a.lossy] if a.lossy else [])
        for spec, lossy in legs:
            Q, C = (spec.split(":") + ["3"])[:2]
            mask, out = os.path.join(work, "m.mask"), os.path.join(work, "agree.mcq")
            r = {"mask_step": runs([DECOMPRESS, "--agree-mask", "--gpu", folder, C, mask])}
            n_rows, _, bits = subprocess.run([DECOMPRESS, "--agree-mask", "--gpu", folder, C, mask], check=True, capture_output=True, text=True).stdout.split()
            r["mask_bits_share"] = round(int(bits) / (int(n_rows) * L), 4)
            r["member"] = dict(runs([MCOMZ, "e", "--fastq-qual", str(L), "--agree", Q, mask] + (["--lossy", lossy] if lossy else []) + ["--gpu", fq, out]), bytes=os.path.getsize(out))
            name = "-a %s:%s" % (Q, C) + (" -b %s" % lossy if lossy else "")
            res["agree"][name] = r
            sizes[name] = {"qual.mcq": r["member"]["bytes"], "mask_bits_share": r["mask_bits_share"]}
        res["ok"] = True
        line = json.dumps(res)
        print(line)
        for path, text in ((a.out, line), (a.sizes, json.dumps(sizes))):
            if path:
                with open(path, "w") as f:
                    f.write(text + "\n")
        return 0
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150, dest="L")
    ap.add_argument("--binned", action="store_true")
    ap.add_argument("--fastq", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lossy", nargs="+", default=None, metavar="SPEC")
    ap.add_argument("--host-check", action="store_true")
    ap.add_argument("--agree", nargs="+", default=None, metavar="Q[:C]")
    ap.add_argument("--sizes", default=None)
    a = ap.parse_args()
    if a.agree:
        return agree_main(a)
    if a.lossy:
        return lossy_main(a)
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
