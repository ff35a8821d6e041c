#!/usr/bin/env python3
"""Read-name coder size and timing.

  python tools/name_bench.py --sizes [--records 3000,200000,2000000] [--out profiles/r11_name_sizes.json]
  python tools/name_bench.py --archive 20000000 [--repeats 3] [--dir DIR] [--out FILE]
  python tools/name_bench.py --records 20000000 [--style illumina|sra] [--gpu] [--skip-host] [--repeats 3] [--dir DIR] [--out FILE]

--sizes: on the CPU, by the host twins.  For both generators of tests/name_cases.py and every record count: the `.mcn` member, each of
its seven streams (raw and as the member holds it), and `.bwt`, `.rans`, `xz -6` and `bz2 -9` of the name text.  One JSON document.
Without --sizes, files -> files on one name text: `bin/mcomz e --names` / `mcomz d` on the host twin (and on GPU 0 with --gpu) against
`xz -6 -T16` of the same text, both directions.  Every route runs once to warm up and `--repeats` times measured: wall clock around
the child process, median and spread (max - min); every decoded file is compared with its source and the two routes' members with one
another (--skip-host: the GPU route and xz only, for sizes at which the host twin takes minutes).  One JSON line (also written to --out).  Exit status 1 when a route fails or bytes differ.  Nothing is retried.
--archive N: `bin/minicom -d -G` of a `-p -Q -N -G` archive of N synthetic reads of 100 bases against the same file's archive without -N
(the parent's route is the yardstick; the difference is the cost of names), median of --repeats with the spread, outputs compared with
the input.  Needs a GPU."""
import argparse
import bz2
import filecmp
import json
import lzma
import os
import shutil
import statistics
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MCOMZ = os.path.join(ROOT, "bin", "mcomz")
STREAMS = ("ops", "delta", "num", "tlen", "text", "plus", "ptext")


sys.path.insert(0, os.path.join(ROOT, "tests"))
from name_cases import illumina, sra  # noqa: E402  (the generators of the tests: one copy)


def name_text(names):
    return b"".join(nm + b"\n\n" for nm in names)


def sizes(counts):
    from minicom_amd import pipeline
    rows = []
    for style, gen in (("illumina", illumina), ("sra", sra)):
        for n in counts:
            text = name_text(gen(1, n))
            member = pipeline.name_encode(text, n)
            assert pipeline.name_decode(member) == text
            lens = struct.unpack_from("<7Q", member, 32)
            row = {"style": style, "records": n, "text": len(text), "mcn": len(member), "kind": member[5], "streams": dict(zip(STREAMS, lens)),
                   "bwt": len(pipeline.bwt_encode(text)), "rans": len(pipeline.rans_encode(text)), "xz6": len(lzma.compress(text, preset=6)),
                   "bz2_9": len(bz2.compress(text, 9))}
            row["bytes_per_name"] = round(len(member) / n, 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return {"tool": "tools/name_bench.py --sizes", "generators": "tests/name_cases.py, seed 1, bare '+' lines", "rows": rows}


def timed(cmd, repeats, cwd=None):
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, cwd=cwd)
    ts = []
    for _ in range(repeats):
        t = time.perf_counter(); subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, cwd=cwd); ts.append(time.perf_counter() - t)
    return {"median_s": round(statistics.median(ts), 4), "spread_s": round(max(ts) - min(ts), 4)}


def archive(n, repeats, where, out_path):
    """minicom -d -G with and without names"""
    from minicom_amd import synth
    minicom = os.path.join(ROOT, "bin", "minicom")
    d = tempfile.mkdtemp(dir=where)
    try:
        reads = synth.synth_reads(1002, n, 100)
        rng = np.random.default_rng(3)
        quals = rng.integers(35, 74, (n, 100), dtype=np.uint8)
        names = illumina(1, n)
        with open(os.path.join(d, "X.fastq"), "wb") as f:
            for i in range(n):
                f.write(b"@" + names[i] + b"\n" + reads[i].tobytes() + b"\n+\n" + quals[i].tobytes() + b"\n")
        res = {"reads": n, "fastq": os.path.getsize(os.path.join(d, "X.fastq"))}
        ok = True
        for tag, flag in (("with_names", ["-N"]), ("without_names", [])):
            sub = os.path.join(d, tag); os.mkdir(sub)
            os.link(os.path.join(d, "X.fastq"), os.path.join(sub, "X.fastq"))
            subprocess.run(["bash", minicom, "-r", "X.fastq", "-p", "-Q", "-G"] + flag, cwd=sub, check=True, stdout=subprocess.DEVNULL)
            res[tag + "_archive"] = os.path.getsize(os.path.join(sub, "X_comp_order.minicom"))
            res[tag + "_decode"] = timed(["bash", minicom, "-d", "X_comp_order.minicom", "-G"], repeats, cwd=sub)
            if tag == "with_names":
                ok &= filecmp.cmp(os.path.join(sub, "X.fastq"), os.path.join(sub, "X_comp_order_dec.fastq"), shallow=False)
        res["bytes_ok"] = bool(ok)
        line = json.dumps(res)
        print(line)
        if out_path:
            with open(out_path, "w") as f:
                f.write(line + "\n")
        return 0 if ok else 1
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", action="store_true"); ap.add_argument("--records", default=None); ap.add_argument("--style", default="illumina")
    ap.add_argument("--gpu", action="store_true"); ap.add_argument("--skip-host", action="store_true"); ap.add_argument("--archive", type=int, default=0); ap.add_argument("--repeats", type=int, default=3); ap.add_argument("--dir", default=None); ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.sizes:
        doc = sizes([int(v) for v in (a.records or "3000,200000,2000000").split(",")])
        if a.out:
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1); f.write("\n")
        return 0
    if a.archive:
        return archive(a.archive, a.repeats, a.dir, a.out)
    n = int(a.records or 20000000)
    d = tempfile.mkdtemp(dir=a.dir)
    ok = True
    try:
        src = os.path.join(d, "names.txt")
        with open(src, "wb") as f:
            f.write(name_text((illumina if a.style == "illumina" else sra)(1, n)))
        res = {"style": a.style, "records": n, "text": os.path.getsize(src)}
        routes = ([] if a.skip_host else [("host", [])]) + ([("gpu", ["--gpu"])] if a.gpu else [])
        for tag, flag in routes:
            mem, back = os.path.join(d, tag + ".mcn"), os.path.join(d, tag + ".txt")
            res[tag + "_encode"] = timed([MCOMZ, "e", "--names"] + flag + [src, mem], a.repeats)
            res[tag + "_decode"] = timed([MCOMZ, "d"] + flag + [mem, back], a.repeats)
            res[tag + "_bytes"] = os.path.getsize(mem)
            ok &= filecmp.cmp(src, back, shallow=False)
        if a.gpu and not a.skip_host:
            res["same_member"] = filecmp.cmp(os.path.join(d, "host.mcn"), os.path.join(d, "gpu.mcn"), shallow=False); ok &= res["same_member"]
        if shutil.which("xz"):
            xz = os.path.join(d, "names.txt.xz")
            res["xz_encode"] = timed(["sh", "-c", "xz -6 -T16 -k -f -c '%s' > '%s'" % (src, xz)], a.repeats)
            res["xz_decode"] = timed(["sh", "-c", "xz -d -T16 -c '%s' > '%s'" % (xz, os.path.join(d, "xz.txt"))], a.repeats)
            res["xz_bytes"] = os.path.getsize(xz)
        res["bytes_ok"] = bool(ok)
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
