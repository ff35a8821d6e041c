#!/usr/bin/env python3
"""Read-name coder size and timing (DESIGN.md sections 3.10 and 3.12).

  python tools/name_bench.py --sizes [--records 3000,200000,2000000] [--out profiles/r11_name_sizes.json]
  python tools/name_bench.py --mate-sizes [--records 200000] [--out profiles/r13_mate_name_sizes.json]
  python tools/name_bench.py --mate [--records 2000000] [--style illumina|slash|sra] [--gpu] [--skip-host] [--repeats 3] [--dir DIR] [--out FILE]
  python tools/name_bench.py --mate-archive 2000000 [--repeats 3] [--dir DIR] [--out FILE]
  python tools/name_bench.py --archive 20000000 [--repeats 3] [--dir DIR] [--out FILE]
  python tools/name_bench.py --records 20000000 [--style illumina|sra] [--gpu] [--skip-host] [--repeats 3] [--dir DIR] [--out FILE]

--sizes: on the CPU, by the host twins.  For both generators of tests/name_cases.py and every record count: the `.mcn` member, each of
its seven streams (raw and as the member holds it), and `.bwt`, `.rans`, `xz -6` and `bz2 -9` of the name text.  One JSON document.
--mate-sizes: on the CPU, by the host twins.  For the three pair styles of tests/mate_name_cases.py (` 1:` / ` 2:`, `/1` / `/2`, the same
names in both files) and every record count: the name text of file 2 as the member coded against file 1's names (kind 2) and as the
member coded alone, with the seven streams of each.  One JSON document.
--mate: files -> files on one pair of name texts: `mcomz e --names --mate TEXT1` / `mcomz d --mate TEXT1` (the member of file 2 coded against
file 1's names, kind 2) against `mcomz e --names` / `mcomz d` of the same text coded alone, on the host twin and with --gpu on GPU 0; warm-up
run, median and spread of --repeats, bytes checked.  --mate-archive N: `bin/minicom -d -G` of a `-1 -2 -p -Q -N -G` archive of 2 x N synthetic
reads of 100 bases against the same pair's archive without -N, outputs compared with the inputs.  Needs a GPU.  One JSON line each; no time
is a pass / fail condition.  Both modes also write --profile (default profiles/r13_pair_order.txt): the figures of the mode that ran, the
other mode's figures as the file held them, and **unmeasured on hardware** for whatever has no figure from a GPU (a --mate run without
--gpu measures the host twin only: its GPU lines stay unmeasured).
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


def mate_sizes(counts):
    from minicom_amd import pipeline
    from mate_name_cases import STYLES
    rows = []
    for style, gen in STYLES:
        for n in counts:
            first, second = gen(1, n)
            mate, text = name_text(first), name_text(second)
            member, alone = pipeline.name_encode(text, n, mate=mate), pipeline.name_encode(text, n)
            assert pipeline.name_decode(member, mate=mate) == text
            row = {"style": style, "records": n, "text": len(text), "name_2_against_name_1": len(member), "kind": member[5],
                   "streams": dict(zip(STREAMS, struct.unpack_from("<7Q", member, 32))), "name_2_alone": len(alone), "kind_alone": alone[5],
                   "streams_alone": dict(zip(STREAMS, struct.unpack_from("<7Q", alone, 32))), "ratio": round(len(alone) / len(member), 1)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return {"tool": "tools/name_bench.py --mate-sizes", "generators": "tests/mate_name_cases.py, seed 1, bare '+' lines", "rows": rows}


PROFILE = os.path.join(ROOT, "profiles", "r13_pair_order.txt")
UNMEASURED = "**unmeasured on hardware**"


def write_profile(path, key, res):
    """the text record of --mate / --mate-archive: `key` gets `res`, the other key keeps what the file held"""
    held = {"mate": None, "mate-archive": None}
    if os.path.exists(path):
        for line in open(path):
            for k in held:
                if line.startswith("json %s: " % k):
                    held[k] = json.loads(line[len("json %s: " % k):])
    held[key] = res
    m, a = held["mate"], held["mate-archive"]

    def t(r, k):
        return "%.3f s (spread %.3f)" % (r[k]["median_s"], r[k]["spread_s"]) if r and k in r else UNMEASURED

    out = ["Names of a pair's second file coded against the first file's, and the pair archive in input order (DESIGN.md section 3.12)", "",
           "Written by tools/name_bench.py --mate / --mate-archive; wall clock around the child process, one warm-up run, median of the repeats with",
           "the spread (max - min); every decoded file compared with its source.  No time is a pass / fail condition.", "",
           "1. `mcomz e --names --mate TEXT1` / `mcomz d --mate TEXT1` (kind 2) against `mcomz e --names` / `mcomz d` of the same text coded alone",
           "   python tools/name_bench.py --mate --records 2000000 --gpu [--skip-host]",
           "   records: %s, style: %s, name text of file 2: %s bytes" % ((m["records"], m["style"], m["text_2"]) if m else (UNMEASURED, "-", "-"))]
    for tag, label in (("gpu", "GPU 0 (--gpu)"), ("host", "host twin")):
        out.append("   %s" % label)
        for kind, what in (("mate", "against the mate"), ("alone", "alone")):
            size = m.get("%s_%s_bytes" % (tag, kind)) if m else None
            out.append("     %-17s encode %s, decode %s, member %s" % (what, t(m, "%s_%s_encode" % (tag, kind)), t(m, "%s_%s_decode" % (tag, kind)),
                                                                        ("%d bytes" % size) if size is not None else (UNMEASURED if tag == "gpu" else "not run")))
    out += ["", "2. `minicom -d -G` of a `-1 -2 -p -Q -N -G` archive against the same pair's archive without -N (the difference is the cost of names)",
            "   python tools/name_bench.py --mate-archive N",
            "   pairs: %s (2 x N reads of 100 bases), the two FASTQ files: %s bytes" % ((a["pairs"], a["fastq"]) if a else (UNMEASURED, "-"))]
    for tag, label in (("with_names", "with names"), ("without_names", "without names")):
        out.append("     %-14s decode %s, archive %s" % (label, t(a, tag + "_decode"), ("%d bytes" % a[tag + "_archive"]) if a else UNMEASURED))
    out += ["", "Anything else about these routes -- larger inputs, real instrument names, the encode side of the archive -- is %s." % UNMEASURED, ""]
    for k in ("mate", "mate-archive"):
        if held[k] is not None:
            out.append("json %s: %s" % (k, json.dumps(held[k])))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def mate(n, style, gpu, skip_host, repeats, where, out_path, profile=None):
    """kind 2 against the member coded alone: encode and decode, host twin and GPU"""
    from mate_name_cases import STYLES
    d = tempfile.mkdtemp(dir=where)
    ok = True
    try:
        first, second = dict(STYLES)[style](1, n)
        t1, t2 = os.path.join(d, "names_1.txt"), os.path.join(d, "names_2.txt")
        with open(t1, "wb") as f:
            f.write(name_text(first))
        with open(t2, "wb") as f:
            f.write(name_text(second))
        res = {"style": style, "records": n, "text_2": os.path.getsize(t2)}
        for tag, flag in ([] if skip_host else [("host", [])]) + ([("gpu", ["--gpu"])] if gpu else []):
            for kind, e_args, d_args in (("mate", ["--mate", t1], ["--mate", t1]), ("alone", [], [])):
                mem, back = os.path.join(d, "%s_%s.mcn" % (tag, kind)), os.path.join(d, "%s_%s.txt" % (tag, kind))
                res["%s_%s_encode" % (tag, kind)] = timed([MCOMZ, "e", "--names"] + e_args + flag + [t2, mem], repeats)
                res["%s_%s_decode" % (tag, kind)] = timed([MCOMZ, "d"] + d_args + flag + [mem, back], repeats)
                res["%s_%s_bytes" % (tag, kind)] = os.path.getsize(mem)
                ok &= filecmp.cmp(t2, back, shallow=False)
        if gpu and not skip_host:
            res["same_members"] = all(filecmp.cmp(os.path.join(d, "host_%s.mcn" % k), os.path.join(d, "gpu_%s.mcn" % k), shallow=False) for k in ("mate", "alone")); ok &= res["same_members"]
        res["bytes_ok"] = bool(ok)
        line = json.dumps(res)
        print(line)
        if profile:
            write_profile(profile, "mate", res)
        if out_path:
            with open(out_path, "w") as f:
                f.write(line + "\n")
        return 0 if ok else 1
    finally:
        shutil.rmtree(d, ignore_errors=True)


def mate_archive(n, repeats, where, out_path, profile=None):
    """minicom -d -G of a pair kept in input order, with and without names"""
    from minicom_amd import synth
    from mate_name_cases import illumina_pair
    minicom = os.path.join(ROOT, "bin", "minicom")
    d = tempfile.mkdtemp(dir=where)
    try:
        reads = synth.synth_reads(1002, 2 * n, 100)
        quals = np.random.default_rng(3).integers(35, 74, (2 * n, 100), dtype=np.uint8)
        names = illumina_pair(1, n)
        for k in (0, 1):
            with open(os.path.join(d, "A_%d.fastq" % (k + 1)), "wb") as f:
                for i in range(n):
                    f.write(b"@" + names[k][i] + b"\n" + reads[k * n + i].tobytes() + b"\n+\n" + quals[k * n + i].tobytes() + b"\n")
        res = {"pairs": n, "fastq": sum(os.path.getsize(os.path.join(d, "A_%d.fastq" % k)) for k in (1, 2))}
        ok = True
        for tag, flag in (("with_names", ["-N"]), ("without_names", [])):
            sub = os.path.join(d, tag); os.mkdir(sub)
            for k in (1, 2):
                os.link(os.path.join(d, "A_%d.fastq" % k), os.path.join(sub, "A_%d.fastq" % k))
            subprocess.run(["bash", minicom, "-1", "A_1.fastq", "-2", "A_2.fastq", "-p", "-Q", "-G"] + flag, cwd=sub, check=True, stdout=subprocess.DEVNULL)
            res[tag + "_archive"] = os.path.getsize(os.path.join(sub, "A_comp_pe_order.minicom"))
            res[tag + "_decode"] = timed(["bash", minicom, "-d", "A_comp_pe_order.minicom", "-G"], repeats, cwd=sub)
            if tag == "with_names":
                ok &= all(filecmp.cmp(os.path.join(sub, "A_%d.fastq" % k), os.path.join(sub, "A_comp_pe_order_dec_%d.fastq" % k), shallow=False) for k in (1, 2))
        res["bytes_ok"] = bool(ok)
        line = json.dumps(res)
        print(line)
        if profile:
            write_profile(profile, "mate-archive", res)
        if out_path:
            with open(out_path, "w") as f:
                f.write(line + "\n")
        return 0 if ok else 1
    finally:
        shutil.rmtree(d, ignore_errors=True)


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
    ap.add_argument("--sizes", action="store_true"); ap.add_argument("--mate-sizes", action="store_true"); ap.add_argument("--mate", action="store_true"); ap.add_argument("--mate-archive", type=int, default=0); ap.add_argument("--profile", default=PROFILE); ap.add_argument("--records", default=None); ap.add_argument("--style", default="illumina")
    ap.add_argument("--gpu", action="store_true"); ap.add_argument("--skip-host", action="store_true"); ap.add_argument("--archive", type=int, default=0); ap.add_argument("--repeats", type=int, default=3); ap.add_argument("--dir", default=None); ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.sizes:
        doc = sizes([int(v) for v in (a.records or "3000,200000,2000000").split(",")])
        if a.out:
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1); f.write("\n")
        return 0
    if a.mate_sizes:
        doc = mate_sizes([int(v) for v in (a.records or "200000").split(",")])
        if a.out:
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1); f.write("\n")
        return 0
    if a.mate:
        return mate(int(a.records or 2000000), a.style, a.gpu, a.skip_host, a.repeats, a.dir, a.out, a.profile)
    if a.mate_archive:
        return mate_archive(a.mate_archive, a.repeats, a.dir, a.out, a.profile)
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
