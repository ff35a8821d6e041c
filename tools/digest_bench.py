"""Times of `minicom -K` and of the check behind `minicom -d`, on one GPU.

The digest pass: `mcomz e --fastq-digest --gpu` on a synthetic FASTQ of --reads x --L next to `mcomz e --fastq-names --gpu` on the same
file -- both are one pass through the same piece loop.  The two kernels alone: one run of the digest pass under `rocprofv3
--kernel-trace --stats`.  The decode with its check: `minicom -d -G` on the `-p -Q -N` archive of that file made with and without -K.
Medians of --repeats runs (wall clock around the child process), spread = max - min.  -> OUT (default profiles/r19_digest.txt); without
a GPU the file says "unmeasured on hardware".

    python tools/digest_bench.py [--reads 2000000] [--L 150] [--repeats 5] [--out FILE]
"""
import argparse
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "bin")


def synth_fastq(seed: int, n: int, L: int, path: str) -> int:
    """reads of the synthetic genome with Illumina-style names and qualities that fall towards the end; returns the bytes written"""
    import numpy as np
    from minicom_amd import synth
    total = 0
    all_reads = synth.synth_reads(seed, n, L)
    with open(path, "wb") as f:
        for first in range(0, n, 250000):
            m = min(250000, n - first)
            reads = all_reads[first:first + m]
            g = np.random.default_rng(seed + first)
            steps = g.choice(np.array([-2, -1, 0, 0, 0, 0, 1], dtype=np.int16), size=(m, L)) - (g.random((m, L)) < np.arange(L) / (4.0 * L))
            quals = (33 + np.clip(40 + np.cumsum(steps, axis=1), 2, 41)).astype(np.uint8)
            out = []
            for i in range(m):
                k = first + i
                out.append(b"@SIM:1:FC:1:%d:%d:%d 1:N:0:ACGT\n" % (1101 + k // 4000, 1000 + 7 * (k % 4000), 2000 + k) + reads[i].tobytes() + b"\n+\n" + quals[i].tobytes() + b"\n")
            blob = b"".join(out)
            f.write(blob)
            total += len(blob)
    return total


def timed(cmd, repeats, cwd, clean=()):
    ts = []
    for _ in range(repeats):
        for c in clean:
            for p in glob.glob(os.path.join(cwd, c)):
                os.remove(p)
        t0 = time.perf_counter()
        subprocess.run(cmd, cwd=cwd, check=True, stdout=subprocess.DEVNULL)
        ts.append((time.perf_counter() - t0) * 1e3)
    return "median %.1f ms, spread %.1f ms (%d runs)" % (statistics.median(ts), max(ts) - min(ts), repeats)


def kernels_alone(cmd, cwd):
    """per-kernel totals of one run under rocprofv3: lines for the two digest kernels, or why there are none"""
    d = os.path.join(cwd, "kt")
    try:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "kt", "--"] + cmd, cwd=cwd, check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL, timeout=300)
    except (OSError, subprocess.SubprocessError) as e:
        return ["  not collected: %s" % e]
    lines = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                if "k_fastq_record_hashes" in name or "k_digest_reduce" in name or "k_dc_line" in name or "line_index" in name:
                    lines.append("  %s: %s calls, total %.3f ms, average %.1f us" % (name.split("(")[0], row.get("Calls"), float(row.get("TotalDurationNs", 0)) / 1e6, float(row.get("AverageNs", 0)) / 1e3))
    shutil.rmtree(d, ignore_errors=True)
    return lines or ["  not collected: no kernel statistics were written"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--L", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_digest.txt"))
    a = ap.parse_args()
    import torch
    head = "tools/digest_bench.py --reads %d --L %d --repeats %d\n" % (a.reads, a.L, a.repeats)
    if not torch.cuda.is_available():
        with open(a.out, "w") as f:
            f.write(head + "unmeasured on hardware\n")
        return
    mcomz, minicom = os.path.join(BIN, "mcomz"), os.path.join(BIN, "minicom")
    lines = [head.rstrip("\n"), "device: " + torch.cuda.get_device_name(0)]
    with tempfile.TemporaryDirectory(dir=".") as td:
        td = os.path.abspath(td)
        size = synth_fastq(1900, a.reads, a.L, os.path.join(td, "X.fastq"))
        lines.append("input: %d records, %d bytes of FASTQ (plain)" % (a.reads, size))
        subprocess.run([mcomz, "e", "--fastq-digest", "--gpu", "X.fastq", "d.txt"], cwd=td, check=True, stdout=subprocess.DEVNULL)       # warm-up: page cache, code objects
        lines.append("the digest pass (whole process, one pass through the shared piece loop each):")
        lines.append("  mcomz e --fastq-digest --gpu: " + timed([mcomz, "e", "--fastq-digest", "--gpu", "X.fastq", "d.txt"], a.repeats, td))
        lines.append("  mcomz e --fastq-names --gpu:  " + timed([mcomz, "e", "--fastq-names", "--gpu", "X.fastq", "n.mcn"], a.repeats, td))
        lines.append("  mcomz e --fastq-digest (host twin): " + timed([mcomz, "e", "--fastq-digest", "X.fastq", "d.txt"], 1, td))
        lines.append("the kernels alone (one run of the digest pass under rocprofv3 --kernel-trace --stats):")
        lines += kernels_alone([mcomz, "e", "--fastq-digest", "--gpu", "X.fastq", "d.txt"], td)
        for tag, flags in (("with", ["-K"]), ("without", [])):
            d = os.path.join(td, tag)
            os.mkdir(d)
            os.link(os.path.join(td, "X.fastq"), os.path.join(d, "X.fastq"))
            t0 = time.perf_counter()
            subprocess.run([minicom, "-r", "X.fastq", "-p", "-Q", "-N", "-G"] + flags, cwd=d, check=True, stdout=subprocess.DEVNULL)
            lines.append("minicom -r X.fastq -p -Q -N -G %s: %.1f s (one run), archive %d bytes" % (" ".join(flags) or "  ", time.perf_counter() - t0, os.path.getsize(os.path.join(d, "X_comp_order.minicom"))))
        lines.append("the decode with its check (minicom -d X_comp_order.minicom -G, the output file removed between runs):")
        for tag in ("with", "without"):
            d = os.path.join(td, tag)
            subprocess.run([minicom, "-d", "X_comp_order.minicom", "-G"], cwd=d, check=True, stdout=subprocess.DEVNULL)
            lines.append("  %s digest.txt: " % tag + timed([minicom, "-d", "X_comp_order.minicom", "-G"], a.repeats, d, clean=("X_comp_order_dec.fastq",)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
