"""Sizes and times of `minicom -p -V`.

Sizes (CPU, through the host twins): synthetic FASTQ with 0 %, 1 %, 10 % and 50 % of the reads trimmed; per share the packed size of
len.bin, odd.seq and odd.qual (the container's rANS stage) against `xz -6` of the same bytes, and qual.mcq + packed odd.qual against
`xz -6` of all quality lines.  -> profiles/r17_ragged_sizes.json
Times (only with a GPU): 2 M x 150 bp with 10 % trimmed; each of the four passes and `minicom -d -G`, against the same steps on the same
file with the odd records removed and no -V (the path without this feature: the baseline).  Medians of --repeats runs, spread = max - min.
-> profiles/r17_ragged.txt; without a GPU the file says "unmeasured on hardware".

    python tools/ragged_bench.py [--reads 20000] [--time-reads 2000000] [--repeats 3] [--no-times]
"""
import argparse
import json
import lzma
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "bin")


def synth_fastq(seed: int, n: int, L: int, share: float) -> bytes:
    """reads of the synthetic genome, a `share` of them trimmed at the 3' end to 30 .. L - 1 bases; qualities that fall towards the end"""
    import numpy as np
    from minicom_amd import synth
    reads = synth.synth_reads(seed, n, L)
    g = np.random.default_rng(seed)
    steps = g.choice(np.array([-2, -1, 0, 0, 0, 0, 1], dtype=np.int16), size=(n, L)) - (g.random((n, L)) < np.arange(L) / (4.0 * L))
    quals = (33 + np.clip(40 + np.cumsum(steps, axis=1), 2, 41)).astype(np.uint8)
    rng = random.Random(seed)
    out = []
    for i in range(n):
        l = rng.randrange(30, L) if rng.random() < share else L
        out.append(b"@SIM:1:FC:1:%d:%d:%d 1:N:0:ACGT\n" % (1101 + i // 4000, 1000 + 7 * (i % 4000), 2000 + i) + reads[i, :l].tobytes() + b"\n+\n" + quals[i, :l].tobytes() + b"\n")
    return b"".join(out)


def sizes(n: int, L: int) -> dict:
    from minicom_amd import pipeline
    rows = []
    with tempfile.TemporaryDirectory() as td:
        for share in (0.0, 0.01, 0.10, 0.50):
            text = synth_fastq(1700 + int(share * 100), n, L, share)
            fq = os.path.join(td, "in.fastq")
            with open(fq, "wb") as f:
                f.write(text)
            t = lambda name: os.path.join(td, name)
            nrec, modal, n_odd = pipeline.fastq_lengths(fq, t("len.bin"))
            pipeline.fastq_ragged_files(fq, 1, modal, t("len.bin"), t("rows"), t("odd.seq"))
            pipeline.fastq_quality_member_ragged(fq, modal, t("len.bin"), t("qual.mcq"), t("odd.qual"))
            row = {"share_trimmed": share, "records": nrec, "L": modal, "n_odd": n_odd, "fastq_bytes": len(text)}
            for name in ("len.bin", "odd.seq", "odd.qual"):
                data = open(t(name), "rb").read()
                row[name] = {"raw": len(data), "rans": len(pipeline.rans_encode(data)) if n_odd else 0, "xz6": len(lzma.compress(data, preset=6)) if n_odd else 0}
            all_quals = b"".join(text.split(b"\n")[3::4])
            row["quality"] = {"qual.mcq": os.path.getsize(t("qual.mcq")), "qual.mcq+odd.qual.rans": os.path.getsize(t("qual.mcq")) + row["odd.qual"]["rans"],
                              "xz6_of_all_quality_lines": len(lzma.compress(all_quals, preset=6)), "quality_bytes": len(all_quals)}
            rows.append(row)
    return {"tool": "tools/ragged_bench.py", "reads": n, "L": L, "where": "CPU, host twins (device = -1)", "rows": rows}


def timed(cmd, repeats, cwd):
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        subprocess.run(cmd, cwd=cwd, check=True, stdout=subprocess.DEVNULL)
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 1), "spread_ms": round(max(ts) - min(ts), 1)}


def times(n: int, L: int, repeats: int) -> dict:
    """each pass as `bin/minicom -V` runs it, then the whole script both ways, then -d -G"""
    out = {}
    with tempfile.TemporaryDirectory(dir=".") as td:
        text = synth_fastq(1710, n, L, 0.10)
        recs = text.split(b"\n")
        even = b"".join(b"\n".join(recs[k:k + 4]) + b"\n" for k in range(0, len(recs) - 1, 4) if len(recs[k + 1]) == L)
        for tag, data in (("ragged", text), ("baseline", even)):
            d = os.path.join(td, tag)
            os.mkdir(d)
            with open(os.path.join(d, "X.fastq"), "wb") as f:
                f.write(data)
        r, b = os.path.join(td, "ragged"), os.path.join(td, "baseline")
        mcomz, sg = os.path.join(BIN, "mcomz"), os.path.join(BIN, "minicomsg")
        for d in (r, b):
            os.mkdir(os.path.join(d, "s"))
        out["lengths"] = {"ragged": timed([mcomz, "e", "--fastq-lengths", "--gpu", "X.fastq", "len.bin"], repeats, r), "baseline": None}
        out["core"] = {"ragged": timed([sg, "X.fastq", "s", "-p", "-V", str(L), "len.bin"], repeats, r), "baseline": timed([sg, "X.fastq", "s", "-p"], repeats, b)}
        out["quality"] = {"ragged": timed([mcomz, "e", "--fastq-qual", str(L), "--ragged", "len.bin", "--gpu", "X.fastq", "q.mcq", "odd.qual"], repeats, r),
                          "baseline": timed([mcomz, "e", "--fastq-qual", str(L), "--gpu", "X.fastq", "q.mcq"], repeats, b)}
        out["names"] = {"ragged": timed([mcomz, "e", "--fastq-names", "--gpu", "X.fastq", "n.mcn"], repeats, r), "baseline": timed([mcomz, "e", "--fastq-names", "--gpu", "X.fastq", "n.mcn"], repeats, b)}
        minicom = os.path.join(BIN, "minicom")
        subprocess.run([minicom, "-r", "X.fastq", "-p", "-V", "-Q", "-N", "-G"], cwd=r, check=True, stdout=subprocess.DEVNULL)
        subprocess.run([minicom, "-r", "X.fastq", "-p", "-Q", "-N", "-G"], cwd=b, check=True, stdout=subprocess.DEVNULL)
        out["minicom -d -G"] = {"ragged": timed([minicom, "-d", "X_comp_order.minicom", "-G"], repeats, r), "baseline": timed([minicom, "-d", "X_comp_order.minicom", "-G"], repeats, b)}
        out["archive_bytes"] = {"ragged": os.path.getsize(os.path.join(r, "X_comp_order.minicom")), "baseline": os.path.getsize(os.path.join(b, "X_comp_order.minicom"))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--L", type=int, default=100)
    ap.add_argument("--time-reads", type=int, default=2000000)
    ap.add_argument("--time-L", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-times", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    s = sizes(a.reads, a.L)
    with open(os.path.join(a.out_dir, "r17_ragged_sizes.json"), "w") as f:
        json.dump(s, f, indent=1)
        f.write("\n")
    import torch
    lines = ["minicom -p -V (DESIGN.md section 3.16): tools/ragged_bench.py", ""]
    if a.no_times or not torch.cuda.is_available():
        lines += ["times of the four passes and of minicom -d -G at %d x %d bp, 10 %% trimmed, against the same file without its odd records and without -V:" % (a.time_reads, a.time_L),
                  "unmeasured on hardware"]
    else:
        t = times(a.time_reads, a.time_L, a.repeats)
        lines.append("%d x %d bp, 10 %% trimmed; medians of %d runs in ms (spread = max - min); baseline = the same file without its odd records, no -V" % (a.time_reads, a.time_L, a.repeats))
        for k, v in t.items():
            lines.append("%-16s %s" % (k, json.dumps(v)))
    with open(os.path.join(a.out_dir, "r17_ragged.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"sizes": os.path.join(a.out_dir, "r17_ragged_sizes.json"), "times": os.path.join(a.out_dir, "r17_ragged.txt")}))


if __name__ == "__main__":
    main()
