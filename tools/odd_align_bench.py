"""Sizes and times of `minicom -p -V -A`.

golden_cpu (no GPU): the golden -p stream files of tests/golden (2 015 reads of 150 bases) with a share of the decoded reads added again,
trimmed at the 3' end to 31 .. 149 bases, as odd records; odd.aln and the residual by the host twins alone.  Reproducible anywhere.
synthetic_gpu (needs a GPU; without one the rows already in the file are kept): synthetic FASTQ of tools/ragged_bench.py (reads of one genome, a share of them trimmed at the 3' end) through the core on GPU 0, then the
odd reads against the contigs just dumped -- by the host twins (device -1) and by the kernels of csrc/odd_align.hip, whose files must be
equal.  Per share: n_odd, n_aligned, the bytes of odd.seq as -V stores it and of odd.aln + the residual odd.seq, each raw and through the
container's rANS stage (host twin).  -> profiles/r21_odd_align_sizes.json
Times: the folder call on either route, median of --repeats runs and spread = max - min.  -> profiles/r21_odd_align.txt
The contigs of synthetic_gpu come from the core, so that part needs a GPU; no time is a pass / fail condition.

    python tools/odd_align_bench.py [--reads 20000] [--L 100] [--repeats 3] [--out-dir profiles]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stream_folder(fq: str, td: str):
    """the ungrouped stream files of `minicom -p -V` in td: len.bin, odd.seq and what the core dumps"""
    from minicom_amd.pipeline import Pipeline, fastq_lengths
    len_path = os.path.join(td, "len.bin")
    n, L, n_odd = fastq_lengths(fq, len_path, device=0)
    p = Pipeline.from_fastq_ragged(fq, L, len_path, os.path.join(td, "odd.seq"), device=0)
    try:
        p.pre_process()
        p.cluster_dump(td, order=True, paired=False)
    finally:
        p.close()
    return n, L, n_odd


def one_share(n: int, L: int, share: float, repeats: int) -> dict:
    from minicom_amd import pipeline
    from tools.ragged_bench import synth_fastq
    with tempfile.TemporaryDirectory(dir=".") as top:
        fq = os.path.join(top, "in.fastq")
        with open(fq, "wb") as f:
            f.write(synth_fastq(2100 + int(share * 100), n, L, share))
        base = os.path.join(top, "streams")
        os.mkdir(base)
        nrec, modal, n_odd = stream_folder(fq, base)
        full = open(os.path.join(base, "odd.seq"), "rb").read()
        row = {"share_trimmed": share, "records": nrec, "L": modal, "n_odd": n_odd, "ref_bytes": sum(os.path.getsize(os.path.join(base, f)) for f in os.listdir(base) if f.startswith("ref.bin."))}
        files, ms = {}, {"host": [], "gpu": []}
        for route, device in (("host", None), ("gpu", 0)):
            for k in range(repeats):
                d = os.path.join(top, "%s%d" % (route, k))
                shutil.copytree(base, d)
                t0 = time.perf_counter()
                counts = pipeline.odd_align_folder(d, device=device)
                ms[route].append((time.perf_counter() - t0) * 1e3)
                files[route] = (counts, open(os.path.join(d, "odd.aln"), "rb").read() if counts[1] else b"", open(os.path.join(d, "odd.seq"), "rb").read())
                shutil.rmtree(d)
        assert files["host"] == files["gpu"], "the GPU route and the host twins disagree"
        (n_odd2, n_aligned, res_bytes), member, residual = files["gpu"]
        enc = lambda b: len(pipeline.rans_encode(b)) if b else 0
        row.update({"n_aligned": n_aligned, "n_mismatch": int.from_bytes(member[48:56], "little") if member else 0,
                    "odd.seq of -V": {"raw": len(full), "rans": enc(full)},
                    "odd.aln": {"raw": len(member), "rans": enc(member)}, "residual odd.seq": {"raw": len(residual), "rans": enc(residual)}})
        row["rans of -V -A over rans of -V"] = round((row["odd.aln"]["rans"] + row["residual odd.seq"]["rans"]) / max(row["odd.seq of -V"]["rans"], 1), 4)
        row["times_ms"] = {r: {"median": round(statistics.median(v), 1), "spread": round(max(v) - min(v), 1)} for r, v in ms.items()}
        return row


def golden_share(share: float) -> dict:
    """the golden -p stream files with trimmed copies of a share of their reads as odd records, through the host twins"""
    import gzip
    import io
    import random
    import tarfile
    from minicom_amd import pipeline
    golden = os.path.join(ROOT, "tests", "golden")
    with tempfile.TemporaryDirectory() as d:
        with gzip.open(os.path.join(golden, "streams_order_stages_L150.tar.gz"), "rb") as g:
            tarfile.open(fileobj=io.BytesIO(g.read())).extractall(d)
        with gzip.open(os.path.join(golden, "stages_L150.reads.gz"), "rb") as f:
            rows = f.read().split(b"\n")[:-1]
        rng = random.Random(2100 + int(share * 100))
        lens, odd = bytearray(), []
        for row in rows:                                      # an odd record in front of the read it is a trimmed copy of
            if rng.random() < share:
                odd.append(row[:rng.randrange(31, 150)])
                lens.append(len(odd[-1]) - 1)
            lens.append(149)
        full = b"".join(odd)
        open(os.path.join(d, "len.bin"), "wb").write(bytes(lens))
        open(os.path.join(d, "odd.seq"), "wb").write(full)
        n_odd, n_aligned, res_bytes = pipeline.odd_align_folder(d)
        member = open(os.path.join(d, "odd.aln"), "rb").read() if n_aligned else b""
        residual = open(os.path.join(d, "odd.seq"), "rb").read()
        enc = lambda b: len(pipeline.rans_encode(b)) if b else 0
        row = {"share_trimmed": share, "records": len(lens), "L": 150, "n_odd": n_odd, "n_aligned": n_aligned, "ref_bytes": os.path.getsize(os.path.join(d, "ref.bin.0")),
               "odd.seq of -V": {"raw": len(full), "rans": enc(full)}, "odd.aln": {"raw": len(member), "rans": enc(member)},
               "residual odd.seq": {"raw": len(residual), "rans": enc(residual)}}
        row["rans of -V -A over rans of -V"] = round((row["odd.aln"]["rans"] + row["residual odd.seq"]["rans"]) / max(row["odd.seq of -V"]["rans"], 1), 4)
        return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--L", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    os.makedirs(a.out_dir, exist_ok=True)
    sizes_path = os.path.join(a.out_dir, "r21_odd_align_sizes.json")
    sizes = {"tool": "tools/odd_align_bench.py",
             "golden_cpu": {"where": "CPU, host twins (device = -1) over tests/golden/streams_order_stages_L150.tar.gz", "rows": [golden_share(sh) for sh in (0.10, 0.30, 0.50)]}}
    rows = []
    if torch.cuda.is_available():
        rows = [one_share(a.reads, a.L, share, a.repeats) for share in (0.10, 0.30, 0.50)]
        sizes["synthetic_gpu"] = {"reads": a.reads, "L": a.L, "where": "core on GPU 0; odd.aln by the host twins and by the kernels, equal bytes",
                                  "rows": [{k: v for k, v in r.items() if k != "times_ms"} for r in rows]}
    elif os.path.exists(sizes_path):
        kept = json.load(open(sizes_path))
        if "synthetic_gpu" in kept:
            sizes["synthetic_gpu"] = kept["synthetic_gpu"]
    with open(sizes_path, "w") as f:
        json.dump(sizes, f, indent=1)
        f.write("\n")
    print(json.dumps(sizes, indent=1))
    if not rows:
        return
    with open(os.path.join(a.out_dir, "r21_odd_align.txt"), "w") as f:
        f.write("tools/odd_align_bench.py --reads %d --L %d --repeats %d: mcomh_odd_align_folder, whole call (files read, index, search, member, files written)\n" % (a.reads, a.L, a.repeats))
        f.write("the GPU route includes creating a context; a few thousand odd reads do not fill the card: these are latencies of a small job, not throughput\n")
        for r in rows:
            t = r["times_ms"]
            f.write("share %.2f  n_odd %6d  aligned %6d  host twins %8.1f ms (spread %.1f)  GPU %8.1f ms (spread %.1f)\n" %
                    (r["share_trimmed"], r["n_odd"], r["n_aligned"], t["host"]["median"], t["host"]["spread"], t["gpu"]["median"], t["gpu"]["spread"]))


if __name__ == "__main__":
    main()
