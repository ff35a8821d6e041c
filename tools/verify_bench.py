#!/usr/bin/env python3
"""Verifier timing: archive + FASTQ -> verdict on the GPU (mcomh_verify_gpu), against the GPU decode-to-file route of the same archive.

  python tools/verify_bench.py --reads 20000000 --len 150 --mode default|order|paired [--sets 1] [--dir DIR] [--repeats 3]

Builds an archive of synthetic reads on GPU 0 as tools/decode_bench.py does and writes the same reads as FASTQ file(s); then runs each route
once to warm up (page cache included) and `--repeats` times measured, wall clock around calls that return with the answer (the files closed).
One JSON line: both medians and spreads (max - min), the verify call's split of its median run (ingest, upload + indices, decode, compare, the
compare by device events) and the compare's bytes per second against its byte model (both tables read by the hash and
again by the compare, eight sort passes that read and write 16 bytes per record).  Exit status 1 when the verdict is not "identical" or a
route fails; nothing is retried.  One process."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_fastq(path, reads):
    """four-line records of fixed width, a million reads at a time"""
    n, L = reads.shape
    w = 11 + (L + 1) + 2 + (L + 1)
    with open(path, "wb") as f:
        for lo in range(0, n, 1 << 20):
            hi = min(n, lo + (1 << 20))
            rec = np.empty((hi - lo, w), dtype=np.uint8)
            rec[:, 0] = ord("@")
            ids = np.arange(lo, hi, dtype=np.int64)
            for d in range(9):
                rec[:, 9 - d] = 48 + (ids // 10 ** d) % 10
            rec[:, 10] = 10
            rec[:, 11:11 + L] = reads[lo:hi]
            rec[:, 11 + L] = 10
            rec[:, 12 + L] = ord("+"); rec[:, 13 + L] = 10
            rec[:, 14 + L:14 + 2 * L] = ord("I")
            rec[:, 14 + 2 * L] = 10
            f.write(rec.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150, dest="L")
    ap.add_argument("--mode", choices=["default", "order", "paired"], default="default")
    ap.add_argument("--sets", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the archive, the FASTQ and the outputs go (default: a temporary directory)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("verify_bench: no GPU", file=sys.stderr)
        return 1
    import minicom_amd
    from minicom_amd import pipeline
    from minicom_amd.pipeline import Pipeline, decompress, decompress_pe, decompress_gpu_times, verify

    work = tempfile.mkdtemp(prefix="verify_bench_", dir=a.dir)
    try:
        ctx = minicom_amd.Context(0)
        reads = ctx.synth_reads(4242, a.reads, a.L).cpu().numpy()
        p = Pipeline(reads, host_threads=8, stream_sets=a.sets)
        p.pre_process()
        arch = os.path.join(work, "archive"); os.mkdir(arch)
        p.cluster_dump(arch, order=a.mode == "order", paired=a.mode == "paired")
        p.close()
        n = reads.shape[0]
        fq = [os.path.join(work, "in_1.fastq")] + ([os.path.join(work, "in_2.fastq")] if a.mode == "paired" else [])
        if a.mode == "paired":
            write_fastq(fq[0], reads[:n // 2]); write_fastq(fq[1], reads[n // 2:2 * (n // 2)])
        else:
            write_fastq(fq[0], reads)
        del reads, p, ctx
        torch.cuda.empty_cache(); pipeline.pool_trim()
        res = {"reads": a.reads, "L": a.L, "mode": a.mode, "sets": a.sets, "fastq_bytes": sum(os.path.getsize(f) for f in fq),
               "stream_bytes": sum(os.path.getsize(os.path.join(arch, f)) for f in os.listdir(arch))}

        def decode():
            outs = [os.path.join(work, "out.1")] + ([os.path.join(work, "out.2")] if a.mode == "paired" else [])
            t0 = time.perf_counter()
            if a.mode == "paired":
                decompress_pe(arch, *outs, device=0)
            else:
                decompress(arch, outs[0], order=a.mode == "order", device=0)
            return (time.perf_counter() - t0) * 1e3, decompress_gpu_times()

        def check():
            t0 = time.perf_counter()
            r = verify(arch, fq[0], fq[1] if a.mode == "paired" else None, order=a.mode == "order", device=0)
            return (time.perf_counter() - t0) * 1e3, r

        for tag, route in (("decode_to_file", decode), ("verify", check)):
            route()                                                       # warm-up
            runs = [route() for _ in range(a.repeats)]
            ms = [r[0] for r in runs]
            mid = sorted(range(len(ms)), key=lambda i: ms[i])[len(ms) // 2]
            res[tag + "_ms"] = round(statistics.median(ms), 1)
            res[tag + "_spread_ms"] = round(max(ms) - min(ms), 1)
            res[tag + "_runs_ms"] = [round(x, 1) for x in ms]
            if tag == "verify":
                r = runs[mid][1]
                res["verify_split_ms"] = {k: round(v, 1) for k, v in r["times_ms"].items()}
                res["identical"] = all(x[1]["identical"] for x in runs)
                res["ingest_share"] = round(r["times_ms"]["ingest"] / r["times_ms"]["total"], 3)
                units = r["n_input"] + r["n_archive"]
                rows = (2 if a.mode == "paired" else 1) * (r["n_input"] * a.L + r["n_archive"] * (a.L + 1))
                model = rows if a.mode == "order" else 2 * rows + 8 * 2 * 16 * units
                res["compare_model_bytes"] = model
                res["compare_gb_per_s"] = round(model / (r["times_ms"]["compare_device"] * 1e-3) / 1e9, 1)
            else:
                res["decode_split_ms"] = {k: round(v, 1) for k, v in runs[mid][1].items()}
        res["verify_over_decode"] = round(res["verify_ms"] / res["decode_to_file_ms"], 2)
        print(json.dumps(res))
        return 0 if res["identical"] else 1
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
