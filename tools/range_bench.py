#!/usr/bin/env python3
"""Range-decode timing: records [first, first + count) of a -p archive on the GPU against the full decode of the
same build.

  python tools/range_bench.py --reads 20000000 --len 150 [--share 20] [--sets 1] [--dir DIR] [--repeats 3]

Builds a -p archive of synthetic reads on GPU 0 with tools/decode_bench.py's generator (minicom_amd.synth on the card, the Pipeline's
encoders), then times, on the unpacked stream files -- the step `minicom -d -G [-R]` runs behind the unpacking --

  * the range decoder (mcomh_decompress_order_range, device 0) for 1 / --share of the records at the front, the middle and the end,
  * the full decoder (mcomh_decompress_order_gpu),

each once to warm up (page cache included) and --repeats times measured: wall clock around calls that return with the output file closed,
the median and the spread (max - min).  Beside each, the split of the median run (mcomh_decompress_gpu_times): "decode_kernels_ms" is
taken by device events around the decode of phase B -- k_dc_reads for the full decode; k_dc_check_dest, k_dc_select and k_dc_reads_sel
for a range.  The three ranges are also checked against the slices of the full output.  One JSON line; exit status 1 when a slice differs
or a route fails; nothing is retried.  One process."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150, dest="L")
    ap.add_argument("--share", type=int, default=20, help="a range is 1 / SHARE of the records")
    ap.add_argument("--sets", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the archive and the outputs go (default: a temporary directory)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("range_bench: no GPU", file=sys.stderr)
        return 1
    import minicom_amd
    from minicom_amd import pipeline
    from minicom_amd.pipeline import Pipeline, decompress, decompress_range, decompress_gpu_times

    work = tempfile.mkdtemp(prefix="range_bench_", dir=a.dir)
    try:
        ctx = minicom_amd.Context(0)
        reads = ctx.synth_reads(4242, a.reads, a.L).cpu().numpy()          # made on the card (the host generator takes minutes at this size)
        p = Pipeline(reads, host_threads=8, stream_sets=a.sets)
        p.pre_process()
        arch = os.path.join(work, "archive"); os.mkdir(arch)
        p.cluster_dump(arch, order=True)
        p.close()
        del reads, p, ctx
        torch.cuda.empty_cache(); pipeline.pool_trim()
        count = max(1, a.reads // a.share)
        row = a.L + 1

        def timed(fn):
            fn()                                                         # warm-up
            runs, splits = [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                n = fn()
                runs.append((time.perf_counter() - t0) * 1e3)
                splits.append(decompress_gpu_times())
            mid = sorted(range(len(runs)), key=lambda i: runs[i])[len(runs) // 2]
            return {"ms": round(statistics.median(runs), 1), "spread_ms": round(max(runs) - min(runs), 1), "runs_ms": [round(x, 1) for x in runs],
                    "records": n, "split_ms": {k: round(v, 2) for k, v in splits[mid].items()}}

        full_path = os.path.join(work, "full.reads")
        res = {"reads": a.reads, "L": a.L, "sets": a.sets, "range_records": count,
               "stream_bytes": sum(os.path.getsize(os.path.join(arch, f)) for f in os.listdir(arch)),
               "full": timed(lambda: decompress(arch, full_path, order=True, device=0))}
        same = True
        for tag, first in (("front", 0), ("middle", (a.reads - count) // 2), ("end", a.reads - count)):
            out = os.path.join(work, tag + ".reads")
            res[tag] = timed(lambda: decompress_range(arch, out, first, count, device=0))
            res[tag]["first"] = first
            with open(full_path, "rb") as f:
                f.seek(first * row)
                same = same and f.read(count * row) == open(out, "rb").read()
            os.remove(out)
        res["same_output"] = same
        for tag in ("front", "middle", "end"):
            res[tag]["of_full"] = round(res[tag]["ms"] / res["full"]["ms"], 3)
            res[tag]["kernels_of_full"] = round(res[tag]["split_ms"]["decode_kernels_ms"] / max(res["full"]["split_ms"]["decode_kernels_ms"], 1e-9), 3)
        print(json.dumps(res))
        return 0 if same else 1
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
