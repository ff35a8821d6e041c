#!/usr/bin/env python3
"""Decoder timing, stream files -> finished output file(s): the host route (mcomh_decompress*) against the GPU route (mcomh_decompress*_gpu).

  python tools/decode_bench.py --reads 20000000 --len 150 --mode default|order|paired [--sets 1] [--dir DIR] [--repeats 3]

Builds an archive of synthetic reads on GPU 0 (minicom_amd.synth, the Pipeline's encoders), then runs each route once to warm up (page cache
included) and `--repeats` times measured: wall clock around calls that return with the output files closed.  One JSON line: both medians and
spreads (max - min), the GPU route's split of its median run (mcomh_decompress_gpu_times) and the md5 of both routes' outputs.  Exit status 1
when the outputs differ or a route fails; nothing is retried.  One process."""
import argparse
import hashlib
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def md5_of(paths):
    out = []
    for p in paths:
        h = hashlib.md5()
        with open(p, "rb") as f:
            for blk in iter(lambda: f.read(1 << 24), b""):
                h.update(blk)
        out.append(h.hexdigest())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150, dest="L")
    ap.add_argument("--mode", choices=["default", "order", "paired"], default="default")
    ap.add_argument("--sets", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the archive and the outputs go (default: a temporary directory)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("decode_bench: no GPU", file=sys.stderr)
        return 1
    import minicom_amd
    from minicom_amd import pipeline
    from minicom_amd.pipeline import Pipeline, decompress, decompress_pe, decompress_gpu_times

    work = tempfile.mkdtemp(prefix="decode_bench_", dir=a.dir)
    try:
        ctx = minicom_amd.Context(0)
        reads = ctx.synth_reads(4242, a.reads, a.L).cpu().numpy()          # made on the card (the host generator takes minutes at this size)
        p = Pipeline(reads, host_threads=8, stream_sets=a.sets)
        p.pre_process()
        arch = os.path.join(work, "archive"); os.mkdir(arch)
        p.cluster_dump(arch, order=a.mode == "order", paired=a.mode == "paired")
        p.close()
        del reads, p, ctx
        torch.cuda.empty_cache(); pipeline.pool_trim()
        stream_bytes = sum(os.path.getsize(os.path.join(arch, f)) for f in os.listdir(arch))

        def route(device, tag):
            outs = [os.path.join(work, tag + ".1")] + ([os.path.join(work, tag + ".2")] if a.mode == "paired" else [])
            t0 = time.perf_counter()
            n = decompress_pe(arch, *outs, device=device) if a.mode == "paired" else decompress(arch, outs[0], order=a.mode == "order", device=device)
            return (time.perf_counter() - t0) * 1e3, n, outs

        res = {"reads": a.reads, "L": a.L, "mode": a.mode, "sets": a.sets, "stream_bytes": stream_bytes}
        for device, tag in ((None, "host"), (0, "gpu")):
            route(device, tag)                                           # warm-up
            runs, splits = [], []
            for _ in range(a.repeats):
                ms, n, outs = route(device, tag)
                runs.append(ms)
                if device is not None:
                    splits.append(decompress_gpu_times())
            res[tag + "_ms"] = round(statistics.median(runs), 1)
            res[tag + "_spread_ms"] = round(max(runs) - min(runs), 1)
            res[tag + "_runs_ms"] = [round(x, 1) for x in runs]
            res[tag + "_md5"] = md5_of(outs)
            res["n_out"] = n
            if device is not None:
                mid = sorted(range(len(runs)), key=lambda i: runs[i])[len(runs) // 2]
                res["gpu_split_ms"] = {k: round(v, 1) for k, v in splits[mid].items()}
                res["output_bytes"] = sum(os.path.getsize(o) for o in outs)
        res["speedup"] = round(res["host_ms"] / res["gpu_ms"], 2)
        res["same_output"] = res["host_md5"] == res["gpu_md5"]
        print(json.dumps(res))
        return 0 if res["same_output"] else 1
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
