#!/usr/bin/env python3
"""BGZF output timing.

  python tools/bgzf_bench.py [--kernel-bytes 1073741824] [--reads 20000000] [--len 150] [--repeats 3] [--dir DIR]

Two measurements, one JSON line:
  kernel   mcom_bgzf_encode alone over --kernel-bytes of synthetic FASTQ on the card (a 4 MB text of tests/bgzf_cases.synthetic_fastq,
           tiled: blocks of 65280 bytes never see the tiling): GB/s of input, median of --repeats after one warm-up, and the coded size
  decode   the GPU decoder of a default-mode archive of --reads reads (built as tools/decode_bench.py builds it) to a plain file and to a
           `.gz` file, same build, same archive: medians, spreads, the phase times of mcomh_decompress_gpu_times for the median run, both
           output sizes; the .gz file is read back through gzip and compared with the plain one by md5
Exit status 1 when the two outputs differ; nothing is retried.  One process."""
import argparse
import hashlib
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def md5_plain(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def md5_gz(path):
    h = hashlib.md5()
    d = zlib.decompressobj(31)
    with open(path, "rb") as f:
        buf = b""
        while True:
            blk = f.read(1 << 24)
            buf += blk
            while buf:
                h.update(d.decompress(buf))
                if not d.eof:
                    buf = b""
                    break
                buf = d.unused_data
                d = zlib.decompressobj(31)
            if not blk:
                break
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-bytes", type=int, default=1 << 30)
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--len", type=int, default=150, dest="L")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("bgzf_bench: no GPU", file=sys.stderr)
        return 1
    import minicom_amd
    from minicom_amd import pipeline
    from minicom_amd.pipeline import Pipeline, decompress, decompress_gpu_times
    import bgzf_cases as BC

    res = {}
    ctx = minicom_amd.Context(0)
    if a.kernel_bytes:
        text = torch.from_numpy(np.frombuffer(BC.synthetic_fastq(51, 15000), dtype=np.uint8).copy()).cuda()
        raw = text.repeat((a.kernel_bytes + text.numel() - 1) // text.numel())[:a.kernel_bytes].contiguous()
        out = torch.empty(int(ctx.lib.mcom_bgzf_bound(a.kernel_bytes)), dtype=torch.uint8, device="cuda:0")
        coded = ctx.bgzf_encode(raw, out=out).numel()                      # warm-up
        runs = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.bgzf_encode(raw, out=out)
            runs.append((time.perf_counter() - t0) * 1e3)
        ms = statistics.median(runs)
        res["kernel"] = {"bytes": a.kernel_bytes, "coded_bytes": coded, "ms": round(ms, 2), "spread_ms": round(max(runs) - min(runs), 2),
                         "runs_ms": [round(x, 2) for x in runs], "GBps_in": round(a.kernel_bytes / ms / 1e6, 2)}
        del raw, out, text
        torch.cuda.empty_cache()
    same = True
    if a.reads:
        work = tempfile.mkdtemp(prefix="bgzf_bench_", dir=a.dir)
        try:
            reads = ctx.synth_reads(4242, a.reads, a.L).cpu().numpy()
            p = Pipeline(reads, host_threads=8)
            p.pre_process()
            arch = os.path.join(work, "archive"); os.mkdir(arch)
            p.cluster_dump(arch)
            p.close()
            del reads, p
            torch.cuda.empty_cache(); pipeline.pool_trim()
            dec = {"reads": a.reads, "L": a.L}
            for tag, name in (("plain", "out.reads"), ("gz", "out.reads.gz")):
                path = os.path.join(work, name)
                run = lambda: (time.perf_counter(), decompress(arch, path, device=0), time.perf_counter())
                run()                                                      # warm-up
                runs, splits = [], []
                for _ in range(a.repeats):
                    t0, _, t1 = run()
                    runs.append((t1 - t0) * 1e3); splits.append(decompress_gpu_times())
                mid = sorted(range(len(runs)), key=lambda i: runs[i])[len(runs) // 2]
                dec[tag] = {"ms": round(statistics.median(runs), 1), "spread_ms": round(max(runs) - min(runs), 1), "runs_ms": [round(x, 1) for x in runs],
                            "split_ms": {k: round(v, 1) for k, v in splits[mid].items()}, "output_bytes": os.path.getsize(path)}
            dec["md5_plain"] = md5_plain(os.path.join(work, "out.reads")); dec["md5_gz_inflated"] = md5_gz(os.path.join(work, "out.reads.gz"))
            same = dec["md5_plain"] == dec["md5_gz_inflated"]
            dec["same_text"] = same
            dec["gz_over_plain_time"] = round(dec["gz"]["ms"] / dec["plain"]["ms"], 3)
            res["decode"] = dec
        finally:
            shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(res))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
