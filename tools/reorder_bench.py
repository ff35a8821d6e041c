#!/usr/bin/env python3
"""What `minicom -q` costs and saves against `minicom -p -Q`, on GPU 0, on one synthetic FASTQ file.

  python tools/reorder_bench.py --rows 2000000 --len 150 [--repeats 3] [--dir DIR] [--out FILE] [--sizes-out FILE]

The reads are minicom_amd.synth.synth_reads, the qualities the generator of tools/qual_bench.py.  Reported as one JSON line:
  sizes    the members of the `-q` archive and of the `-p -Q` archive of the same file (codec rans): the saving is idsbin
  member   wall ms of `mcomz e --fastq-qual L --gpu IN OUT` with and without `--order FILE`, one warm-up and --repeats measured runs
           each: median and spread (max - min); the two members hold the same rows in another order
  gather   mcom_qual_gather_rows alone on the resident matrix, by device events: median ms of --repeats launches after a warm-up, and
           the bytes per second against its byte model 2 n L + 4 n
Nothing is retried; exit status 1 when a step fails."""
import argparse
import contextlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
MCOMZ = os.path.join(ROOT, "bin", "mcomz")


def write_fastq(path, reads, quals):
    """records `@<i+1>`, read, `+`, qualities, written in blocks of equal name width"""
    n, L = reads.shape
    with open(path, "wb") as f:
        lo = 0
        while lo < n:
            digits = len(str(lo + 1))
            hi = min(n, 10 ** digits - 1)
            for a in range(lo, hi, 1 << 19):
                b = min(hi, a + (1 << 19))
                m = b - a
                rec = np.empty((m, 2 * L + 6 + digits), dtype=np.uint8)
                rec[:, 0] = ord("@")
                v = np.arange(a + 1, b + 1)
                for k in range(digits - 1, -1, -1):
                    rec[:, 1 + k] = 48 + v % 10; v //= 10
                at = 1 + digits
                rec[:, at] = 10; rec[:, at + 1:at + 1 + L] = reads[a:b]; at += 1 + L
                rec[:, at] = 10; rec[:, at + 1] = ord("+"); rec[:, at + 2] = 10; rec[:, at + 3:at + 3 + L] = quals[a:b]; rec[:, at + 3 + L] = 10
                rec.tofile(f)
            lo = hi


def timed(cmd):
    t0 = time.perf_counter()
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    ms = (time.perf_counter() - t0) * 1e3
    if p.returncode:
        raise RuntimeError("%s failed: %s" % (" ".join(cmd), p.stderr.decode(errors="replace")[-500:]))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--len", type=int, default=150, dest="L")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes-out", default=None)
    ap.add_argument("--keep", action="store_true", help="leave the FASTQ file and the order file in --dir (for a profiler run of the member step)")
    a = ap.parse_args()
    import torch
    from minicom_amd import Context, container, synth
    from minicom_amd.pipeline import Pipeline
    from qual_bench import synth_quals
    n, L = a.rows, a.L
    if a.keep and not a.dir:
        ap.error("--keep needs --dir")
    where = contextlib.nullcontext(a.dir) if a.keep else tempfile.TemporaryDirectory(dir=a.dir)
    with where as td:
        reads = synth.synth_reads(1002, n, L)
        quals = synth_quals(7, n, L)
        fq = os.path.join(td, "in.fastq")
        write_fastq(fq, reads, quals)
        res = {"rows": n, "L": L, "repeats": a.repeats, "fastq_bytes": os.path.getsize(fq)}
        # sizes of the two archives
        q = container.compress_fastq(fq, os.path.join(td, "q.minicom"), codec="rans", device=0, quality_reordered=True)
        pq = container.compress_fastq(fq, os.path.join(td, "pq.minicom"), codec="rans", device=0, order=True, quality=True)
        res["sizes"] = {"-q": {k: v for k, v in q.items() if k != "n_reads"}, "-p -Q": {k: v for k, v in pq.items() if k != "n_reads"},
                        "total -q": sum(v for k, v in q.items() if k != "n_reads"), "total -p -Q": sum(v for k, v in pq.items() if k != "n_reads")}
        res["sizes"]["saving"] = res["sizes"]["total -p -Q"] - res["sizes"]["total -q"]
        # the order file of this input
        dump = os.path.join(td, "dump"); os.makedirs(dump, exist_ok=True)
        p = Pipeline.from_fastq(fq, device=0)
        try:
            p.pre_process(); p.keep_read_order(True); p.cluster_dump(dump)
        finally:
            p.close()
        order_path = os.path.join(td, "read_order.bin")
        os.replace(os.path.join(dump, "read_order.bin"), order_path)
        # the member step, with and without the order
        plain = [MCOMZ, "e", "--fastq-qual", str(L), "--gpu", fq, os.path.join(td, "plain.mcq")]
        ordered = [MCOMZ, "e", "--fastq-qual", str(L), "--order", order_path, "--gpu", fq, os.path.join(td, "ordered.mcq")]
        res["member"] = {}
        for name, cmd in (("plain", plain), ("ordered", ordered)):
            timed(cmd)
            ms = [timed(cmd) for _ in range(a.repeats)]
            res["member"][name] = {"median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms), "bytes": os.path.getsize(cmd[-1])}
        # the gather alone
        ctx = Context(0)
        d_rows = torch.from_numpy(quals).cuda()
        d_order = torch.from_numpy(np.fromfile(order_path, dtype="<u4").view(np.int32)).cuda()
        out = torch.empty_like(d_rows)
        ctx.qual_gather_rows(d_rows, d_order, out=out)
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            _, flags = ctx.qual_gather_rows(d_rows, d_order, out=out)
            e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
            if flags:
                raise RuntimeError("the order is not a permutation: flags %d" % flags)
        model = 2 * n * L + 4 * n
        res["gather"] = {"median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms), "model_bytes": model,
                         "model_GBps": model / (statistics.median(ms) * 1e-3) / 1e9, "note": "wall of the synchronous call by device events: includes the clearing of the marks and the launch"}
        if not bool((out == d_rows[d_order.long()]).all()):
            raise RuntimeError("the gathered rows differ from torch indexing")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if a.sizes_out:
        with open(a.sizes_out, "w") as f:
            f.write(json.dumps({"rows": n, "L": L, **res["sizes"]}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    try:
        sys.exit(main())
    except Exception as e:                                  # noqa: BLE001
        print("reorder_bench failed: %s" % e, file=sys.stderr)
        sys.exit(1)
