#!/usr/bin/env python3
"""Entropy-stage timing, files -> files: `xz -6 -T16` (what bin/minicom runs on a machine without bsc) against bin/mcomz on the host twin
(one thread) and on GPU 0 -- the `.rans` coder and the block-sorting `.bwt` coder (its host twin once per file, for the size and one
time: it is a specification, not a fast coder); the size under Python's bz2 at level 9 beside them -- for every stream file of a synthetic read set, both directions.

  python tools/entropy_bench.py --reads 20000000 --len 150 --mode default|order [--repeats 3] [--dir DIR] [--out FILE]

Builds the stream set as tools/decode_bench.py does (same generator, same seed), runs every route once per file to warm up (page cache
included) and `--repeats` times measured: wall clock around the child process.  Per file and for the whole set: raw bytes, coded bytes
and median / spread (max - min) per route, the (model, stride) the coder chose, and the GPU route's own split of its median run
(mcomh_entropy_times through minicom_amd.pipeline.entropy_file, in this process: read + upload, codec call, download + write).
One JSON line (also written to --out).  Exit status 1 when a route fails, when a decoded file differs from its source, or when the GPU
route over the whole set is not faster than xz by more than the sum of the two spreads, in either direction.  Nothing is retried."""
import argparse
import bz2
import filecmp
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MCOMZ = os.path.join(ROOT, "bin", "mcomz")


def timed(cmd, stdout=None):
    t0 = time.perf_counter()
    p = subprocess.run(cmd, stdout=stdout, stderr=subprocess.PIPE)
    ms = (time.perf_counter() - t0) * 1e3
    if p.returncode:
        raise RuntimeError("%s failed: %s" % (" ".join(cmd), p.stderr.decode(errors="replace")[-500:]))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150, dest="L")
    ap.add_argument("--mode", choices=["default", "order"], default="default")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("entropy_bench: no GPU", file=sys.stderr)
        return 1
    import minicom_amd
    from minicom_amd import pipeline
    from minicom_amd.pipeline import Pipeline

    work = tempfile.mkdtemp(prefix="entropy_bench_", dir=a.dir)
    try:
        ctx = minicom_amd.Context(0)
        reads = ctx.synth_reads(4242, a.reads, a.L).cpu().numpy()
        p = Pipeline(reads, host_threads=8)
        p.pre_process()
        arch = os.path.join(work, "streams"); os.mkdir(arch)
        p.cluster_dump(arch, order=a.mode == "order")
        p.close()
        del reads, p, ctx
        torch.cuda.empty_cache(); pipeline.pool_trim()

        def routes(src):
            xz, rh, rg, back = src + ".xz", src + ".h.rans", src + ".g.rans", src + ".back"

            def xz_e():
                with open(xz, "wb") as f:
                    return timed(["xz", "-6", "-T16", "-c", src], stdout=f)

            def xz_d():
                with open(back, "wb") as f:
                    return timed(["xz", "-d", "-T16", "-c", xz], stdout=f)
            bh, bg = src + ".h.bwt", src + ".g.bwt"
            return {"xz": (xz_e, xz_d, xz), "host": (lambda: timed([MCOMZ, "e", src, rh]), lambda: timed([MCOMZ, "d", rh, back]), rh),
                    "gpu": (lambda: timed([MCOMZ, "e", "--gpu", src, rg]), lambda: timed([MCOMZ, "d", "--gpu", rg, back]), rg),
                    # the block-sorting coder: further columns, outside the verdict and the exit status (bwt_same_bytes reports them)
                    "bwt_host": (lambda: timed([MCOMZ, "e", "--bwt", src, bh]), lambda: timed([MCOMZ, "d", bh, back]), bh),
                    "bwt_gpu": (lambda: timed([MCOMZ, "e", "--bwt", "--gpu", src, bg]), lambda: timed([MCOMZ, "d", "--gpu", bg, back]), bg)}

        res = {"reads": a.reads, "L": a.L, "mode": a.mode, "repeats": a.repeats, "files": {}}
        tot = {r: {"enc": [0.0] * a.repeats, "dec": [0.0] * a.repeats, "bytes": 0} for r in ("xz", "host", "gpu", "bwt_host", "bwt_gpu")}
        bz2_total = 0
        raw_total = 0
        same = True
        bwt_same = True
        for name in sorted(os.listdir(arch)):
            src = os.path.join(arch, name)
            if name == "info.txt" or not os.path.isfile(src):
                continue
            row = {"raw": os.path.getsize(src)}
            raw_total += row["raw"]
            for r, (enc, dec, coded) in routes(src).items():
                once = r == "bwt_host"                                 # (one run, no warm-up: minutes per file on a large set)
                if not once:
                    enc(); dec()                                       # warm-up
                e = [enc() for _ in range(1 if once else a.repeats)] * (a.repeats if once else 1)
                d = [dec() for _ in range(1 if once else a.repeats)] * (a.repeats if once else 1)
                back_ok = filecmp.cmp(src, src + ".back", shallow=False)
                if r.startswith("bwt"):
                    bwt_same = bwt_same and back_ok
                else:
                    same = same and back_ok
                row[r] = {"bytes": os.path.getsize(coded), "enc_ms": round(statistics.median(e), 1), "enc_spread_ms": round(max(e) - min(e), 1),
                          "dec_ms": round(statistics.median(d), 1), "dec_spread_ms": round(max(d) - min(d), 1)}
                for i in range(a.repeats):
                    tot[r]["enc"][i] += e[i]; tot[r]["dec"][i] += d[i]
                tot[r]["bytes"] += row[r]["bytes"]
            with open(src + ".g.rans", "rb") as f:
                head = f.read(8)
            row["model"], row["stride"] = head[5], head[6]
            same = same and filecmp.cmp(src + ".h.rans", src + ".g.rans", shallow=False)
            bwt_same = bwt_same and filecmp.cmp(src + ".h.bwt", src + ".g.bwt", shallow=False)
            with open(src, "rb") as f:                                 # the yardstick of its kind: a block-sorting coder that is installed (size only)
                row["bz2_9_bytes"] = len(bz2.compress(f.read(), 9))
            bz2_total += row["bz2_9_bytes"]
            # the GPU route's own split, in this process (no process start, no runtime start-up)
            pipeline.entropy_file(src, src + ".s.rans", True, 0)
            row["gpu_split_enc"] = {k: round(v, 1) for k, v in pipeline.entropy_file(src, src + ".s.rans", True, 0).items()}
            pipeline.entropy_file(src + ".s.rans", src + ".back", False, 0)
            row["gpu_split_dec"] = {k: round(v, 1) for k, v in pipeline.entropy_file(src + ".s.rans", src + ".back", False, 0).items()}
            res["files"][name] = row
        res["raw_bytes"] = raw_total
        res["bz2_9_bytes"] = bz2_total
        for r in tot:
            res[r] = {"bytes": tot[r]["bytes"]}
            for k in ("enc", "dec"):
                res[r][k + "_ms"] = round(statistics.median(tot[r][k]), 1)
                res[r][k + "_spread_ms"] = round(max(tot[r][k]) - min(tot[r][k]), 1)
        res["same_bytes"] = same
        res["bwt_same_bytes"] = bwt_same
        ok = same
        for k in ("enc", "dec"):
            margin = res["xz"][k + "_ms"] - res["gpu"][k + "_ms"]
            res[k + "_gpu_faster_than_xz_by_ms"] = round(margin, 1)
            ok = ok and margin > res["xz"][k + "_spread_ms"] + res["gpu"][k + "_spread_ms"]
        res["ok"] = ok
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return 0 if ok else 1
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
