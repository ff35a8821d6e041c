#!/usr/bin/env python3
"""BGZF input inflated on the GPU: timing.

  python tools/inflate_bench.py [--kernel-bytes 1073741824] [--reads 2000000] [--len 150] [--repeats 5] [--dir DIR]
                                [--parent-mcomz PATH] [--skip-kernel] [--skip-member] [--out FILE]

  kernel   mcom_gzip_inflate alone over --kernel-bytes of synthetic FASTQ on the card (a text of 64 blocks of 65280 bytes of
           tests/bgzf_cases.synthetic_fastq, its members tiled), packed by the project's own encoder and packed by Python's zlib at level 6
           in 65280-byte blocks: device events around the synchronous call (its table check, its launch, the statuses coming back), one
           warm-up, median and spread (max - min) of --repeats, GB/s of text.
  member   `mcomz e --fastq-qual L --gpu` and `mcomz e --fastq-names --gpu` on a BGZF file of --reads x --len: wall clock around the child
           process, one warm-up (page cache included), median and spread of --repeats.  With --parent-mcomz the same file goes through that
           build of the parent commit's mcomz as well, and the line says whether this build is faster by more than the two spreads
           together; the two members must be the same bytes.

One JSON line (also written to --out).  Nothing is retried."""
import argparse
import filecmp
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
MCOMZ = os.path.join(ROOT, "bin", "mcomz")
BLOCK = 65280


def timed(cmd):
    t0 = time.perf_counter()
    p = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    ms = (time.perf_counter() - t0) * 1e3
    if p.returncode:
        raise RuntimeError("%s failed: %s" % (" ".join(cmd), p.stderr.decode(errors="replace")[-500:]))
    return ms


def summary(ms):
    return {"ms": round(statistics.median(ms), 2), "spread_ms": round(max(ms) - min(ms), 2), "runs": len(ms)}


def fastq_file(path, n, L):
    """four-line records of one width: names @SIM:1:FC:1:<tile>:<x>:<y>, reads of the synthetic genome, the tests' synthetic qualities"""
    from minicom_amd import synth
    from qual_bench import synth_quals
    with open(path, "wb") as f:
        for at in range(0, n, 250000):
            m = min(250000, n - at)
            reads = synth.synth_reads(7 + at, m, L)
            quals = synth_quals(5 + at, m, L)
            idx = np.arange(at, at + m)
            name = np.frombuffer(b"@SIM:1:FC:1:0000:00000:00000", dtype=np.uint8)
            rec = np.empty((m, len(name) + 2 * L + 5), np.uint8)
            rec[:, :len(name)] = name
            for k in range(4):
                rec[:, 15 - k] = 48 + idx // 250 // 10 ** k % 10
            for k in range(5):
                rec[:, 21 - k] = 48 + idx * 7 % 100000 // 10 ** k % 10
                rec[:, 27 - k] = 48 + idx * 13 % 100000 // 10 ** k % 10
            o = len(name)
            rec[:, o] = 10; rec[:, o + 1:o + 1 + L] = reads; rec[:, o + 1 + L] = 10; rec[:, o + 2 + L] = ord("+"); rec[:, o + 3 + L] = 10
            rec[:, o + 4 + L:o + 4 + 2 * L] = quals; rec[:, o + 4 + 2 * L] = 10
            f.write(rec.tobytes())


def kernel_part(a):
    import torch
    import bgzf_cases as BC
    import minicom_amd
    from minicom_amd import pipeline
    from minicom_amd.hip import GZIP_MEMBER_DTYPE
    ctx = minicom_amd.Context(0)
    tile = BC.synthetic_fastq(61, 20000)[:64 * BLOCK]
    assert len(tile) == 64 * BLOCK
    reps = max(1, a.kernel_bytes // len(tile))
    res = {"text_bytes": reps * len(tile), "members": reps * 64}

    def zlib6(text):
        out = []
        for at in range(0, len(text), BLOCK):
            blk = text[at:at + BLOCK]
            c = zlib.compressobj(6, zlib.DEFLATED, -15)
            pay = c.compress(blk) + c.flush()
            size = 18 + len(pay) + 8
            out.append(BC.EOF[:16] + (size - 1).to_bytes(2, "little") + pay + zlib.crc32(blk).to_bytes(4, "little") + len(blk).to_bytes(4, "little"))
        return b"".join(out)
    for tag, packed in (("own_encoder", pipeline.bgzf_encode(tile, eof=False)), ("zlib_level_6", zlib6(tile))):
        tab, text, used, ok = pipeline.gzip_walk(packed)
        assert ok and text == len(tile) and len(tab) == 64
        big = np.tile(tab, reps)
        k = np.repeat(np.arange(reps, dtype=np.uint64), 64)
        big["in_off"] += k * np.uint64(len(packed))
        big["out_off"] += k * np.uint64(len(tile))
        d_in = torch.from_numpy(np.frombuffer(packed, dtype=np.uint8).copy()).cuda().repeat(reps)
        d_tab = torch.from_numpy(big.view(np.uint8).reshape(-1).copy()).cuda()
        d_out = torch.empty(reps * len(tile), dtype=torch.uint8, device="cuda:0")
        assert d_tab.numel() == reps * 64 * GZIP_MEMBER_DTYPE.itemsize
        _, st = ctx.gzip_inflate(d_in, d_tab, out=d_out)                    # warm-up
        assert int(st.max()) == 0 and bytes(d_out[-len(tile):].cpu().numpy()) == tile and bytes(d_out[:len(tile)].cpu().numpy()) == tile
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            ctx.gzip_inflate(d_in, d_tab, out=d_out)
            e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        r = summary(ms)
        r["compressed_bytes"] = reps * len(packed)
        r["text_GB_per_s"] = round(reps * len(tile) / r["ms"] / 1e6, 2)
        res[tag] = r
        del d_in, d_tab, d_out
    return res


def member_part(a, work):
    fq = os.path.join(work, "r.fastq")
    fastq_file(fq, a.reads, a.L)
    gz = fq + ".gz"
    timed([MCOMZ, "z", "--gpu", fq, gz])
    res = {"reads": a.reads, "L": a.L, "fastq_bytes": os.path.getsize(fq), "bgzf_bytes": os.path.getsize(gz)}
    os.remove(fq)
    builds = [("this", MCOMZ)] + ([("parent", a.parent_mcomz)] if a.parent_mcomz else [])
    steps = {"fastq_qual": ["e", "--fastq-qual", str(a.L), "--gpu"], "fastq_names": ["e", "--fastq-names", "--gpu"]}
    for step, args in steps.items():
        res[step] = {}
        for tag, exe in builds:
            out = os.path.join(work, "%s_%s.member" % (step, tag))
            timed([exe] + args + [gz, out])                                  # warm-up
            res[step][tag] = summary([timed([exe] + args + [gz, out]) for _ in range(a.repeats)])
            res[step][tag]["member_bytes"] = os.path.getsize(out)
        if a.parent_mcomz:
            t, p = res[step]["this"], res[step]["parent"]
            res[step]["same_member"] = filecmp.cmp(os.path.join(work, step + "_this.member"), os.path.join(work, step + "_parent.member"), shallow=False)
            res[step]["faster_by_ms"] = round(p["ms"] - t["ms"], 2)
            res[step]["faster_by_more_than_both_spreads"] = p["ms"] - t["ms"] > p["spread_ms"] + t["spread_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-bytes", type=int, default=1 << 30)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--len", type=int, default=150, dest="L")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--parent-mcomz", default=None)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-member", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("inflate_bench: no GPU", file=sys.stderr)
        return 1
    res = {"repeats": a.repeats}
    work = tempfile.mkdtemp(prefix="inflate_bench_", dir=a.dir)
    try:
        if not a.skip_kernel:
            res["kernel"] = kernel_part(a)
        if not a.skip_member:
            res["member"] = member_part(a, work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
