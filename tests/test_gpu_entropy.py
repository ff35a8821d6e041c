"""The built-in entropy stage on the GPU (csrc/entropy.hip) against its host twin: identical bytes, cross
decoding, the same hostile members refused, and the command line end to end with -G."""
import gzip
import os
import subprocess
import tarfile

import numpy as np
import pytest

import entropy_cases as ec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")


@pytest.fixture(scope="module")
def ctx():
    import minicom_amd
    return minicom_amd.Context(0)


def _dev(b):
    import torch
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda() if len(b) else torch.empty(0, dtype=torch.uint8, device="cuda")


def _host(t) -> bytes:
    return t.cpu().numpy().tobytes()


def test_device_bytes_equal_host_bytes_and_cross_decode(ctx, golden_dir):
    """every golden member and every synthetic case, default choice and every forced (model, stride): device encode == host encode,
    device decode of the host's member and host decode of the device's member give the original"""
    from minicom_amd import pipeline
    members = {"synthetic/" + k: v for k, v in ec.synthetic_members().items()}
    members.update(ec.golden_members(golden_dir))
    for name, raw in members.items():
        d_raw = _dev(raw)
        forced = ec.MODELS if (name.startswith("synthetic/") or name.startswith("order_stages_L100/") or name.startswith("pe_stages_L150/")) else ()
        for hint in (None,) + tuple(forced):
            kw = {} if hint is None else {"model": hint[0], "stride": hint[1]}
            host = pipeline.rans_encode(raw, **kw)
            dev = _host(ctx.rans_encode(d_raw, **kw))
            assert dev == host, (name, hint, len(dev), len(host))
            assert _host(ctx.rans_decode(_dev(host))) == raw, (name, hint)
            assert pipeline.rans_decode(dev) == raw, (name, hint)


def test_a_member_of_300_mb(ctx, golden_dir):
    """~300 MB (2.4 G bits: a 32-bit bit offset would wrap; 146 k segments, 572 workgroups): the same bytes as the host twin, and back"""
    from minicom_amd import pipeline
    import torch
    raw = ec.big_member(golden_dir, 300 * 1000 * 1000 + 1234)
    d_raw = torch.from_numpy(raw).cuda()
    for kw in ({}, {"model": 2, "stride": 1}):
        dev = ctx.rans_encode(d_raw, **kw)
        host = pipeline.rans_encode(raw.tobytes(), **kw)
        assert int(dev.shape[0]) == len(host)
        assert torch.equal(dev.cpu(), torch.from_numpy(np.frombuffer(host, dtype=np.uint8).copy())), kw
        back = ctx.rans_decode(dev)
        assert torch.equal(back, d_raw), kw
        del dev, back


def test_hostile_members_device_refuses_what_the_host_refuses(ctx, golden_dir):
    """a reduced, seeded sample of the CPU test's corpus (every 7th truncation, 300 flips) for the order-0 / order-1 members of one
    stream file: the device accepts exactly what the host accepts, and what it accepts is the original"""
    from minicom_amd import pipeline
    from minicom_amd.hip import McomError
    name, raw = ec.pick_hostile_member(golden_dir)
    for kw in ({}, {"model": 2, "stride": 2}):
        member = pipeline.rans_encode(raw, **kw)
        assert ec.parse_member(member)[0]["model"] != 0
        for label, bad in ec.hostile_corpus(member, flips=300, truncations=range(0, len(member), 7)):
            try:
                want = pipeline.rans_decode(bad, cap=len(raw))
            except McomError:
                want = None
            try:
                got = _host(ctx.rans_decode(_dev(bad), cap=len(raw)))
            except McomError:
                got = None
            assert got == want, (label, kw)
            assert want is None or want == raw, label


def _run(cmd, cwd):
    p = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-3000:]
    return p.stdout.decode(errors="replace")


@pytest.mark.parametrize("mode,tag,suffix", [("r", "stages_L100", "_comp"), ("p", "order_stages_L100", "_comp_order"), ("pe", "pe_stages_L100", "_comp_pe")])
def test_minicom_G_end_to_end(golden_dir, tmp_path, mode, tag, suffix):
    """minicom -r / -p / -1 -2 with -G at -t 1: every member ends in .rans, the archive holds the reference's stream files byte for byte,
    and both `minicom -d -G` and `minicom -d` (host twin) give the reads back"""
    from minicom_amd import container
    with gzip.open(os.path.join(golden_dir, "stages_L100.reads.gz"), "rb") as f:
        rows = f.read().split(b"\n")[:-1]
    half = len(rows) // 2

    def fastq(path, rs):
        with open(path, "wb") as f:
            for i, r in enumerate(rs):
                f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))
    if mode == "pe":
        fastq(tmp_path / "s_1.fastq", rows[:half]); fastq(tmp_path / "s_2.fastq", rows[half:2 * half])
        _run(["bash", os.path.join(BIN, "minicom"), "-1", "s_1.fastq", "-2", "s_2.fastq", "-t", "1", "-G"], tmp_path)
    else:
        fastq(tmp_path / "s.fastq", rows)
        _run(["bash", os.path.join(BIN, "minicom"), "-r", "s.fastq", "-t", "1", "-G"] + (["-p"] if mode == "p" else []), tmp_path)
    arch = tmp_path / ("s" + suffix + ".minicom")
    with tarfile.open(arch) as t:
        names = [os.path.basename(m.name) for m in t.getmembers() if m.isfile()]
    assert len(names) > 5 and all(n == "info.txt" or n.endswith(".rans") for n in names), names
    d = tmp_path / "unpacked"
    container.unpack(str(arch), str(d), device=0)
    want = {k.split("/")[1]: v for k, v in ec.golden_members(golden_dir).items() if k.split("/")[0] == tag}
    want.pop("ids.txt.0", None)
    assert sorted(os.listdir(d)) == sorted(want)
    for name, data in want.items():
        assert (d / name).read_bytes() == data, name
    base = arch.name[: -len(".minicom")]
    for flags in (["-G"], []):
        _run(["bash", os.path.join(BIN, "minicom"), "-d", arch.name] + flags, tmp_path)
        if mode == "pe":
            a = (tmp_path / (base + "_dec_1.reads")).read_bytes().split(b"\n")[:-1]
            b = (tmp_path / (base + "_dec_2.reads")).read_bytes().split(b"\n")[:-1]
            assert sorted(zip(a, b)) == sorted(zip(rows[:half], rows[half:2 * half])), flags
        else:
            got = (tmp_path / (base + "_dec.reads")).read_bytes().split(b"\n")[:-1]
            assert (got == rows if mode == "p" else sorted(got) == sorted(rows)), flags
