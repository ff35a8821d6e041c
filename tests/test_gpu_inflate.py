"""gzip members inflated on the device (csrc/inflate.hip): mcom_gzip_inflate gives the bytes and statuses of the
host twin and of the standard library's zlib on every case of tests/inflate_cases.py at unaligned addresses, writes nothing outside the
slots, refuses tables that leave the buffers, and the two FASTQ passes take a BGZF file through it with the rows and the name text of the
plain file.  The damaged members are refusal tests of bounded code (tests/test_inflate.py runs the same model over them, and over
thousands of mutations under the sanitizers, on the CPU); they go to the card only between good members."""
import ctypes as C
import glob
import gzip
import os
import struct
import subprocess
import tarfile
import zlib

import numpy as np
import pytest
import torch

import bgzf_cases as BC
import inflate_cases as IC
import minicom_amd
from minicom_amd import pipeline

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    return minicom_amd.Context(0)


@pytest.fixture(scope="module")
def everything():
    """every case between good ones, laid out once, with the twin's answer"""
    cs = IC.interleaved()
    data, tab, room = IC.layout(cs)
    out, st = pipeline.gzip_inflate_members(data, tab, room, fill=0xAA)
    IC.check(cs, tab, out, st, 0xAA, "twin")
    return cs, data, tab, room, out, st


def _device(ctx, data: bytes, tab, room: int, in_off: int = 0, out_off: int = 0, fill: int = 0xAA):
    n = len(data)
    src = torch.zeros(n + 16, dtype=torch.uint8, device="cuda:0")
    if n:
        src[in_off:in_off + n] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    buf = torch.full((room + 16,), fill, dtype=torch.uint8, device="cuda:0")
    _, st = ctx.gzip_inflate(src[in_off:in_off + n], tab, out=buf[out_off:out_off + room])
    return buf.cpu().numpy(), bytes(st.cpu().numpy())


@pytest.mark.parametrize("in_off,out_off", [(0, 0), (1, 3), (3, 1)])
def test_every_case_at_unaligned_addresses(ctx, everything, in_off, out_off):
    cs, data, tab, room, twin_out, twin_st = everything
    buf, st = _device(ctx, data, tab, room, in_off, out_off)
    assert (buf[:out_off] == 0xAA).all() and (buf[out_off + room:] == 0xAA).all()             # the guards around d_out
    out = buf[out_off:out_off + room].tobytes()
    IC.check(cs, tab, out, st, 0xAA, "device")                                                  # zlib's bytes, the rules' statuses, nothing outside the slots
    assert st == twin_st
    for i, c in enumerate(cs):
        if c.want == IC.OK:
            a = int(tab[i]["out_off"])
            assert out[a:a + c.isize] == twin_out[a:a + c.isize], c.name


def test_launch_shapes(ctx):
    # no member
    out, st = ctx.gzip_inflate(torch.empty(0, dtype=torch.uint8, device="cuda:0"), np.zeros(0, dtype=IC.MEMBER_DTYPE), out=torch.full((8,), 0xAA, dtype=torch.uint8, device="cuda:0"))
    assert st.numel() == 0 and (out.cpu().numpy() == 0xAA).all()
    # one member
    c = IC.case("fastq_l6")
    data, tab, room = IC.layout([c], guard=2)
    buf, st = _device(ctx, data, tab, room, 1, 1)
    IC.check([c], tab, buf[1:1 + room].tobytes(), st, 0xAA, "one")
    # 3000 members of 40 bytes of text each: more workgroups than CUs
    text = BC.synthetic_fastq(5, 600)[:3000 * 40]
    cs = [IC.good("m%d" % i, IC.deflate(text[40 * i:40 * i + 40], (1, 6, 9)[i % 3], (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED)[i % 2])) for i in range(3000)]
    data, tab, room = IC.layout(cs, guard=1)
    buf, st = _device(ctx, data, tab, room)
    IC.check(cs, tab, buf[:room].tobytes(), st, 0xAA, "3000")


def test_bad_tables_are_refused_and_nothing_is_written(ctx):
    a, b = IC.case("fastq_l6"), IC.case("fastq_l1")
    data, tab, room = IC.layout([a, b], guard=0)
    for field, value in (("out_off", int(tab[1]["out_off"]) - 1), ("in_bytes", len(data)), ("in_off", len(data) + 1), ("isize", b.isize + 1)):
        t2 = tab.copy(); t2[1][field] = value                                                   # slots that overlap; a payload that leaves d_in; a slot that leaves d_out
        with pytest.raises(minicom_amd.McomError):
            _device(ctx, data, t2, room)
        src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
        buf = torch.full((room,), 0xAA, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(minicom_amd.McomError):
            ctx.gzip_inflate(src, t2, out=buf)
        assert (buf.cpu().numpy() == 0xAA).all()
    with pytest.raises(minicom_amd.McomError):
        _device(ctx, data, tab[::-1].copy(), room)
    buf, st = _device(ctx, data, tab, room)
    assert st == b"\0\0" and buf[:room].tobytes() == a.text + b.text


def test_pipeline_routes_and_the_encoders_output(ctx, tmp_path):
    data = BC.cases()["len130561"] + BC.cases()["fastq"] + BC.cases()["random"]
    z = pipeline.bgzf_encode(data, device=0)                                                    # the project's own encoder's output comes back
    assert pipeline.gzip_inflate(z, device=0) == pipeline.gzip_inflate(z) == (data, b"\0" * (len(BC.members(z)) + 1))
    (tmp_path / "a.gz").write_bytes(z)
    pipeline.gunzip_file(str(tmp_path / "a.gz"), str(tmp_path / "a.dev"), device=0)
    pipeline.gunzip_file(str(tmp_path / "a.gz"), str(tmp_path / "a.host"))
    assert (tmp_path / "a.dev").read_bytes() == (tmp_path / "a.host").read_bytes() == data
    r = subprocess.run([os.path.join(ROOT, "bin", "mcomz"), "u", "--gpu", str(tmp_path / "a.gz"), str(tmp_path / "a.cli")])
    assert r.returncode == 0 and (tmp_path / "a.cli").read_bytes() == data
    bad = bytearray(z)
    at, size = BC.members(z)[1]
    bad[at + size - 6] ^= 4                                                                     # the second member's CRC
    got, st = pipeline.gzip_inflate(bytes(bad), device=0)
    assert st == pipeline.gzip_inflate(bytes(bad))[1] and st[1] == IC.CHECK and st.count(b"\0") == len(st) - 1 and got[:BC.BLOCK] == data[:BC.BLOCK] and got[2 * BC.BLOCK:] == data[2 * BC.BLOCK:]
    (tmp_path / "bad.gz").write_bytes(bytes(bad))
    with pytest.raises(minicom_amd.McomError):
        pipeline.gunzip_file(str(tmp_path / "bad.gz"), str(tmp_path / "bad.out"), device=0)
    assert not (tmp_path / "bad.out").exists()


# ---- the two FASTQ passes over a BGZF file ----
N_REC, L_REC = 2000, 100


def _small_members(text: bytes, step: int = 97) -> bytes:
    """members of `step` bytes of text, so that their ends fall inside every kind of line; empty members in the middle, no closing one"""
    out = []
    for k, at in enumerate(range(0, len(text), step)):
        piece = text[at:at + step]
        out.append(IC.bgzf_member(IC.deflate(piece, (1, 6, 0)[k % 3]), zlib.crc32(piece), len(piece)))
        if k % 50 == 7:
            out += [BC.EOF, BC.EOF]
    return b"".join(out)


def _device_members() -> int:
    lib = pipeline.load_host_library()
    lib.mcomh_test_gz_device_members.restype = C.c_long
    return int(lib.mcomh_test_gz_device_members())


@pytest.fixture(scope="module")
def fastq(tmp_path_factory):
    d = tmp_path_factory.mktemp("gz_fastq")
    text = BC.synthetic_fastq(91, N_REC, L_REC)
    (d / "plain.fastq").write_bytes(text)
    rows = pipeline.fastq_qualities(str(d / "plain.fastq"), L_REC).cpu().numpy()
    names = pipeline.fastq_names(str(d / "plain.fastq"))
    assert rows.shape == (N_REC, L_REC) and names[1] == N_REC
    return d, text, rows, names


@pytest.mark.parametrize("form", ["encoder", "small_members", "small_members_no_last_newline"])
def test_the_passes_inflate_bgzf_on_the_device(fastq, form):
    d, text, rows, names = fastq
    z = pipeline.bgzf_encode(text) if form == "encoder" else _small_members(text if form == "small_members" else text[:-1])
    assert gzip.decompress(z) == (text[:-1] if form.endswith("newline") else text)
    path = str(d / (form + ".fastq.gz"))
    open(path, "wb").write(z)
    for piece in (0, 300):
        got = pipeline.fastq_qualities(path, L_REC, piece_bytes=piece).cpu().numpy()
        assert _device_members() > 0, (form, piece)
        assert np.array_equal(got, rows), (form, piece)
        assert pipeline.fastq_names(path, piece_bytes=piece) == names, (form, piece)
        assert _device_members() > 0, (form, piece)


def test_other_forms_go_through_zlib_with_the_same_rows(fastq):
    d, text, rows, names = fastq
    z = pipeline.bgzf_encode(text)
    ms = BC.members(z)
    at, size = ms[1]
    no_bc = z[:at] + gzip.compress(text[BC.BLOCK:2 * BC.BLOCK], 6) + z[at + size:]              # one member's BC field removed: a plain gzip member in its place
    for tag, data in (("plain_gzip", gzip.compress(text, 6)), ("no_bc", no_bc)):
        path = str(d / (tag + ".fastq.gz"))
        open(path, "wb").write(data)
        assert np.array_equal(pipeline.fastq_qualities(path, L_REC).cpu().numpy(), rows), tag
        assert _device_members() == 0, tag
        assert pipeline.fastq_names(path) == names and _device_members() == 0, tag
    flipped = bytearray(z); flipped[at + size - 7] ^= 0x10                                     # one member's CRC
    path = str(d / "crc.fastq.gz")
    open(path, "wb").write(bytes(flipped))
    for call in (lambda: pipeline.fastq_qualities(path, L_REC), lambda: pipeline.fastq_names(path)):
        with pytest.raises(minicom_amd.McomError, match="damaged gzip stream"):                 # the zlib route's words
            call()
        assert _device_members() == 0


def _minicom(args, cwd):
    p = subprocess.run(["bash", os.path.join(ROOT, "bin", "minicom")] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    return p.returncode, p.stdout.decode(errors="replace")


def test_minicom_on_a_bgzf_input(fastq, tmp_path):
    """`minicom -r X.fastq.gz -p -Q -N -G` makes the archive of the plain file -- the same members, qual.mcq and name.mcn byte for byte --
    and `-d -c` says identical against the .gz file and against the plain one"""
    d, text, rows, names = fastq
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    (a / "X.fastq").write_bytes(text)
    (b / "X.fastq.gz").write_bytes(pipeline.bgzf_encode(text))
    rc, out = _minicom(["-r", "X.fastq", "-p", "-Q", "-N", "-G", "-t", "2"], a)
    assert rc == 0, out[-3000:]
    rc, out = _minicom(["-r", "X.fastq.gz", "-p", "-Q", "-N", "-G", "-t", "2"], b)
    assert rc == 0, out[-3000:]
    arc_a, arc_b = glob.glob(str(a / "*.minicom")), glob.glob(str(b / "*.minicom"))
    assert len(arc_a) == 1 and len(arc_b) == 1

    def members(path):
        with tarfile.open(path) as t:
            return {os.path.basename(m.name): t.extractfile(m).read() for m in t.getmembers() if m.isfile()}
    ma, mb = members(arc_a[0]), members(arc_b[0])
    assert sorted(ma) == sorted(mb) and {"qual.mcq", "name.mcn"} <= set(ma)
    for k in ("qual.mcq", "name.mcn"):                                                          # what the two passes make: byte for byte
        assert ma[k] == mb[k], k
    # (the read streams travel as a tar of files, whose headers carry the time of the run: they are held against both files instead)
    rc, out = _minicom(["-d", os.path.basename(arc_b[0]), "-c", "X.fastq.gz"], b)
    assert rc == 0 and out.count("identical") == 3, out[-3000:]
    rc, out = _minicom(["-d", os.path.basename(arc_b[0]), "-c", str(a / "X.fastq")], b)
    assert rc == 0 and out.count("identical") == 3, out[-3000:]
