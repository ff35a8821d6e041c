"""gzip members inflated by the host twin (host/mcom_gzip_gpu.cpp over csrc/inflate_model.hpp) and the walk over
BGZF headers (mcom_gzip_walk), held against the standard library's zlib on every input of tests/inflate_cases.py;
tests/test_gpu_inflate.py holds the device against the same cases."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_cases as BC
import inflate_cases as IC
import minicom_amd
from minicom_amd import pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MCOMZ = os.path.join(ROOT, "bin", "mcomz")


# ---- the walk ----
def test_walk_of_the_encoders_output():
    data = BC.cases()["len130561"]
    z = pipeline.bgzf_encode(data)
    tab, text, used, ok = pipeline.gzip_walk(z)
    ms = BC.members(z)
    assert ok and used == len(z) and text == len(data) and len(tab) == len(ms) + 1
    for (at, size), row, k in zip(ms, tab, range(len(ms))):
        want = data[k * BC.BLOCK:(k + 1) * BC.BLOCK]
        assert (row["in_off"], row["in_bytes"], row["out_off"], row["isize"], row["crc"]) == (at + 18, size - 26, k * BC.BLOCK, len(want), zlib.crc32(want))
    assert tab[-1]["isize"] == 0 and tab[-1]["in_bytes"] == 2 and tab[-1]["out_off"] == len(data)
    assert pipeline.gzip_walk(b"")[1:] == (0, 0, True)


def test_walk_skips_fname_and_other_subfields_and_counts():
    a, b, c = IC.case("fastq_l6"), IC.case("one_byte_fixed"), IC.case("empty_l6")
    extra = b"XY" + struct.pack("<H", 3) + b"abc"                                       # a second FEXTRA subfield in front of BC
    m = [IC.bgzf_member(a.payload, a.crc, a.isize, extra=extra, name=b"reads.fastq"), IC.bgzf_member(b.payload, b.crc, b.isize), IC.bgzf_member(c.payload, c.crc, c.isize, name=b"x")]
    z = b"".join(m)
    tab, text, used, ok = pipeline.gzip_walk(z)
    assert ok and used == len(z) and text == a.isize + 1 and len(tab) == 3
    assert z[int(tab[0]["in_off"]):int(tab[0]["in_off"] + tab[0]["in_bytes"])] == a.payload and tab[0]["in_off"] == 12 + 6 + len(extra) + len(b"reads.fastq") + 1
    assert z[int(tab[2]["in_off"]):int(tab[2]["in_off"] + tab[2]["in_bytes"])] == c.payload and tab[2]["out_off"] == a.isize + 1
    got, st = pipeline.gzip_inflate(z)
    assert got == a.text + b.text and st == b"\0\0\0"
    # the count-only form, and a table with room for two
    lib = minicom_amd.load_library()
    n, t, u = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert lib.mcom_gzip_walk(z, len(z), None, 0, C.byref(n), C.byref(t), C.byref(u)) == 0 and (n.value, t.value, u.value) == (3, a.isize + 1, len(z))
    two = np.zeros(2, dtype=IC.MEMBER_DTYPE)
    assert lib.mcom_gzip_walk(z, len(z), two.ctypes.data, 2, C.byref(n), C.byref(t), C.byref(u)) == 0 and (n.value, u.value) == (2, len(m[0]) + len(m[1]))
    assert (two == tab[:2]).all()


def test_walk_stops_at_what_is_not_a_whole_bgzf_member():
    a, b = IC.case("fastq_l6"), IC.case("fastq_l1")
    ma, mb = IC.bgzf_member(a.payload, a.crc, a.isize), IC.bgzf_member(b.payload, b.crc, b.isize)
    plain = zlib.compressobj(6, zlib.DEFLATED, 31)
    no_bc = plain.compress(a.text) + plain.flush()                                      # a gzip member without FEXTRA
    for z, whole in ((ma + mb[:-1], 1), (ma + mb[:10], 1), (ma + no_bc + mb, 1), (ma + mb + no_bc, 2), (no_bc, 0),
                     (ma + mb[:3] + bytes([mb[3] | 0x20]) + mb[4:], 1)):                   # truncated last member; no BC in the middle; a reserved flag bit
        tab, text, used, ok = pipeline.gzip_walk(z)
        assert not ok and len(tab) == whole and used == (0, len(ma), len(ma) + len(mb))[whole] and text == (0, a.isize, a.isize + b.isize)[whole]     # the whole members in front of the stop
        with pytest.raises(minicom_amd.McomError):
            pipeline.gzip_inflate(z)
    # a size below header plus trailer
    short = bytearray(IC.bgzf_member(b"\x03\x00", 0, 0)); struct.pack_into("<H", short, 16, 24)
    assert not pipeline.gzip_walk(bytes(short))[3]


# ---- the twin on every case ----
def test_the_cases_are_what_zlib_says():
    for c in IC.cases():
        text = IC.zlib_text(c.payload)
        fine = text is not None and len(text) == c.isize and zlib.crc32(text) == c.crc
        assert (c.want == IC.OK) == fine, c.name
    wants = {c.want for c in IC.cases()}
    assert wants == {IC.OK, IC.CORRUPT, IC.TRUNCATED, IC.ROOM, IC.CHECK}


def test_twin_on_every_case_with_guards():
    cs = IC.interleaved()
    assert {c.name for c in cs} == {c.name for c in IC.cases()}
    for i, c in enumerate(cs):
        if c.want != IC.OK:
            assert cs[i - 1].want == IC.OK and cs[i + 1].want == IC.OK                  # a good member on either side of every bad one
    data, tab, room = IC.layout(cs)
    out, st = pipeline.gzip_inflate_members(data, tab, room, fill=0xAA)
    IC.check(cs, tab, out, st, 0xAA, "twin")


def test_twin_members_alone_and_bad_tables():
    for c in IC.cases():
        data, tab, room = IC.layout([c], guard=3)
        out, st = pipeline.gzip_inflate_members(data, tab, room, fill=0x55)
        IC.check([c], tab, out, st, 0x55, "alone")
    a, b = IC.case("fastq_l6"), IC.case("fastq_l1")
    data, tab, room = IC.layout([a, b], guard=0)
    assert pipeline.gzip_inflate_members(data, tab, room)[1] == b"\0\0"
    for field, value in (("out_off", tab[1]["out_off"] - 1), ("in_bytes", len(data)), ("in_off", len(data) + 1), ("isize", b.isize + 1)):
        t2 = tab.copy(); t2[1][field] = value
        with pytest.raises(minicom_amd.McomError):
            pipeline.gzip_inflate_members(data, t2, room)
    t2 = tab[::-1].copy()                                                               # out of order
    with pytest.raises(minicom_amd.McomError):
        pipeline.gzip_inflate_members(data, t2, room)
    assert pipeline.gzip_inflate_members(b"", tab[:0], 0) == (b"", b"")


def test_gzip_inflate_of_a_buffer_and_its_return_values():
    lib = pipeline.load_host_library()
    data = BC.cases()["fastq"]
    z = pipeline.bgzf_encode(data)
    assert pipeline.gzip_inflate(z) == (data, b"\0" * (len(BC.members(z)) + 1))
    got = C.c_uint64()
    out = C.create_string_buffer(len(data))
    assert lib.mcomh_gzip_inflate(z, len(z), out, len(data), C.byref(got)) == 0 and got.value == len(data) and out.raw == data
    assert lib.mcomh_gzip_inflate(z, len(z), out, len(data) - 1, C.byref(got)) == -4 and got.value == len(data)
    assert lib.mcomh_gzip_inflate(z, len(z) - 1, out, len(data), C.byref(got)) == -1
    at, size = BC.members(z)[0]
    flipped = bytearray(z); flipped[at + size - 8] ^= 1
    assert lib.mcomh_gzip_inflate(bytes(flipped), len(z), out, len(data), C.byref(got)) == IC.CHECK
    flipped = bytearray(z); flipped[at + 18] |= 6                                       # BTYPE 3
    assert lib.mcomh_gzip_inflate(bytes(flipped), len(z), out, len(data), C.byref(got)) == IC.CORRUPT


# ---- files and the command line ----
def test_gunzip_file_round_trip_and_refusals(tmp_path):
    data = BC.cases()["len130561"] + BC.cases()["fastq"]
    (tmp_path / "a").write_bytes(data)
    assert subprocess.run([MCOMZ, "z", str(tmp_path / "a"), str(tmp_path / "a.gz")]).returncode == 0
    assert subprocess.run([MCOMZ, "u", str(tmp_path / "a.gz"), str(tmp_path / "a.back")]).returncode == 0
    assert (tmp_path / "a.back").read_bytes() == data
    pipeline.gunzip_file(str(tmp_path / "a.gz"), str(tmp_path / "a.py"))
    assert (tmp_path / "a.py").read_bytes() == data
    z = bytearray((tmp_path / "a.gz").read_bytes())
    at, size = BC.members(bytes(z))[1]
    z[at + size - 5] ^= 0x40                                                            # the second member's CRC
    (tmp_path / "bad.gz").write_bytes(bytes(z))
    with pytest.raises(minicom_amd.McomError):
        pipeline.gunzip_file(str(tmp_path / "bad.gz"), str(tmp_path / "bad.out"))
    assert not (tmp_path / "bad.out").exists()
    r = subprocess.run([MCOMZ, "u", str(tmp_path / "bad.gz"), str(tmp_path / "bad.out2")], capture_output=True, text=True)
    assert r.returncode == 1 and not (tmp_path / "bad.out2").exists() and "bad.gz" in r.stderr
    (tmp_path / "cut.gz").write_bytes(bytes(z[:len(z) - 30]))                           # not BGZF to its end
    with pytest.raises(minicom_amd.McomError):
        pipeline.gunzip_file(str(tmp_path / "cut.gz"), str(tmp_path / "cut.out"))
    assert not (tmp_path / "cut.out").exists()
    with pytest.raises(minicom_amd.McomError):
        pipeline.gunzip_file(str(tmp_path / "missing.gz"), str(tmp_path / "m.out"))
    for args in (["u"], ["u", "x"], ["u", "a", "b", "c"], ["u", "--gpu", "a", "b", "c"]):
        r = subprocess.run([MCOMZ] + args, capture_output=True, text=True)
        assert r.returncode == 1 and "usage: mcomz u [--gpu] IN.gz OUT" in r.stderr
    r = subprocess.run([MCOMZ, "x"], capture_output=True, text=True)
    assert r.returncode == 1 and "usage: mcomz e|d" in r.stderr and "mcomz z [--gpu] IN OUT.gz" in r.stderr and "mcomz u [--gpu] IN.gz OUT" in r.stderr


def test_surface():
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    dev, host, hooks = strip("mcom.h"), strip("mcom_host.h"), strip("mcom_test.h")
    lib, hl = minicom_amd.load_library(), pipeline.load_host_library()
    for name in ("mcom_gzip_walk", "mcom_gzip_inflate"):
        assert re.search(r"\b%s\s*\(" % name, dev) and hasattr(lib, name) and name in minicom_amd.ABI_SYMBOLS, name
    for name in ("mcomh_gzip_inflate", "mcomh_gzip_inflate_members", "mcomh_gunzip_file"):
        assert re.search(r"\b%s\s*\(" % name, host) and hasattr(hl, name) and name in pipeline.HOST_ABI_SYMBOLS, name
    assert re.search(r"\bmcomh_test_gz_device_members\s*\(", hooks) and hasattr(hl, "mcomh_test_gz_device_members")
    assert "mcom_gzip_member" in dev and "MCOM_GZIP_CHECK" in dev
    assert not [s for s in minicom_amd.ABI_SYMBOLS if s.startswith("mcom_decode_") and "gzip" in s]


# ---- the model under the sanitizers ----
def test_the_inflate_model_under_the_sanitizers(tmp_path):
    """tests/fuzz_inflate_model.cpp: the twin over the corpus below and several thousand seeded mutations of it (bit flips, cuts, spliced
    headers), every payload and every output in a heap block of exactly its size, every verdict and every byte held against
    host/mcom_inflate.cpp's mcom_gunzip_member.  Stand-alone: nothing is loaded into Python under a sanitizer."""
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ has no sanitizer runtime here")
    exe = tmp_path / "fuzz_inflate_model"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "minicom_amd", "host"), "fuzz_inflate_model", "FUZZ_INFLATE_OUT=" + str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    n = 0
    for c in IC.cases():
        if IC.fits_bgzf(c) and (len(c.payload) < 20000 or c.name in ("fastq_l6", "fibonacci_huffman_only", "hand_dist32768")):
            (corpus / ("%03d.gz" % n)).write_bytes(IC.bgzf_member(c.payload, c.crc, c.isize))
            n += 1
    assert n > 100
    r = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "fuzz_inflate_model ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
