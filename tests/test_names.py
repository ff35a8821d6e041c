"""Read names and '+' lines as `.mcn` members on the host: the plain C++ twin of the GPU coder
(host/mcom_names.cpp) against the independent reference (tests/name_reference.py).  No GPU anywhere in this file; the device side is
tests/test_gpu_names.py."""
import lzma
import os
import re
import subprocess

import pytest

import name_cases as nc
import name_reference as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = 96


def _coders():
    from minicom_amd import pipeline
    return pipeline.bwt_encode, pipeline.rans_encode, pipeline.bwt_decode, pipeline.rans_decode


def _ref_decode(member):
    _, _, bd, rd = _coders()
    return NR.ref_decode(member, bd, rd)


def _host_refuses(member) -> bool:
    from minicom_amd import McomError, pipeline
    try:
        pipeline.name_decode(member)
    except McomError:
        return True
    return False


@pytest.mark.parametrize("name,names,plus", nc.degenerate(), ids=[c[0] for c in nc.degenerate()])
def test_host_twin_emits_the_reference_bytes(name, names, plus):
    """every degenerate name text: the same bytes as the reference, and both decoders give the text back -- also from the kind the
    choice did not take"""
    from minicom_amd import pipeline
    be, re_, _, _ = _coders()
    text, n = nc.text_of(names, plus), len(names)
    assert pipeline.name_text(names, plus) == text
    got = pipeline.name_encode(text, n)
    assert got == NR.ref_encode(text, n, be, re_), (name, len(got))
    assert pipeline.name_info(got) == (n, len(text))
    assert pipeline.name_decode(got) == text and _ref_decode(got) == text
    for kind in ((0, 1) if n else (0,)):
        m = NR.ref_encode(text, n, be, re_, kind=kind)
        assert m[5] == kind and pipeline.name_decode(m) == text, (name, kind)


@pytest.mark.parametrize("gen", [nc.illumina, nc.sra], ids=["illumina", "sra"])
def test_generated_names_beat_xz(gen):
    """3000 records of each generator: the reference's bytes, kind 0, and smaller than lzma preset 6 of the same text (the Python
    model of the format gave 11.5 KB against 13.7 KB and 10.7 KB against 13.9 KB for the five name streams)"""
    from minicom_amd import pipeline
    be, re_, _, _ = _coders()
    text = nc.text_of(gen(1, 3000))
    m = pipeline.name_encode(text)
    assert m == NR.ref_encode(text, 3000, be, re_) and m[5] == 0
    assert pipeline.name_decode(m) == text
    assert len(m) < len(lzma.compress(text, preset=6)), (len(m), len(lzma.compress(text, preset=6)))


@pytest.mark.parametrize("rps", [1, 7, 4096])
def test_host_decodes_reference_members_at_other_recs_per_seg(rps):
    from minicom_amd import pipeline
    be, re_, _, _ = _coders()
    names = nc.illumina(4, 600)
    text = nc.text_of(names, nc.mixed_plus(names, 4))
    m = NR.ref_encode(text, 600, be, re_, recs_per_seg=rps, kind=0)
    assert int.from_bytes(m[28:30], "little") == rps
    assert pipeline.name_decode(m) == text and _ref_decode(m) == text
    if rps != 256:
        assert m != pipeline.name_encode(text, 600)


def test_noncanonical_members_decode():
    from minicom_amd import pipeline
    for name, member, text in nc.noncanonical():
        assert _ref_decode(member) == text, name
        assert pipeline.name_decode(member) == text, name


def test_one_crafted_member_per_refusal_rule():
    """the reference names the rule, the host twin refuses the member"""
    text, n, base = nc.small()
    assert _ref_decode(base) == text and not _host_refuses(base)
    rules = set()
    for name, rule, member in nc.crafted():
        with pytest.raises(NR.NameRefused) as e:
            _ref_decode(member)
        assert e.value.rule == rule, (name, e.value.rule)
        assert _host_refuses(member), name
        rules.add(rule)
    assert rules >= {"op above 5", "END count", "op counts", "tlen sum", "plus kind", "ptext", "newline", "no previous token", "value", "25th token",
                     "name above 255", "text length", "crc", "header", "raw lengths", "embedded"}
    # kind 1: an embedded member of another text, with another CRC, a damaged one, and a text that is not two lines per record
    from minicom_amd import pipeline
    be, re_, _, _ = _coders()
    good = NR.ref_encode(text, n, be, re_, kind=1)
    assert _ref_decode(good) == text and not _host_refuses(good)
    flipped = bytearray(good); flipped[-1] ^= 0x10
    three = b"a\nb\nc\n"
    long_line = b"x" * 256 + b"\n\n"
    import zlib
    bad_lines = NR.ref_header(1, 1, len(three), zlib.crc32(three), 256, [0] * 7) + re_(three)
    bad_long = NR.ref_header(1, 1, len(long_line), zlib.crc32(long_line), 256, [0] * 7) + re_(long_line)
    for name, member in (("embedded text", good[:HEADER] + re_(text[:-2] + b"x\n")), ("embedded crc", good[:24] + bytes(4) + good[28:]), ("embedded damage", bytes(flipped)),
                         ("odd lines", bad_lines), ("long line", bad_long)):
        with pytest.raises(NR.NameRefused):
            _ref_decode(member)
        assert _host_refuses(member), name


def test_hostile_corpus_is_refused_or_exact():
    """every truncation and 200 bit flips of a small member: refused, or decoded to exactly what the reference decodes; never a crash.
    The host twin and the reference take the same decision for every member."""
    from minicom_amd import pipeline
    for member in nc.truncations() + nc.bit_flips():
        try:
            want = _ref_decode(member)
        except NR.NameRefused:
            want = None
        if want is None:
            assert _host_refuses(member)
        else:
            assert pipeline.name_decode(member) == want


def test_refused_inputs_name_the_record():
    from minicom_amd import McomError, pipeline
    for name, text, n, rec in nc.refused_inputs():
        with pytest.raises(McomError) as e:
            pipeline.name_encode(text, n)
        if rec is not None:
            assert "record %d " % (rec + 1) in str(e.value), (name, str(e.value))


@pytest.mark.parametrize("name,names,plus", nc.degenerate(), ids=[c[0] for c in nc.degenerate()])
def test_size_bound_against_the_rans_member(name, names, plus):
    """.mcn <= the `.rans` member of the name text + the header"""
    from minicom_amd import pipeline
    text = nc.text_of(names, plus)
    assert len(pipeline.name_encode(text, len(names))) <= len(pipeline.rans_encode(text)) + HEADER


def test_file_forms_and_mcomz(tmp_path):
    """mcomh_name_pack_file / _unpack_file and `mcomz e --names` / `mcomz d`: the member of pipeline.name_encode, the text back; a
    damaged member and a text with a 256-byte name leave no output file"""
    from minicom_amd import McomError, pipeline
    names = nc.sra(2, 500)
    text = nc.text_of(names, nc.mixed_plus(names, 1))
    src, mem, back = tmp_path / "names.txt", tmp_path / "name.mcn", tmp_path / "back.txt"
    src.write_bytes(text)
    pipeline.name_file(str(src), str(mem), True)
    assert mem.read_bytes() == pipeline.name_encode(text)
    pipeline.name_file(str(mem), str(back), False)
    assert back.read_bytes() == text
    mcomz = os.path.join(ROOT, "bin", "mcomz")
    mem2, back2 = tmp_path / "m2.mcn", tmp_path / "b2.txt"
    assert subprocess.run([mcomz, "e", "--names", str(src), str(mem2)]).returncode == 0 and mem2.read_bytes() == mem.read_bytes()
    assert subprocess.run([mcomz, "d", str(mem2), str(back2)]).returncode == 0 and back2.read_bytes() == text
    bad = bytearray(mem.read_bytes()); bad[len(bad) // 2] ^= 0x40
    (tmp_path / "bad.mcn").write_bytes(bytes(bad))
    out = tmp_path / "never.txt"
    with pytest.raises(McomError):
        pipeline.name_file(str(tmp_path / "bad.mcn"), str(out), False)
    assert subprocess.run([mcomz, "d", str(tmp_path / "bad.mcn"), str(out)], stderr=subprocess.DEVNULL).returncode == 1
    (tmp_path / "long.txt").write_bytes(b"ok\n\n" + b"n" * 256 + b"\n\n")
    r = subprocess.run([mcomz, "e", "--names", str(tmp_path / "long.txt"), str(out)], stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"record 2" in r.stderr
    assert not out.exists()


def test_a_gpu_route_without_a_gpu_is_an_error(tmp_path):
    """device= asks for the GPU coder: without a GPU that is an error, never the host twin"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this machine has a GPU: the refusal is tested where there is none")
    from minicom_amd import McomError, pipeline
    (tmp_path / "t.txt").write_bytes(b"a\n\n")
    with pytest.raises(McomError):
        pipeline.name_file(str(tmp_path / "t.txt"), str(tmp_path / "t.mcn"), True, device=0)
    assert not (tmp_path / "t.mcn").exists()
    with pytest.raises(Exception):
        pipeline.name_encode(b"a\n\n", 1, device=0)
    (tmp_path / "f.fastq").write_bytes(b"@a\nACGT\n+\nIIII\n")
    with pytest.raises(McomError):
        pipeline.fastq_name_member(str(tmp_path / "f.fastq"), str(tmp_path / "f.mcn"), device=0)
    with pytest.raises(McomError):
        pipeline.verify_names(str(tmp_path), str(tmp_path / "f.fastq"))
    assert not (tmp_path / "f.mcn").exists()
    r = subprocess.run([os.path.join(ROOT, "bin", "mcomz"), "e", "--names", "--gpu", str(tmp_path / "t.txt"), str(tmp_path / "t.mcn")], stderr=subprocess.DEVNULL)
    assert r.returncode == 1 and not (tmp_path / "t.mcn").exists()


def test_the_surface_exists():
    """headers, libraries, pipeline and Context"""
    import minicom_amd
    from minicom_amd import pipeline
    from minicom_amd.hip import Context
    h = open(os.path.join(ROOT, "include", "mcom.h")).read()
    hh = open(os.path.join(ROOT, "include", "mcom_host.h")).read()
    dev = ["mcom_name_bound", "mcom_name_encode", "mcom_name_info", "mcom_name_decode", "mcom_name_compare", "mcom_name_text_offsets", "mcom_fastq_name_text", "mcom_fastq_emit_named"]
    host = ["mcomh_name_bound", "mcomh_name_info", "mcomh_name_encode", "mcomh_name_decode", "mcomh_name_pack_file", "mcomh_name_unpack_file",
            "mcomh_fastq_names_to_device", "mcomh_fastq_name_member", "mcomh_verify_names_gpu"]
    lib, hl = minicom_amd.load_library(), pipeline.load_host_library()
    for s in dev:
        assert re.search(r"\b%s\s*\(" % s, h) and s in minicom_amd.ABI_SYMBOLS and getattr(lib, s)
    for s in host:
        assert re.search(r"\b%s\s*\(" % s, hh) and s in pipeline.HOST_ABI_SYMBOLS and getattr(hl, s)
    for f in ("name_text", "name_encode", "name_decode", "name_info", "name_file", "fastq_name_member", "fastq_names", "verify_names"):
        assert callable(getattr(pipeline, f))
    for f in ("name_encode", "name_decode", "name_compare", "fastq_names", "fastq_emit_named"):
        assert callable(getattr(Context, f))
    assert "MCOM_FASTQ_F_LONG = 16" in h
    assert int(lib.mcom_name_bound(1000)) == int(hl.mcomh_name_bound(1000)) >= 1000 + HEADER


# ---- name.mcn in a -p -Q archive: the host route ("Archive and decoders") -----------------------------------------
def _named_archive(golden_dir, d, with_qual=True):
    """the golden -p stream files of stages_L100 in folder d with a host-coded qual.mcq and name.mcn (generated names, mixed '+' lines);
    returns (the FASTQ the archive stands for, n)"""
    import gzip
    import io
    import tarfile
    import numpy as np
    import qual_cases as qc
    from minicom_amd import pipeline
    d.mkdir()
    with gzip.open(os.path.join(golden_dir, "streams_order_stages_L100.tar.gz"), "rb") as g:
        tf = tarfile.open(fileobj=io.BytesIO(g.read()))
        for m in tf.getmembers():
            (d / m.name).write_bytes(tf.extractfile(m).read())
    with gzip.open(os.path.join(golden_dir, "stages_L100.reads.gz"), "rb") as f:
        rows = f.read().split(b"\n")[:-1]
    n = len(rows)
    quals = np.resize(qc.synth_quals(21, 2000, 100), (n, 100))
    names = nc.illumina(5, n)
    plus = nc.mixed_plus(names, 3)
    if with_qual:
        (d / "qual.mcq").write_bytes(pipeline.qual_encode(quals))
    (d / "name.mcn").write_bytes(pipeline.name_encode(nc.text_of(names, plus), n))
    want = b"".join(b"@" + a + b"\n" + r + b"\n+" + p + b"\n" + q.tobytes() + b"\n" for a, p, r, q in zip(names, plus, rows, quals))
    return want, n


def test_host_route_gives_the_named_fastq_back(golden_dir, tmp_path):
    """golden -p streams + host-coded qual.mcq and name.mcn -> a FASTQ with generated names and mixed '+' lines, byte for byte, through
    mcomh_decompress_fastq, `decompress --fastq` and container.decompress_file; the container keeps name.mcn as it is and reports it"""
    import tarfile
    from minicom_amd import container, pipeline
    d = tmp_path / "arch"
    want, n = _named_archive(golden_dir, d)
    out = tmp_path / "out.fastq"
    assert pipeline.decompress_fastq(str(d), str(out)) == n
    assert out.read_bytes() == want
    p = subprocess.run([os.path.join(ROOT, "bin", "decompress"), "--fastq", str(d), str(tmp_path / "out2.fastq")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.split()[0] == str(n), p.stdout + p.stderr
    assert (tmp_path / "out2.fastq").read_bytes() == want
    arc = str(tmp_path / "a.minicom")
    sizes = container.pack(str(d), arc, codec="rans")
    assert sizes["name.mcn"] == (d / "name.mcn").stat().st_size
    with tarfile.open(arc) as t:
        assert t.extractfile("name.mcn").read() == (d / "name.mcn").read_bytes()
    assert container.unpack(arc, str(tmp_path / "back")) == {"order": True, "paired": False, "quality": True, "names": True}
    assert container.decompress_file(arc, str(tmp_path / "out3.fastq")) == n
    assert (tmp_path / "out3.fastq").read_bytes() == want


def test_host_route_refuses_a_name_member_that_does_not_fit(golden_dir, tmp_path):
    """name.mcn of another n, name.mcn without qual.mcq, a damaged member: an error and no output file, library and executable"""
    from minicom_amd import McomError, pipeline
    out = tmp_path / "never.fastq"

    def refused(d):
        with pytest.raises(McomError):
            pipeline.decompress_fastq(str(d), str(out))
        assert not out.exists()
        p = subprocess.run([os.path.join(ROOT, "bin", "decompress"), "--fastq", str(d), str(out)], capture_output=True)
        assert p.returncode == 1 and not out.exists()

    d = tmp_path / "other_n"
    _, n = _named_archive(golden_dir, d)
    names = nc.illumina(5, n - 1)
    (d / "name.mcn").write_bytes(pipeline.name_encode(nc.text_of(names), n - 1))
    refused(d)
    d = tmp_path / "no_qual"
    _named_archive(golden_dir, d, with_qual=False)
    refused(d)
    d = tmp_path / "damaged"
    _named_archive(golden_dir, d)
    b = bytearray((d / "name.mcn").read_bytes()); b[len(b) // 2] ^= 4; (d / "name.mcn").write_bytes(bytes(b))
    refused(d)


def test_fastq_name_member_host_twin(tmp_path):
    """mcomh_fastq_name_member without a GPU (what `minicom -N` runs without -G, `mcomz e --fastq-names`): the member is the coder's for
    the file's names and '+' texts (plain, without the last newline, gzip); a missing '@' or '+', a 256-byte name and a file that ends
    inside a record are errors that name the record and leave no output file"""
    import gzip
    from minicom_amd import McomError, pipeline
    names = nc.sra(8, 200) + [b"", b"z" * 255]
    plus = nc.mixed_plus(names, 4)
    recs = [b"@" + a + b"\nACGT\n+" + p + b"\nIIII\n" for a, p in zip(names, plus)]
    want = pipeline.name_encode(nc.text_of(names, plus), len(names))
    for tag, data in (("plain", b"".join(recs)), ("no_newline", b"".join(recs)[:-1]), ("gz", gzip.compress(b"".join(recs)))):
        src, mem = tmp_path / (tag + (".fastq.gz" if tag == "gz" else ".fastq")), tmp_path / (tag + ".mcn")
        src.write_bytes(data)
        assert pipeline.fastq_name_member(str(src), str(mem)) == len(names)
        assert mem.read_bytes() == want, tag
    mcomz = os.path.join(ROOT, "bin", "mcomz")
    p = subprocess.run([mcomz, "e", "--fastq-names", str(tmp_path / "plain.fastq"), str(tmp_path / "z.mcn")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.split() == [str(len(names))] and (tmp_path / "z.mcn").read_bytes() == want
    out = tmp_path / "never.mcn"
    for tag, rec, repl in (("no @", 17, b"X" + recs[17][1:]), ("no +", 30, recs[30].replace(b"\n+", b"\n-", 1)), ("256", 40, b"@" + b"n" * 256 + b"\nACGT\n+\nIIII\n"),
                           ("inside", len(recs) - 1, b"@x\nACGT\n+\n")):
        bad = list(recs); bad[rec] = repl
        (tmp_path / "bad.fastq").write_bytes(b"".join(bad))
        with pytest.raises(McomError) as e:
            pipeline.fastq_name_member(str(tmp_path / "bad.fastq"), str(out))
        assert "record %d" % (rec + 1) in str(e.value), (tag, str(e.value))
        assert not out.exists()
        p = subprocess.run([mcomz, "e", "--fastq-names", str(tmp_path / "bad.fastq"), str(out)], capture_output=True, text=True)
        assert p.returncode == 1 and "record %d" % (rec + 1) in p.stderr and not out.exists()


def _minicom(args, cwd):
    p = subprocess.run(["bash", os.path.join(ROOT, "bin", "minicom")] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    return p.returncode, p.stdout.decode(errors="replace")


def test_minicom_N_needs_p_and_Q(tmp_path):
    """`minicom -r x.fastq -p -N`, `-r x.fastq -N -Q` and `-1 a -2 b -N`: exit 1 with the message, no archive and no _comp folder; the
    usage text knows -N, and compress_fastq(names=True) asks for order and quality"""
    from minicom_amd import container
    (tmp_path / "x.fastq").write_bytes(b"@a\nACGT\n+\nIIII\n")
    for args in (["-r", "x.fastq", "-p", "-N"], ["-r", "x.fastq", "-N", "-Q"], ["-r", "x.fastq", "-N"], ["-1", "x.fastq", "-2", "x.fastq", "-N"]):
        rc, out = _minicom(args, tmp_path)
        assert rc == 1 and "-N needs -p -Q" in out, (args, out[-500:])
        assert sorted(p.name for p in tmp_path.iterdir()) == ["x.fastq"], args
    rc, out = _minicom(["-h"], tmp_path)
    assert rc == 0 and "-N " in out and "names" in out
    for kw in ({"order": True}, {"quality": True, "order": False}, {}):
        with pytest.raises(ValueError):
            container.compress_fastq(str(tmp_path / "x.fastq"), str(tmp_path / "x.minicom"), names=True, **kw)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["x.fastq"]
