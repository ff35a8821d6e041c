"""`.mcn` kind 2 on the host: the name text of the second file of a pair coded against the first file's -- the
plain C++ twin (host/mcom_names.cpp) against the independent reference (tests/mate_name_reference.py).  No GPU anywhere in this file;
the device side is tests/test_gpu_mate_names.py."""
import os
import subprocess

import pytest

import mate_name_cases as mc
import mate_name_reference as MR
import name_reference as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = 96


def _coders():
    from minicom_amd import pipeline
    return pipeline.bwt_encode, pipeline.rans_encode, pipeline.bwt_decode, pipeline.rans_decode


def _ref_decode(member, mate):
    _, _, bd, rd = _coders()
    return MR.ref_decode_mate(member, mate, bd, rd)


def _host_decode(member, mate):
    """the text, or None when the host twin refuses"""
    from minicom_amd import McomError, pipeline
    try:
        return pipeline.name_decode(member, mate=mate)
    except McomError:
        return None


def test_reference_self_check():
    """the reference's own checks, over the library's `.bwt` coders this time; the host twin decodes the member they make"""
    from minicom_amd import pipeline
    member, mate, text = MR.self_check(pipeline.bwt_encode, pipeline.bwt_decode)
    assert member[5] == 2 and pipeline.name_decode(member, mate=mate) == text


@pytest.mark.parametrize("name,names,plus,mnames,mplus", mc.cases(), ids=[c[0] for c in mc.cases()])
def test_host_twin_emits_the_reference_bytes(name, names, plus, mnames, mplus):
    """every case: the reference's bytes (its choice of kind included), never more than the member without a mate, the text back from
    both decoders -- also from the kind-2 member where the choice did not take it -- and kind 2 refused without the mate"""
    from minicom_amd import McomError, pipeline
    be, re_, _, _ = _coders()
    text, mate, n = mc.text_of(names, plus), mc.text_of(mnames, mplus), len(names)
    got = pipeline.name_encode(text, n, mate=mate)
    want = MR.ref_encode_mate(text, n, mate, be, re_)
    assert got == want, (name, len(got), len(want), got[5], want[5])
    alone = pipeline.name_encode(text, n)
    assert len(got) <= len(alone) and (got == alone or (got[5] == 2 and len(got) < len(alone))), name
    assert pipeline.name_info(got, mate=True) == (n, len(text))
    assert pipeline.name_decode(got, mate=mate) == text and _ref_decode(got, mate) == text
    forced = MR.ref_encode_mate(text, n, mate, be, re_, kind=2)
    assert forced[5] == 2 and forced[28:30] == b"\x01\x00"
    assert pipeline.name_decode(forced, mate=mate) == text and _ref_decode(forced, mate) == text, name
    with pytest.raises(McomError):
        pipeline.name_decode(forced)
    with pytest.raises(McomError):
        pipeline.name_info(forced)
    if name in ("n255", "n256", "n257", "n1000", "identical", "inc", "plus_mixed", "mate_plus_nonempty"):
        assert got[5] == 2, name
    if name == "unrelated":
        assert got == alone and got[5] != 2


def test_the_mates_plus_lines_do_not_reach_the_streams():
    """two mates that differ in their '+' lines alone: the same streams, another mate crc"""
    from minicom_amd import pipeline
    a, b = mc.illumina_pair(5, 500)
    text = mc.text_of(b)
    m1 = pipeline.name_encode(text, 500, mate=mc.text_of(a))
    m2 = pipeline.name_encode(text, 500, mate=mc.text_of(a, mc.nc.mixed_plus(a, 1)))
    assert m1[5] == m2[5] == 2 and m1[:88] == m2[:88] and m1[96:] == m2[96:] and m1[88:92] != m2[88:92]


def test_noncanonical_members_decode():
    for name, member, mate, text in mc.noncanonical():
        assert _ref_decode(member, mate) == text, name
        assert _host_decode(member, mate) == text, name


def test_one_crafted_member_per_refusal_rule():
    """the reference names the rule, the host twin refuses the member"""
    from minicom_amd import McomError, pipeline
    text, n, mate, base = mc.small()
    assert _ref_decode(base, mate) == text and _host_decode(base, mate) == text
    rules = set()
    for name, rule, member, m in mc.crafted():
        with pytest.raises(NR.NameRefused) as e:
            _ref_decode(member, m)
        assert e.value.rule == rule, (name, e.value.rule)
        assert _host_decode(member, m) is None, name
        rules.add(rule)
    assert rules >= {"mate", "header", "no mate token", "value", "25th token", "name above 255", "text length", "op above 5", "END count", "newline",
                     "plus kind", "op counts", "ptext", "crc"}
    # kind 2 handed to the readers that hold no mate
    _, _, bd, rd = _coders()
    with pytest.raises(NR.NameRefused):
        NR.ref_decode(base, bd, rd)
    with pytest.raises(McomError):
        pipeline.name_decode(base)


def test_hostile_corpus_is_refused_or_exact():
    """every truncation and 200 bit flips of a kind-2 member, and 100 bit flips of the mate under the intact member: refused, or decoded
    to exactly what the reference decodes (a text whose crc is the header's); never a crash.  One decision for twin and reference."""
    import zlib
    import numpy as np
    text, n, mate, base = mc.small()
    corpus = [(m, mate) for m in mc.truncations() + mc.bit_flips()]
    rng = np.random.default_rng(5)
    for _ in range(100):
        b = bytearray(mate); at = int(rng.integers(0, len(b))); b[at] ^= 1 << int(rng.integers(0, 8))
        corpus.append((base, bytes(b)))
    taken = 0
    for member, m in corpus:
        try:
            want = _ref_decode(member, m)
        except NR.NameRefused:
            want = None
        got = _host_decode(member, m)
        assert got == want
        if got is not None:
            taken += 1
            assert zlib.crc32(got) == int.from_bytes(member[24:28], "little")


def test_refused_inputs():
    """a text the coder without a mate refuses is refused here too, with its record; so is a mate that is not two lines per record or
    holds a line above 255 bytes"""
    from minicom_amd import McomError, pipeline
    for name, text, n, rec in mc.nc.refused_inputs():
        with pytest.raises(McomError) as e:
            pipeline.name_encode(text, n, mate=b"m\n\n" * n)
        if rec is not None:
            assert "record %d " % (rec + 1) in str(e.value), (name, str(e.value))
    for mate in (b"", b"a\n\n", b"a\n\nb\n\nc\n\n", b"a\n\nb\n", b"a\n\nb\n\nc", b"a\n\n" + b"n" * 256 + b"\n\n"):
        with pytest.raises(McomError):
            pipeline.name_encode(b"x\n\ny\n\n", 2, mate=mate)


@pytest.mark.parametrize("style,gen", mc.STYLES, ids=[s[0] for s in mc.STYLES])
def test_size_condition(style, gen):
    """200 000 records of each style: name_2 coded against name_1 is at most a tenth of name_2 coded alone (the figures are in
    profiles/r13_mate_name_sizes.json), and decodes"""
    from minicom_amd import pipeline
    a, b = gen(1, 200000)
    text, mate = mc.text_of(b), mc.text_of(a)
    m = pipeline.name_encode(text, 200000, mate=mate)
    alone = pipeline.name_encode(text, 200000)
    print(style, len(m), len(alone))
    assert m[5] == 2 and 10 * len(m) <= len(alone), (style, len(m), len(alone))
    assert pipeline.name_decode(m, mate=mate) == text


def test_file_forms_and_mcomz(tmp_path):
    """mcomh_name_pack_file_mate / _unpack_file_mate and `mcomz e --names --mate` / `mcomz d --mate`: pipeline.name_encode's member, the
    text back; without --mate, with another mate and from a damaged member: exit 1 and no output file"""
    from minicom_amd import McomError, pipeline
    a, b = mc.illumina_pair(2, 500)
    text, mate = mc.text_of(b, mc.nc.mixed_plus(b, 1)), mc.text_of(a)
    src, mt, mem, back = tmp_path / "names2.txt", tmp_path / "names1.txt", tmp_path / "name_2.mcn", tmp_path / "back.txt"
    src.write_bytes(text); mt.write_bytes(mate)
    pipeline.name_file(str(src), str(mem), True, mate_path=str(mt))
    assert mem.read_bytes() == pipeline.name_encode(text, mate=mate) and mem.read_bytes()[5] == 2
    pipeline.name_file(str(mem), str(back), False, mate_path=str(mt))
    assert back.read_bytes() == text
    mcomz = os.path.join(ROOT, "bin", "mcomz")
    mem2, back2 = tmp_path / "m2.mcn", tmp_path / "b2.txt"
    assert subprocess.run([mcomz, "e", "--names", "--mate", str(mt), str(src), str(mem2)]).returncode == 0 and mem2.read_bytes() == mem.read_bytes()
    assert subprocess.run([mcomz, "d", "--mate", str(mt), str(mem2), str(back2)]).returncode == 0 and back2.read_bytes() == text
    out = tmp_path / "never.txt"
    assert subprocess.run([mcomz, "d", str(mem2), str(out)], stderr=subprocess.DEVNULL).returncode == 1 and not out.exists()
    with pytest.raises(McomError):
        pipeline.name_file(str(mem), str(out), False)
    assert subprocess.run([mcomz, "d", "--mate", str(src), str(mem2), str(out)], stderr=subprocess.DEVNULL).returncode == 1 and not out.exists()
    bad = bytearray(mem.read_bytes()); bad[len(bad) // 2] ^= 0x40
    (tmp_path / "bad.mcn").write_bytes(bytes(bad))
    assert subprocess.run([mcomz, "d", "--mate", str(mt), str(tmp_path / "bad.mcn"), str(out)], stderr=subprocess.DEVNULL).returncode == 1 and not out.exists()
    assert subprocess.run([mcomz, "e", "--bwt", "--mate", str(mt), str(src), str(out)], stderr=subprocess.DEVNULL).returncode == 1 and not out.exists()
    # --mate has no meaning for a member of another coder
    (tmp_path / "t.rans").write_bytes(pipeline.rans_encode(text))
    assert subprocess.run([mcomz, "d", "--mate", str(mt), str(tmp_path / "t.rans"), str(out)], stderr=subprocess.DEVNULL).returncode == 1 and not out.exists()
    assert subprocess.run([mcomz, "d", str(tmp_path / "t.rans"), str(out)]).returncode == 0 and out.read_bytes() == text
    out.unlink()
    # a member of kind 0 or 1 decodes with any mate
    plain = tmp_path / "plain.mcn"
    plain.write_bytes(pipeline.name_encode(text))
    assert subprocess.run([mcomz, "d", "--mate", str(src), str(plain), str(back2)]).returncode == 0 and back2.read_bytes() == text


def test_fastq_name_member_mate_host_twin(tmp_path):
    """mcomh_fastq_name_member_mate without a GPU (`mcomz e --fastq-names --mate FILE_1.fastq`): the coder's member for the names of
    file 2 against those of file 1; files that differ in records are an error and leave no member"""
    from minicom_amd import McomError, pipeline
    a, b = mc.illumina_pair(8, 400)
    p1, p2 = mc.nc.mixed_plus(a, 4), mc.nc.mixed_plus(b, 6)
    (tmp_path / "A_1.fastq").write_bytes(b"".join(b"@" + x + b"\nACGT\n+" + p + b"\nIIII\n" for x, p in zip(a, p1)))
    (tmp_path / "A_2.fastq").write_bytes(b"".join(b"@" + x + b"\nACGT\n+" + p + b"\nIIII\n" for x, p in zip(b, p2)))
    want = pipeline.name_encode(mc.text_of(b, p2), 400, mate=mc.text_of(a, p1))
    assert want[5] == 2
    assert pipeline.fastq_name_member(str(tmp_path / "A_2.fastq"), str(tmp_path / "n2.mcn"), mate_path=str(tmp_path / "A_1.fastq")) == 400
    assert (tmp_path / "n2.mcn").read_bytes() == want
    mcomz = os.path.join(ROOT, "bin", "mcomz")
    p = subprocess.run([mcomz, "e", "--fastq-names", "--mate", str(tmp_path / "A_1.fastq"), str(tmp_path / "A_2.fastq"), str(tmp_path / "z.mcn")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.split() == ["400"] and (tmp_path / "z.mcn").read_bytes() == want
    (tmp_path / "short.fastq").write_bytes(b"".join(b"@" + x + b"\nACGT\n+\nIIII\n" for x in a[:399]))
    out = tmp_path / "never.mcn"
    with pytest.raises(McomError) as e:
        pipeline.fastq_name_member(str(tmp_path / "A_2.fastq"), str(out), mate_path=str(tmp_path / "short.fastq"))
    assert "399" in str(e.value) and not out.exists()


def test_a_gpu_route_without_a_gpu_is_an_error(tmp_path):
    """device= asks for the GPU coder: without a GPU that is an error, never the host twin"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this machine has a GPU: the refusal is tested where there is none")
    from minicom_amd import McomError, pipeline
    (tmp_path / "t.txt").write_bytes(b"a/2\n\n"); (tmp_path / "m.txt").write_bytes(b"a/1\n\n")
    with pytest.raises(McomError):
        pipeline.name_file(str(tmp_path / "t.txt"), str(tmp_path / "t.mcn"), True, device=0, mate_path=str(tmp_path / "m.txt"))
    assert not (tmp_path / "t.mcn").exists()
    with pytest.raises(Exception):
        pipeline.name_encode(b"a/2\n\n", 1, device=0, mate=b"a/1\n\n")


def _minicom(args, cwd):
    p = subprocess.run(["bash", os.path.join(ROOT, "bin", "minicom")] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    return p.returncode, p.stdout.decode(errors="replace")


def test_minicom_refusals_are_what_they_were(tmp_path):
    """-1 -2 -Q without -p, -N without -p -Q, -q with -p / -Q / -N: exit 1 with the message they had; -1 -2 -p -N without -Q: exit 1; no
    archive and no _comp folder; the usage text knows the pair in input order; compress_fastq_pair(names=True, quality=False) and
    compress_fastq(order=True, path2=...) raise ValueError"""
    from minicom_amd import container
    (tmp_path / "x.fastq").write_bytes(b"@a\nACGT\n+\nIIII\n")
    pair = ["-1", "x.fastq", "-2", "x.fastq"]
    for args, msg in ((pair + ["-Q"], "-Q needs -p and a single file"), (pair + ["-N"], "-N needs -p -Q"), (pair + ["-Q", "-N"], "-Q needs -p and a single file"),
                      (pair + ["-N", "-Q"], "-N needs -p -Q"), (["-r", "x.fastq", "-N"], "-N needs -p -Q"), (["-r", "x.fastq", "-p", "-N"], "-N needs -p -Q"),
                      (["-r", "x.fastq", "-Q"], "-Q needs -p"), (pair + ["-q", "-p"], "cannot be combined with -p"), (pair + ["-q", "-Q"], "cannot be combined with -Q"),
                      (pair + ["-q", "-N"], "cannot be combined with -N"), (["-r", "x.fastq", "-q", "-p"], "cannot be combined with -p, -Q or -N"),
                      (pair + ["-p", "-N"], "-N needs -p -Q")):
        rc, out = _minicom(args, tmp_path)
        assert rc == 1 and msg in out, (args, rc, out[-500:])
        assert sorted(p.name for p in tmp_path.iterdir()) == ["x.fastq"], args
    rc, out = _minicom(["-h"], tmp_path)
    assert rc == 0 and "_comp_pe_order.minicom" in out and "_dec_1.fastq" in out
    with pytest.raises(ValueError):
        container.compress_fastq_pair(str(tmp_path / "x.fastq"), str(tmp_path / "x.fastq"), str(tmp_path / "x.minicom"), names=True, quality=False)
    with pytest.raises(ValueError):
        container.compress_fastq(str(tmp_path / "x.fastq"), str(tmp_path / "x.minicom"), path2=str(tmp_path / "x.fastq"), order=True)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["x.fastq"]


def test_pair_archive_host_decoders_refuse(tmp_path):
    """mcomh_decompress_order_pe / _fastq_order_pe and `decompress --order-pe` on folders that are no pair kept in input order: an empty one,
    golden -p streams without pe_order.txt, with a pe_order.txt of another count: an error, neither output file"""
    import gzip
    import io
    import tarfile
    from minicom_amd import McomError, pipeline
    golden = os.path.join(ROOT, "tests", "golden", "streams_order_stages_L100.tar.gz")
    d = tmp_path / "arch"; d.mkdir()
    with gzip.open(golden, "rb") as g:
        tf = tarfile.open(fileobj=io.BytesIO(g.read()))
        for m in tf.getmembers():
            (d / m.name).write_bytes(tf.extractfile(m).read())
    o1, o2 = tmp_path / "o1", tmp_path / "o2"
    n = pipeline.decompress(str(d), str(tmp_path / "all.reads"), order=True)
    rows = (tmp_path / "all.reads").read_bytes().split(b"\n")[:-1]

    def refused(fastq):
        with pytest.raises(McomError):
            pipeline.decompress_order_pe(str(d), str(o1), str(o2), fastq=fastq)
        p = subprocess.run([os.path.join(ROOT, "bin", "decompress"), "--fastq-order-pe" if fastq else "--order-pe", str(d), str(o1), str(o2)], capture_output=True)
        assert p.returncode == 1 and not o1.exists() and not o2.exists()

    refused(False); refused(True)                                      # no pe_order.txt
    (d / "pe_order.txt").write_bytes(b"%d\n" % (n // 2 + 1)); refused(False)
    (d / "pe_order.txt").write_bytes(b"x\n"); refused(False)
    if n % 2 == 0:
        (d / "pe_order.txt").write_bytes(b"%d\n" % (n // 2))
        assert pipeline.decompress_order_pe(str(d), str(o1), str(o2)) == n // 2
        assert o1.read_bytes() == b"".join(r + b"\n" for r in rows[:n // 2]) and o2.read_bytes() == b"".join(r + b"\n" for r in rows[n // 2:])
        o1.unlink(); o2.unlink()
        refused(True)                                                  # no quality members
        # host-coded members: the pair comes back as records, name_2 decoded against name_1
        import qual_cases as qc
        h = n // 2
        quals = qc.synth_quals(3, h, 100)
        a, b = mc.illumina_pair(4, h)
        pa, pb = mc.nc.mixed_plus(a, 1), mc.nc.mixed_plus(b, 2)
        (d / "qual_1.mcq").write_bytes(pipeline.qual_encode(quals)); (d / "qual_2.mcq").write_bytes(pipeline.qual_encode(quals[::-1].copy()))
        (d / "name_2.mcn").write_bytes(pipeline.name_encode(mc.text_of(b, pb), h, mate=mc.text_of(a, pa)))
        refused(True)                                                  # name_2 without name_1
        (d / "name_1.mcn").write_bytes(pipeline.name_encode(mc.text_of(a, pa), h))
        assert pipeline.decompress_order_pe(str(d), str(o1), str(o2), fastq=True) == h
        assert o1.read_bytes() == b"".join(b"@" + x + b"\n" + r + b"\n+" + p + b"\n" + q.tobytes() + b"\n" for x, p, r, q in zip(a, pa, rows[:h], quals))
        assert o2.read_bytes() == b"".join(b"@" + x + b"\n" + r + b"\n+" + p + b"\n" + q.tobytes() + b"\n" for x, p, r, q in zip(b, pb, rows[h:], quals[::-1]))
        o1.unlink(); o2.unlink()
        (d / "qual_2.mcq").unlink(); refused(True)                     # one quality member of two


def test_the_surface_exists():
    import re
    import minicom_amd
    from minicom_amd import pipeline
    from minicom_amd.hip import Context
    h = open(os.path.join(ROOT, "include", "mcom.h")).read()
    hh = open(os.path.join(ROOT, "include", "mcom_host.h")).read()
    lib, hl = minicom_amd.load_library(), pipeline.load_host_library()
    for s in ("mcom_name_encode_mate", "mcom_name_decode_mate", "mcom_name_info_mate"):
        assert re.search(r"\b%s\s*\(" % s, h) and s in minicom_amd.ABI_SYMBOLS and getattr(lib, s)
    for s in ("mcomh_name_encode_mate", "mcomh_name_decode_mate", "mcomh_name_info_mate", "mcomh_name_pack_file_mate", "mcomh_name_unpack_file_mate", "mcomh_fastq_name_member_mate"):
        assert re.search(r"\b%s\s*\(" % s, hh) and s in pipeline.HOST_ABI_SYMBOLS and getattr(hl, s)
    for f in ("name_encode_mate", "name_decode_mate"):
        assert callable(getattr(Context, f))
