"""Read names and '+' lines as `.mcn` members on the GPU (csrc/names.hip) against the independent reference
(tests/name_reference.py) and the host twin: identical bytes, cross decoding, inputs at odd addresses with a canary around the output,
the same hostile members refused, and the FASTQ ends (name text out of FASTQ text, records out of rows and name text, the compare)
against plain Python."""
import numpy as np
import pytest

import name_cases as nc
import name_reference as NR

pytestmark = pytest.mark.gpu
CANARY = 0xA5
F_NAME, F_PLUS, F_LONG = 1, 2, 16


@pytest.fixture(scope="module")
def ctx():
    import minicom_amd
    return minicom_amd.Context(0)


def _dev(b, offset=0):
    """the bytes on the device, `offset` bytes into a fresh buffer (an odd address for offset 1 or 3)"""
    import torch
    buf = torch.full((offset + len(b) + 16,), CANARY, dtype=torch.uint8, device="cuda")
    if len(b):
        buf[offset:offset + len(b)] = torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()
    return buf[offset:offset + len(b)]


def _host(t) -> bytes:
    return t.cpu().numpy().tobytes()


def _decode_in_canary(ctx, member, text_len, offset=3):
    """(text, offsets, canary intact?): the member decoded `offset` bytes into a buffer of canary bytes"""
    import torch
    buf = torch.full((offset + text_len + 64,), CANARY, dtype=torch.uint8, device="cuda")
    out, off = ctx.name_decode(_dev(member, 1), out=buf[offset:offset + max(text_len, 1)])
    b = buf.cpu().numpy()
    return _host(out), off.cpu().numpy(), bool((b[:offset] == CANARY).all() and (b[offset + text_len:] == CANARY).all())


def _offsets(names, plus):
    plus = [b""] * len(names) if plus is None else plus
    return np.concatenate([[0], np.cumsum([len(a) + len(b) + 2 for a, b in zip(names, plus)])]).astype(np.int64)


def _check_case(ctx, names, plus, tag):
    from minicom_amd import pipeline
    text, n = nc.text_of(names, plus), len(names)
    want = NR.ref_encode(text, n, pipeline.bwt_encode, pipeline.rans_encode)
    assert pipeline.name_encode(text, n) == want, tag
    for offset in (1, 3, 0):
        got = _host(ctx.name_encode(_dev(text, offset), n))
        assert got == want, (tag, offset, len(got), len(want))
    members = [want, NR.ref_encode(text, n, pipeline.bwt_encode, pipeline.rans_encode, kind=0)]
    if n:
        members.append(NR.ref_encode(text, n, pipeline.bwt_encode, pipeline.rans_encode, kind=1))
    for m in members:
        back, off, intact = _decode_in_canary(ctx, m, len(text))
        assert back == text and intact, (tag, m[5])
        assert np.array_equal(off, _offsets(names, plus)), (tag, m[5])


@pytest.mark.parametrize("name,names,plus", nc.degenerate(), ids=[c[0] for c in nc.degenerate()])
def test_device_emits_the_reference_and_the_host_bytes(ctx, name, names, plus):
    """every degenerate name text from odd addresses: the reference's bytes and the host twin's; the device decodes both kinds into a
    buffer of canary bytes without touching a byte around the text, and returns the record offsets"""
    _check_case(ctx, names, plus, name)


@pytest.mark.parametrize("gen", [nc.illumina, nc.sra], ids=["illumina", "sra"])
def test_generated_names(ctx, gen):
    names = gen(1, 3000)
    _check_case(ctx, names, None, gen.__name__)
    _check_case(ctx, names[:1000], nc.mixed_plus(names[:1000], 3), gen.__name__ + "+")


def test_many_workgroups(ctx):
    """70 000 records: 274 segments, scans and walks over many workgroups; the host twin's bytes, and the text back"""
    from minicom_amd import pipeline
    names = nc.illumina(7, 70000)
    plus = [b"" if i % 1000 else nm for i, nm in enumerate(names)]
    plus[12345] = b"a literal"
    text = nc.text_of(names, plus)
    want = pipeline.name_encode(text, 70000)
    assert want[5] == 0
    assert _host(ctx.name_encode(_dev(text, 1), 70000)) == want
    back, off, intact = _decode_in_canary(ctx, want, len(text))
    assert back == text and intact and np.array_equal(off, _offsets(names, plus))


def test_other_recs_per_seg_and_noncanonical_members(ctx):
    from minicom_amd import pipeline
    names = nc.illumina(4, 600)
    text = nc.text_of(names, nc.mixed_plus(names, 4))
    for rps in (1, 7, 4096):
        m = NR.ref_encode(text, 600, pipeline.bwt_encode, pipeline.rans_encode, recs_per_seg=rps, kind=0)
        back, _, intact = _decode_in_canary(ctx, m, len(text))
        assert back == text and intact, rps
    for name, member, want in nc.noncanonical():
        back, _, intact = _decode_in_canary(ctx, member, len(want))
        assert back == want and intact, name


def test_hostile_members_are_refused_on_the_device(ctx):
    """one crafted member per refusal rule, truncations and bit flips: the device takes the host twin's decision for every one, and a
    refused member leaves the bytes around the output alone"""
    import torch
    from minicom_amd import McomError, pipeline
    text, n, base = nc.small()
    members = [(name, m, True) for name, _, m in nc.crafted()] + [("cut%d" % i, m, None) for i, m in enumerate(nc.truncations())] + \
              [("flip%d" % i, m, None) for i, m in enumerate(nc.bit_flips(60))]
    for name, m, must_refuse in members:
        try:
            want = pipeline.name_decode(m)
        except McomError:
            want = None
        assert not (must_refuse and want is not None), name
        if len(m) < 96:
            with pytest.raises(McomError):
                ctx.name_decode(_dev(m, 1))
            continue
        room = len(text) + 600
        buf = torch.full((room + 64,), CANARY, dtype=torch.uint8, device="cuda")
        try:
            out, _ = ctx.name_decode(_dev(m, 1), out=buf[3:3 + room])
            got = _host(out)
        except McomError:
            got = None
        assert got == want, name
        b = buf.cpu().numpy()
        assert (b[:3] == CANARY).all() and (b[3 + room:] == CANARY).all(), name


def test_refused_inputs_name_the_record(ctx):
    from minicom_amd import McomError
    for name, text, n, rec in nc.refused_inputs():
        with pytest.raises(McomError) as e:
            ctx.name_encode(_dev(text, 1), n)
        if rec is not None:
            assert "record %d " % (rec + 1) in str(e.value), (name, str(e.value))


def _fastq(names, plus, reads, quals) -> bytes:
    return b"".join(b"@" + a + b"\n" + r + b"\n+" + p + b"\n" + q + b"\n" for a, p, r, q in zip(names, plus, reads, quals))


def _rows(n, L, seed):
    rng = np.random.default_rng(seed)
    reads = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), (n, L))
    quals = rng.integers(33, 74, (n, L), dtype=np.uint8)
    return reads, quals


def test_fastq_names_against_a_python_parse(ctx):
    """the name text and the record offsets of FASTQ text, whole and in pieces of whole records cut at every record boundary of a
    small file; every bad-record kind gives its flag bit and the lowest record"""
    names = nc.illumina(2, 50) + [b"", b"x" * 255, b"@+"]
    names[3] = b"r" * 255
    plus = nc.mixed_plus(names, 6); plus[5] = b"p" * 255
    n = len(names)
    reads, quals = _rows(n, 37, 1)
    rd = [r.tobytes() for r in reads]; ql = [q.tobytes() for q in quals]
    want = nc.text_of(names, plus)
    text, off, bits, first = ctx.fastq_names(_dev(_fastq(names, plus, rd, ql), 1))
    assert (_host(text), bits, first) == (want, 0, None) and np.array_equal(off.cpu().numpy(), _offsets(names, plus))
    for cut in range(0, n + 1, 7):
        a, _, ba, _ = ctx.fastq_names(_dev(_fastq(names[:cut], plus[:cut], rd[:cut], ql[:cut]), 3))
        b, _, bb, _ = ctx.fastq_names(_dev(_fastq(names[cut:], plus[cut:], rd[cut:], ql[cut:]), 1), first_record=cut)
        assert _host(a) + _host(b) == want and ba == 0 and bb == 0, cut
    good = _fastq(names, plus, rd, ql).split(b"\n")
    for kind, line, repl, bit in (("no @", 4 * 9, b"X" + names[9], F_NAME), ("empty @ line", 4 * 9, b"", F_NAME), ("no +", 4 * 11 + 2, b"-", F_PLUS),
                                  ("name of 256", 4 * 13, b"@" + b"n" * 256, F_LONG), ("plus of 256", 4 * 13 + 2, b"+" + b"n" * 256, F_LONG)):
        lines = list(good); lines[line] = repl
        lines[4 * 30] = b"no at either"                                    # a later bad record: the lowest one is reported
        text, off, bits, first = ctx.fastq_names(_dev(b"\n".join(lines), 1), first_record=1000)
        assert bits == (bit | F_NAME) and first == 1000 + line // 4, (kind, bits, first)


def test_fastq_emit_named_against_python(ctx):
    """records out of rows and a decoded name text: whole, and from a first record in the middle; rows at a pitch"""
    import torch
    from minicom_amd import pipeline
    names = nc.sra(5, 300) + [b"", b"y" * 255]
    plus = nc.mixed_plus(names, 8); plus[-1] = b"z" * 255
    n, L = len(names), 41
    reads, quals = _rows(n, L, 2)
    want = _fastq(names, plus, [r.tobytes() for r in reads], [q.tobytes() for q in quals])
    text, off = ctx.name_decode(_dev(pipeline.name_encode(nc.text_of(names, plus), n), 1))
    d_reads = torch.from_numpy(np.pad(reads, ((0, 0), (0, 7)))).cuda()[:, :L]
    d_quals = torch.from_numpy(quals).cuda()
    assert _host(ctx.fastq_emit_named(d_reads, d_quals, text, off)) == want
    first = 129
    skip = sum(len(a) + len(p) + 2 * L + 6 for a, p in zip(names[:first], plus[:first]))
    assert _host(ctx.fastq_emit_named(d_reads[first:], d_quals[first:], text, off, first=first)) == want[skip:]
    assert _host(ctx.fastq_emit_named(d_reads[first:first + 1], d_quals[first:first + 1], text, off, first=first)) == want[skip:skip + len(names[first]) + len(plus[first]) + 2 * L + 6]


def test_name_compare(ctx):
    """two name texts record against record: identical, one name changed, one '+' text changed, lengths changed"""
    import torch
    names = nc.illumina(9, 5000)
    plus = nc.mixed_plus(names, 1)
    a = ctx.fastq_names(_dev(_fastq(names, plus, [b"A"] * 5000, [b"I"] * 5000), 1))
    assert ctx.name_compare(a[0], a[1], a[0], a[1]) == (0, None)
    for change in ("name", "plus", "longer"):
        n2, p2 = list(names), list(plus)
        if change == "name":
            n2[4321] = n2[4321][:-1] + b"X"; n2[77] = b"other"; want = (2, 77)
        elif change == "plus":
            p2[2500] = b"changed"; want = (1, 2500)
        else:
            n2[10] = n2[10] + b"!"; want = (1, 10)
        b = ctx.fastq_names(_dev(_fastq(n2, p2, [b"A"] * 5000, [b"I"] * 5000), 3))
        assert ctx.name_compare(a[0], a[1], b[0], b[1]) == want, change


# ---- the product path: FASTQ file -> name.mcn -> archive -> FASTQ, and -c ---------------------------------------------------------------
def test_pieces_cut_a_record_at_every_position(tmp_path):
    """mcomh_fastq_names_to_device with pieces of every size from one record to two: the end of a piece falls on every byte of a
    record, the unfinished record is carried in front of the next piece, and the name text is the Python parse's every time"""
    from minicom_amd import pipeline
    names = [b"read%d/%d x" % (i, i * 7) for i in range(40)]
    names[5] = b""; names[9] = b"y" * 255
    plus = nc.mixed_plus(names, 2)
    recs = [b"@" + a + b"\nACGTACGTAC\n+" + p + b"\nIIIIIIIIII\n" for a, p in zip(names, plus)]
    (tmp_path / "p.fastq").write_bytes(b"".join(recs))
    want = nc.text_of(names, plus)
    longest = max(len(r) for r in recs)
    for piece in range(longest + 1, 2 * longest + 2):
        assert pipeline.fastq_names(str(tmp_path / "p.fastq"), piece_bytes=piece) == (want, 40), piece
    assert pipeline.fastq_names(str(tmp_path / "p.fastq")) == (want, 40)


def test_fastq_name_member_on_the_device(tmp_path):
    """mcomh_fastq_name_member on GPU 0 (`minicom -N -G`, `mcomz e --fastq-names --gpu`): the host twin's member; every bad-record kind
    is an error that names the record, by the library and by mcomz, and leaves no file"""
    import os
    import subprocess
    from minicom_amd import McomError, pipeline
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = nc.illumina(3, 2000)
    plus = nc.mixed_plus(names, 5)
    recs = [b"@" + a + b"\nACGT\n+" + p + b"\nIIII\n" for a, p in zip(names, plus)]
    (tmp_path / "g.fastq").write_bytes(b"".join(recs))
    assert pipeline.fastq_name_member(str(tmp_path / "g.fastq"), str(tmp_path / "host.mcn")) == 2000
    assert pipeline.fastq_name_member(str(tmp_path / "g.fastq"), str(tmp_path / "gpu.mcn"), device=0) == 2000
    assert (tmp_path / "gpu.mcn").read_bytes() == (tmp_path / "host.mcn").read_bytes() == pipeline.name_encode(nc.text_of(names, plus), 2000)
    out = tmp_path / "never.mcn"
    for tag, rec, repl in (("no @", 17, b"X" + recs[17][1:]), ("no +", 30, recs[30].replace(b"\n+", b"\n-", 1)), ("256", 40, b"@" + b"n" * 256 + b"\nACGT\n+\nIIII\n")):
        bad = list(recs); bad[rec] = repl
        (tmp_path / "bad.fastq").write_bytes(b"".join(bad))
        with pytest.raises(McomError) as e:
            pipeline.fastq_name_member(str(tmp_path / "bad.fastq"), str(out), device=0)
        assert "record %d " % (rec + 1) in str(e.value), (tag, str(e.value))
        p = subprocess.run([os.path.join(root, "bin", "mcomz"), "e", "--fastq-names", "--gpu", str(tmp_path / "bad.fastq"), str(out)], capture_output=True, text=True)
        assert p.returncode == 1 and "record %d " % (rec + 1) in p.stderr and not out.exists(), tag


def _minicom(args, cwd):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run(["bash", os.path.join(root, "bin", "minicom")] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    return p.returncode, p.stdout.decode(errors="replace")


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    """3000 x 100 synthetic reads with Illumina-style names and mixed '+' lines as X.fastq, and `minicom -r X.fastq -p -Q -N -G`"""
    import qual_cases as qc
    from minicom_amd import synth
    d = tmp_path_factory.mktemp("n_e2e")
    reads = synth.synth_reads(1002, 3000, 100)
    quals = qc.synth_quals(7, 3000, 100)
    names = nc.illumina(12, 3000)
    plus = nc.mixed_plus(names, 12)
    text = _fastq(names, plus, [r.tobytes() for r in reads], [q.tobytes() for q in quals])
    (d / "X.fastq").write_bytes(text)
    rc, out = _minicom(["-r", "X.fastq", "-p", "-Q", "-N", "-G", "-t", "2"], d)
    assert rc == 0, out[-3000:]
    return d, names, plus, reads, quals, text


def test_end_to_end_gives_the_input_file_back(e2e, tmp_path):
    """-d with and without -G: X_dec.fastq is X.fastq; the archive carries name.mcn; container.decompress_file agrees on both routes"""
    import os
    import tarfile
    from minicom_amd import container
    d, names, plus, reads, quals, text = e2e
    arc = d / "X_comp_order.minicom"
    with tarfile.open(arc) as t:
        assert {"qual.mcq", "name.mcn"} <= {os.path.basename(m.name) for m in t.getmembers()}
    for flags in (["-G"], []):
        (tmp_path / "X_comp_order.minicom").write_bytes(arc.read_bytes())
        rc, out = _minicom(["-d", "X_comp_order.minicom"] + flags, tmp_path)
        assert rc == 0, out[-3000:]
        assert (tmp_path / "X_comp_order_dec.fastq").read_bytes() == text, flags
        (tmp_path / "X_comp_order_dec.fastq").unlink()
    assert container.decompress_file(str(arc), str(tmp_path / "c_gpu.fastq"), device=0) == 3000 and (tmp_path / "c_gpu.fastq").read_bytes() == text
    assert container.decompress_file(str(arc), str(tmp_path / "c_host.fastq")) == 3000 and (tmp_path / "c_host.fastq").read_bytes() == text


def test_minicom_c_holds_names_and_plus_lines(e2e, tmp_path):
    """-d -c X.fastq: 0 with three checks identical; 2 against a copy with one name changed, 2 against one with one '+' text changed; the
    record is named; nothing is left behind; container.verify_file reports the same"""
    from minicom_amd import container
    d, names, plus, reads, quals, text = e2e
    (tmp_path / "a.minicom").write_bytes((d / "X_comp_order.minicom").read_bytes())
    rc, out = _minicom(["-d", "a.minicom", "-c", str(d / "X.fastq")], tmp_path)
    assert rc == 0 and out.count("identical") == 3, out[-3000:]
    rd = [r.tobytes() for r in reads]; ql = [q.tobytes() for q in quals]
    n2 = list(names); n2[1500] = n2[1500][:-1] + b"X"
    p2 = list(plus); p2[2222] = b"another text"
    (tmp_path / "name.fastq").write_bytes(_fastq(n2, plus, rd, ql))
    (tmp_path / "plus.fastq").write_bytes(_fastq(names, p2, rd, ql))
    rc, out = _minicom(["-d", "a.minicom", "-c", "name.fastq"], tmp_path)
    assert rc == 2 and "record 1500" in out, out[-3000:]
    rc, out = _minicom(["-d", "a.minicom", "-c", "plus.fastq"], tmp_path)
    assert rc == 2 and "record 2222" in out, out[-3000:]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a.minicom", "name.fastq", "plus.fastq"]
    rep = container.verify_file(str(tmp_path / "a.minicom"), str(tmp_path / "name.fastq"))
    assert not rep["identical"] and rep["quality"]["identical"] and rep["names"]["n_input"] == rep["names"]["n_archive"] == 3000
    assert rep["names"]["differing"] == 1 and rep["names"]["first_diff"] == 1500


def test_without_N_the_archive_is_as_before(e2e, tmp_path):
    """the same file through `-p -Q -G` without -N: no name.mcn, and -d gives @1 .. with bare '+' lines"""
    import os
    import tarfile
    import qual_cases as qc
    from minicom_amd import container
    d, names, plus, reads, quals, text = e2e
    (tmp_path / "X.fastq").write_bytes(text)
    rc, out = _minicom(["-r", "X.fastq", "-p", "-Q", "-G", "-t", "2"], tmp_path)
    assert rc == 0, out[-3000:]
    with tarfile.open(tmp_path / "X_comp_order.minicom") as t:
        assert "name.mcn" not in [os.path.basename(m.name) for m in t.getmembers()]
    rc, out = _minicom(["-d", "X_comp_order.minicom", "-G"], tmp_path)
    assert rc == 0 and (tmp_path / "X_comp_order_dec.fastq").read_bytes() == qc.fastq_bytes(reads, quals), out[-3000:]
    sizes = container.compress_fastq(str(tmp_path / "X.fastq"), str(tmp_path / "c.minicom"), order=True, quality=True, names=True, codec="rans", device=0, threads=2)
    assert sizes["name.mcn"] > 0 and container.decompress_file(str(tmp_path / "c.minicom"), str(tmp_path / "c.fastq"), device=0) == 3000
    assert (tmp_path / "c.fastq").read_bytes() == text
