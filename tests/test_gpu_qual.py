"""Quality values as `.mcq` members on the GPU (csrc/qual.hip) against the independent reference
(tests/qual_reference.py) and the host twin: identical bytes, cross decoding, rows at a pitch and at odd addresses with a canary around
the output, the same hostile members refused, and the exact counts of the counting kernel on both of its paths."""
import numpy as np
import pytest

import qual_cases as qc
import qual_reference as QR

pytestmark = pytest.mark.gpu
CANARY = 0xA5


@pytest.fixture(scope="module")
def ctx():
    import minicom_amd
    return minicom_amd.Context(0)


def _dev(b):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda() if len(b) else torch.empty(0, dtype=torch.uint8, device="cuda")


def _host(t) -> bytes:
    return t.cpu().numpy().tobytes()


def _pitched(q, pitch, offset):
    """(buffer, view): the matrix on the device with rows `pitch` apart, the first one `offset` bytes into a buffer of canary bytes"""
    import torch
    n, L = q.shape
    buf = torch.full((offset + max(n, 1) * pitch + 64,), CANARY, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + max(n, 1) * pitch].view(max(n, 1), pitch)[:n, :L]
    if n:
        view.copy_(torch.from_numpy(np.array(q, dtype=np.uint8)).cuda())
    return buf, view


def _canary_intact(buf, n, L, pitch, offset) -> bool:
    b = buf.cpu().numpy().copy()
    for r in range(n):
        b[offset + r * pitch:offset + r * pitch + L] = CANARY
    return bool((b == CANARY).all())


@pytest.mark.parametrize("name,q", qc.degenerate(), ids=[c[0] for c in qc.degenerate()])
def test_device_emits_the_reference_and_the_host_bytes(ctx, name, q):
    """every degenerate matrix under the choice and every forced model id, rows at pitch L and L + 1 from odd addresses: the reference's
    bytes and the host twin's; the device decodes both into a pitched table without touching a byte around the rows"""
    from minicom_amd import pipeline
    n, L = q.shape
    rans = pipeline.rans_encode(np.ascontiguousarray(q).tobytes())
    for model in (None, 0, 1, 2, 3, 4, "rans"):
        want = QR.ref_encode(q, model=model, rans_member=rans)
        assert pipeline.qual_encode(q, model) == want, (name, model)
        for pitch, offset in ((L, 1), (L + 1, 3), (L, 0)):
            _, rows = _pitched(q, pitch, offset)
            got = _host(ctx.qual_encode(rows, model))
            assert got == want, (name, model, pitch, offset, len(got), len(want))
        for pitch, offset in ((L, 1), (L + 1, 3)):
            buf, out = _pitched(np.zeros_like(q), pitch, offset)
            if n:
                out.fill_(CANARY)
            back = ctx.qual_decode(_dev(want), out=buf[offset:offset + max(n, 1) * pitch].view(max(n, 1), pitch))
            assert tuple(back.shape) == (n, L) and np.array_equal(back.cpu().numpy(), q), (name, model, pitch)
            assert _canary_intact(buf, n, L, pitch, offset), (name, model, pitch)


def test_more_than_one_workgroup(ctx):
    """265 segments (two workgroups of the coder, the second one partly idle): the host twin's bytes and back, model 3 (tables in LDS)
    and model 4 of 36 values (tables in global memory)"""
    from minicom_amd import pipeline
    q = qc.synth_quals(6, 5290, 100)
    for model in (None, 3, 4):
        host = pipeline.qual_encode(q, model)
        _, rows = _pitched(q, 101, 5)
        dev = ctx.qual_encode(rows, model)
        assert _host(dev) == host, model
        buf, _ = _pitched(np.zeros_like(q), 101, 7)
        back = ctx.qual_decode(dev, out=buf[7:7 + 5290 * 101].view(5290, 101))
        assert np.array_equal(back.cpu().numpy(), q), model
        assert _canary_intact(buf, 5290, 100, 101, 7), model


@pytest.mark.parametrize("rps", [1, 3, 64, 327])
def test_device_decodes_reference_members_at_other_rows_per_seg(ctx, rps):
    q = qc.synth_quals(9, 330, 100)
    for model in (2, 4):
        m = QR.ref_encode(q, model=model, rows_per_seg=rps)
        assert np.array_equal(ctx.qual_decode(_dev(m)).cpu().numpy(), q), (rps, model)


def _decisions(ctx, member, shape):
    """(host, device): the decoded matrix or None; the device decodes between canaries"""
    from minicom_amd import McomError, pipeline
    try:
        want = pipeline.qual_decode(member)
    except McomError:
        want = None
    n, L = shape
    buf, _ = _pitched(np.zeros(shape, np.uint8), L, 1)
    msg = ""
    try:
        got = ctx.qual_decode(_dev(member), out=buf[1:1 + n * L].view(n, L)).cpu().numpy()
    except McomError as e:
        got, msg = None, str(e)
    b = buf.cpu().numpy()
    assert (b[0] == CANARY) and (b[1 + n * L:] == CANARY).all(), "the decoder left its table"
    return want, got, msg


def test_hostile_corpus_gets_the_host_decision(ctx):
    """every truncation, 200 bit flips and one crafted member per refusal rule: the device accepts exactly what the host twin accepts,
    what it accepts is what the host decodes, the rules that only a kernel can judge come back with the flag word, and no byte outside
    the output table changes"""
    q, base = qc.small()
    want, got, _ = _decisions(ctx, base, q.shape)
    assert np.array_equal(want, q) and np.array_equal(got, q)
    for member in qc.truncations() + qc.bit_flips():
        want, got, _ = _decisions(ctx, member, q.shape)
        assert (want is None) == (got is None) and (want is None or np.array_equal(want, got))
    for name, rule, member in qc.crafted():
        want, got, msg = _decisions(ctx, member, q.shape)
        assert want is None and got is None, name
        if rule in ("run<4", "state", "slot", "exhausted", "end"):
            assert "flag 0x" in msg, (name, msg)


@pytest.mark.parametrize("kind", ["A4", "A41"])
def test_counts_of_the_counting_kernel(ctx, kind):
    """mcom_test_qual_hist on 3000 x 100 rows against numpy: 4 values (counters in LDS) and 41 values (the global table)"""
    q = qc.synth_quals(12, 3000, 100, binned=True) if kind == "A4" else qc._alphabet(13, 3000, 100, range(40, 81))
    amap, vals = QR.ref_alphabet(q)
    for pitch, offset in ((100, 0), (101, 3)):
        _, rows = _pitched(q, pitch, offset)
        got_map, A, counts = ctx.qual_test_hist(rows)
        assert got_map == amap and A == len(vals) == (4 if kind == "A4" else 41)
        assert np.array_equal(counts.cpu().numpy(), QR.ref_hist(q, vals)), (kind, pitch)


# ---- FASTQ text <-> rows, and `minicom -Q` end to end ----------------------------------------------------------------------------------
def _parse(text: bytes):
    """the quality lines of a four-line FASTQ text, by Python"""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return np.array([np.frombuffer(l, dtype=np.uint8) for l in lines[3::4]])


def test_quality_rows_of_the_tricky_fastq(ctx, tmp_path):
    """quality lines that begin with '@' and '+': the kernel over one text, then the file route with pieces of 300 bytes asked for (raised to the
    documented minimum 4 (2 L + 64) = 552: about 6.6 records of 83 bytes to a piece, so records straddle), with the last newline missing, and through gzip"""
    import gzip
    from minicom_amd import pipeline
    reads, quals, text = qc.tricky_fastq()
    assert np.array_equal(_parse(text), quals)
    rows, flag, first_bad = ctx.fastq_qualities(_dev(text), 37)
    assert flag == 0 and first_bad is None and np.array_equal(rows.cpu().numpy(), quals)
    _, rows2 = _pitched(np.zeros((125, 37), np.uint8), 40, 3)               # into a pitched table, behind five rows of another piece
    got, flag, _ = ctx.fastq_qualities(_dev(text), 37, first_record=5, out=rows2)
    assert flag == 0 and np.array_equal(got.cpu().numpy()[5:], quals)
    (tmp_path / "t.fastq").write_bytes(text)
    (tmp_path / "nonl.fastq").write_bytes(text[:-1])
    with gzip.open(tmp_path / "t.fastq.gz", "wb") as f:
        f.write(text)
    for name, piece in (("t.fastq", 0), ("t.fastq", 300), ("nonl.fastq", 300), ("nonl.fastq", 0), ("t.fastq.gz", 300)):
        got = pipeline.fastq_qualities(str(tmp_path / name), 37, piece_bytes=piece)
        assert np.array_equal(got.cpu().numpy(), quals), (name, piece)
    (tmp_path / "empty.fastq").write_bytes(b"")
    assert tuple(pipeline.fastq_qualities(str(tmp_path / "empty.fastq"), 37).shape) == (0, 37)


def test_bad_fastq_files_are_refused_and_the_first_bad_record_is_named(ctx, tmp_path):
    """a CRLF line, a short quality line, a byte 127, a missing '@', a missing '+', a file that ends inside a record: an error that names
    the record (from 1), with one piece and with small pieces (300 bytes asked for, 552 used); the kernel's flag bits say which rule"""
    from minicom_amd import McomError, pipeline
    reads, quals, text = qc.tricky_fastq()
    recs = [r + b"\n" for r in text[:-1].split(b"\n")]
    rec = lambda i: b"".join(recs[4 * i:4 * i + 4])
    def with_record(i, new):
        return b"".join(rec(k) if k != i else new for k in range(len(recs) // 4))
    q17 = quals[17].tobytes(); r17 = reads[17].tobytes()
    bad = {"crlf": (with_record(17, b"@18\n" + r17 + b"\n+\n" + q17 + b"\r\n"), 4), "short": (with_record(17, b"@18\n" + r17 + b"\n+\n" + q17[:-1] + b"\n"), 4),
           "127": (with_record(17, b"@18\n" + r17 + b"\n+\n" + q17[:5] + b"\x7f" + q17[6:] + b"\n"), 8), "space": (with_record(17, b"@18\n" + r17 + b"\n+\n" + b" " + q17[1:] + b"\n"), 8),
           "no @": (with_record(17, b"18\n" + r17 + b"\n+\n" + q17 + b"\n"), 1), "no +": (with_record(17, b"@18\n" + r17 + b"\n-\n" + q17 + b"\n"), 2),
           "long read": (with_record(17, b"@18\n" + r17 + b"A\n+\n" + q17 + b"\n"), 4)}
    for name, (t, bits) in bad.items():
        rows, flag, first_bad = ctx.fastq_qualities(_dev(t), 37)
        assert flag == bits and first_bad == 17, (name, flag, first_bad)
        assert np.array_equal(rows.cpu().numpy()[:17], quals[:17]) and np.array_equal(rows.cpu().numpy()[18:], quals[18:]), name
        (tmp_path / "bad.fastq").write_bytes(t)
        for piece in (0, 300):
            with pytest.raises(McomError, match=r"record 18 "):
                pipeline.fastq_qualities(str(tmp_path / "bad.fastq"), 37, piece_bytes=piece)
    (tmp_path / "cut.fastq").write_bytes(text[:-60])
    with pytest.raises(McomError, match=r"ends inside record 120"):
        pipeline.fastq_qualities(str(tmp_path / "cut.fastq"), 37, piece_bytes=300)


def test_fastq_to_member_on_the_device_checks_every_record(ctx, tmp_path):
    """mcomh_fastq_quality_member on GPU 0 (what `minicom -Q -G` runs, `mcomz e --fastq-qual L --gpu`): the host twin's member; every
    bad file of the host test -- the short line balanced by a long one among them -- is refused with the same record named, by the
    library, by mcomz and by `minicom -r X.fastq -p -Q -G`, which leaves no archive"""
    import os
    import subprocess
    from minicom_amd import McomError, pipeline
    reads, quals, text = qc.tricky_fastq()
    (tmp_path / "t.fastq").write_bytes(text)
    assert pipeline.fastq_quality_member(str(tmp_path / "t.fastq"), 37, str(tmp_path / "h.mcq")) == 120
    assert pipeline.fastq_quality_member(str(tmp_path / "t.fastq"), 37, str(tmp_path / "g.mcq"), device=0) == 120
    assert (tmp_path / "g.mcq").read_bytes() == (tmp_path / "h.mcq").read_bytes() == pipeline.qual_encode(quals)
    for name, t in qc.bad_fastqs().items():
        (tmp_path / "bad.fastq").write_bytes(t)
        for device in (None, 0):
            with pytest.raises(McomError, match=r"record 18 "):
                pipeline.fastq_quality_member(str(tmp_path / "bad.fastq"), 37, str(tmp_path / "bad.mcq"), device=device)
            assert not (tmp_path / "bad.mcq").exists(), (name, device)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([os.path.join(root, "bin", "mcomz"), "e", "--fastq-qual", "37", "--gpu", "bad.fastq", "bad.mcq"], cwd=tmp_path, capture_output=True, text=True)
    assert p.returncode == 1 and "record 18 " in p.stderr and not (tmp_path / "bad.mcq").exists(), p.stderr
    (tmp_path / "bad.fastq").write_bytes(qc.bad_fastqs()["127"])             # (one the read parser has no quarrel with: its reads are in order)
    rc, out = _minicom(["-r", "bad.fastq", "-p", "-Q", "-G", "-t", "1"], tmp_path)
    assert rc == 1 and "record 18 " in out and "cannot be kept" in out, out[-3000:]
    assert not list(tmp_path.glob("*.minicom")) and not list(tmp_path.glob("*_comp*"))


@pytest.mark.parametrize("L", [1, 100, 256])
def test_fastq_emit_across_the_decade_boundaries(ctx, L):
    """records 0 .. 1100 (names @1 .. @1101: the boundaries 9/10, 99/100 and 999/1000), whole and from a `first` in the middle of a
    decade, rows at a pitch: the bytes Python writes"""
    rng = np.random.default_rng(L)
    n = 1101
    reads = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, (n, L))]
    quals = rng.integers(33, 127, (n, L)).astype(np.uint8)
    want = qc.fastq_bytes(reads, quals)
    _, d_reads = _pitched(reads, L + 1, 1)
    _, d_quals = _pitched(quals, L, 3)
    assert _host(ctx.fastq_emit(d_reads, d_quals)) == want
    ends = np.cumsum([2 * L + 6 + len(str(i + 1)) for i in range(n)])
    for first, count in ((57, 1044), (995, 10), (9, 1), (1100, 1), (300, 0)):
        got = _host(ctx.fastq_emit(d_reads[first:first + count], d_quals[first:first + count], first=first))
        lo = int(ends[first - 1]) if first else 0
        assert got == want[lo:int(ends[first + count - 1]) if count else lo], (first, count)


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    """3000 x 100 synthetic reads with synth_quals qualities as a FASTQ file named @1 .. with bare + lines, and its -p -Q archive"""
    from minicom_amd import container, synth
    d = tmp_path_factory.mktemp("q_e2e")
    reads = synth.synth_reads(1002, 3000, 100)
    quals = qc.synth_quals(7, 3000, 100)
    text = qc.fastq_bytes(reads, quals)
    (d / "in.fastq").write_bytes(text)
    sizes = container.compress_fastq(str(d / "in.fastq"), str(d / "in.minicom"), order=True, quality=True, codec="rans", device=0, threads=2)
    return d, reads, quals, text, sizes


def test_end_to_end_archive_gives_the_fastq_back(e2e):
    from minicom_amd import container
    d, reads, quals, text, sizes = e2e
    assert sizes["n_reads"] == 3000 and 0 < sizes["qual.mcq"] < quals.size // 2
    assert container.decompress_file(str(d / "in.minicom"), str(d / "gpu.fastq"), device=0) == 3000
    assert (d / "gpu.fastq").read_bytes() == text
    assert container.decompress_file(str(d / "in.minicom"), str(d / "host.fastq")) == 3000
    assert (d / "host.fastq").read_bytes() == text


def test_end_to_end_verify(e2e):
    from minicom_amd import container
    d, reads, quals, text, _ = e2e
    rep = container.verify_file(str(d / "in.minicom"), str(d / "in.fastq"))
    assert rep["identical"] and rep["quality"]["identical"] and rep["quality"]["n_input"] == rep["quality"]["n_archive"] == 3000
    q2 = quals.copy(); q2[1234, 56] = q2[1234, 56] + 1 if q2[1234, 56] < 126 else 125
    (d / "other.fastq").write_bytes(qc.fastq_bytes(reads, q2))
    rep = container.verify_file(str(d / "in.minicom"), str(d / "other.fastq"))
    assert not rep["identical"] and rep["differing"] == 0                      # the reads are the same ...
    assert not rep["quality"]["identical"] and rep["quality"]["differing"] == 1 and rep["quality"]["first_diff"] == 1234


def _minicom(args, cwd):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run(["bash", os.path.join(root, "bin", "minicom")] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    return p.returncode, p.stdout.decode(errors="replace")


def test_minicom_Q_command_line(e2e, tmp_path):
    """bin/minicom -r X.fastq -p -Q -G, then -d -G: the archive carries qual.mcq and the same file comes back"""
    import os
    import tarfile
    d, reads, quals, text, _ = e2e
    (tmp_path / "s.fastq").write_bytes(text)
    rc, out = _minicom(["-r", "s.fastq", "-p", "-Q", "-G", "-t", "2"], tmp_path)
    assert rc == 0, out[-3000:]
    with tarfile.open(tmp_path / "s_comp_order.minicom") as t:
        assert "qual.mcq" in [os.path.basename(m.name) for m in t.getmembers()]
    rc, out = _minicom(["-d", "s_comp_order.minicom", "-G"], tmp_path)
    assert rc == 0, out[-3000:]
    assert (tmp_path / "s_comp_order_dec.fastq").read_bytes() == text


def test_minicom_c_holds_the_quality_lines_too(e2e, tmp_path):
    """bin/minicom -d X.minicom -c X.fastq on a -Q archive: both checks run; identical (exit 0) for the input, different (exit 2) with
    the line named for a FASTQ with one other quality byte; nothing is left behind"""
    d, reads, quals, text, _ = e2e
    (tmp_path / "in.minicom").write_bytes((d / "in.minicom").read_bytes())
    rc, out = _minicom(["-d", "in.minicom", "-c", str(d / "in.fastq")], tmp_path)
    assert rc == 0 and out.count("identical") == 2, out[-3000:]
    q2 = quals.copy(); q2[77, 0] = 33 if q2[77, 0] != 33 else 34
    (tmp_path / "o.fastq").write_bytes(qc.fastq_bytes(reads, q2))
    rc, out = _minicom(["-d", "in.minicom", "-c", "o.fastq"], tmp_path)
    assert rc == 2 and "line 77" in out, out[-3000:]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.minicom", "o.fastq"]
