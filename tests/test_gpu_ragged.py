"""Reads of differing lengths on the GPU (csrc/ragged.hip): each device call against the split in plain Python
(tests/ragged_cases.py), the file calls against their host twins byte for byte, text -> split -> records as an exact round trip, and
`bin/minicom -p -V` end to end: round trips on both decoders and through -z, -d -c, the one-length archive, the refusals."""
import os
import subprocess

import numpy as np
import pytest

import ragged_cases as rc

pytestmark = pytest.mark.gpu
CANARY = 0xA5
F_LENGTH, F_CHAR, F_BASE = 4, 8, 32
CASES = rc.cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _slots(want):
    import torch
    return torch.from_numpy(np.array(want, dtype=np.uint64).view(np.int64).copy()).cuda()


def _pieces(recs, step):
    """(first record, text) of consecutive groups of `step` records"""
    return [(k, rc.text_of(recs[k:k + step])) for k in range(0, len(recs), step)]


def _rows(rows, L):
    import torch
    m = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), L) if rows else np.zeros((0, max(L, 1)), dtype=np.uint8)
    return torch.from_numpy(m.copy()).cuda()


@pytest.mark.parametrize("name,recs", CASES, ids=rc.case_ids())
def test_lengths_histogram_and_slots(ctx, name, recs):
    """len.bin, the histogram (kept on the device across pieces of seven records, from odd addresses) and the modal length; then the
    slots and the three totals"""
    import torch
    want = rc.split(recs)
    n = len(recs)
    lens = torch.full((n + 16,), CANARY, dtype=torch.uint8, device="cuda")
    hist = torch.zeros(256, dtype=torch.int64, device="cuda")
    for first, text in _pieces(recs, 7 if n < 100 else 1777):
        _, _, bits, bad = ctx.fastq_lengths(_dev(text, 1 + first % 3), first, lens, hist)
        assert (bits, bad) == (0, None), (name, first, bits, bad)
    assert _host(lens[:n]) == want["len_bin"]
    assert (lens[n:].cpu().numpy() == CANARY).all()
    h = hist.cpu().numpy()
    assert h.tolist() == np.bincount(np.frombuffer(want["len_bin"], dtype=np.uint8), minlength=256).tolist()
    assert max(range(256), key=lambda b: (h[b], b)) + 1 == want["L"]
    slot, n_even, n_odd, odd_bytes = ctx.ragged_index(lens[:n].clone(), want["L"])
    assert (n_even, n_odd, odd_bytes) == (want["n_even"], want["n_odd"], len(want["odd_seq"]))
    assert slot.cpu().numpy().view(np.uint64).tolist() == want["slots"]


@pytest.mark.parametrize("which", [1, 3])
@pytest.mark.parametrize("name,recs", CASES, ids=rc.case_ids())
def test_rows_and_odd_text(ctx, name, recs, which):
    """the even rows and the odd text of the sequence lines and of the quality lines, gathered piece by piece into tables with canary
    bytes behind every row and around the odd text"""
    import torch
    want = rc.split(recs)
    L, n_even = want["L"], want["n_even"]
    lens, slot = _dev(want["len_bin"]), _slots(want["slots"])
    rows = torch.full((n_even, L + 5), CANARY, dtype=torch.uint8, device="cuda")
    odd_buf = torch.full((len(want["odd_seq"]) + 32,), CANARY, dtype=torch.uint8, device="cuda")
    odd = odd_buf[16:16 + len(want["odd_seq"])]
    for first, text in _pieces(recs, 5 if len(recs) < 100 else 1234):
        bits, bad = ctx.fastq_ragged_rows(_dev(text, 3), which, L, lens, slot, rows, odd, first)
        assert (bits, bad) == (0, None), (name, first, bits, bad)
    got = rows.cpu().numpy()
    assert [r.tobytes() for r in got[:, :L]] == want["even_seq" if which == 1 else "even_qual"]
    assert (got[:, L:] == CANARY).all()
    assert _host(odd) == want["odd_seq" if which == 1 else "odd_qual"]
    b = odd_buf.cpu().numpy()
    assert (b[:16] == CANARY).all() and (b[16 + len(want["odd_seq"]):] == CANARY).all()


@pytest.mark.parametrize("name,recs", CASES, ids=rc.case_ids())
def test_emit_gives_the_text_back(ctx, name, recs):
    """split -> records: with a name text the input byte for byte, without one `@<i+1>` and a bare '+', without qualities one read per
    line; and a range of records in the middle is that part of the whole"""
    import torch
    want = rc.split(recs)
    L, n = want["L"], len(recs)
    lens, slot = _dev(want["len_bin"]), _slots(want["slots"])
    reads, quals = _rows(want["even_seq"], L), _rows(want["even_qual"], L)
    odd_seq, odd_qual = _dev(want["odd_seq"], 1), _dev(want["odd_qual"], 3)
    nt, off = rc.name_text(recs)
    d_off = torch.tensor(off, dtype=torch.int64, device="cuda")
    assert _host(ctx.fastq_emit_ragged(L, lens, slot, reads, odd_seq, quals, odd_qual, _dev(nt), d_off)) == rc.text_of(recs)
    assert _host(ctx.fastq_emit_ragged(L, lens, slot, reads, odd_seq, quals, odd_qual)) == rc.numbered(recs)
    assert _host(ctx.fastq_emit_ragged(L, lens, slot, reads, odd_seq)) == rc.reads_only(recs)
    a, c = n // 3, max(n // 2, 1)
    part = _host(ctx.fastq_emit_ragged(L, lens, slot, reads, odd_seq, quals, odd_qual, _dev(nt), d_off, first=a, count=min(c, n - a)))
    assert part == rc.text_of(recs[a:a + c])
    nums = rc.numbered(recs)
    before = len(rc.numbered(recs[:a]))
    part = _host(ctx.fastq_emit_ragged(L, lens, slot, reads, odd_seq, quals, odd_qual, first=a, count=min(c, n - a)))
    assert part == nums[before:before + len(part)] and part.count(b"\n") == 4 * min(c, n - a)


@pytest.mark.parametrize("name,text,first_bad", rc.bad_records(), ids=[c[0] for c in rc.bad_records()])
def test_bad_records_are_flagged(ctx, name, text, first_bad):
    _, _, bits, bad = ctx.fastq_lengths(_dev(text))
    assert bits != 0 and bad == first_bad - 1, (name, bits, bad)
    want = {"length_0": F_LENGTH, "length_257": F_LENGTH, "unequal_lengths": F_LENGTH, "base_outside_ACGTN": F_BASE, "quality_below_33": F_CHAR, "quality_above_126": F_CHAR}[name]
    assert bits == want, (name, bits)


def test_tables_that_disagree_are_flagged_and_nothing_is_written_outside(ctx):
    """a length byte, a slot kind, an even rank and an odd offset that do not fit the text or the tables: the rows call flags the record
    and leaves the canaries alone, the emit call refuses"""
    import torch
    import minicom_amd
    recs = rc.make_records(31, [100, 100, 40, 100, 41, 100])
    want = rc.split(recs)
    L = want["L"]
    text = _dev(rc.text_of(recs))
    reads, quals = _rows(want["even_seq"], L), _rows(want["even_qual"], L)
    odd_seq, odd_qual = _dev(want["odd_seq"]), _dev(want["odd_qual"])

    def tampered(k, len_byte=None, slot=None):
        lb, sl = bytearray(want["len_bin"]), list(want["slots"])
        if len_byte is not None:
            lb[k] = len_byte
        if slot is not None:
            sl[k] = slot
        return _dev(bytes(lb)), _slots(sl)

    for k, kw in ((1, dict(len_byte=98)), (2, dict(len_byte=99)), (3, dict(slot=rc.ODD | 0)), (4, dict(slot=1)), (5, dict(slot=4)), (4, dict(slot=rc.ODD | 41)),
                  (2, dict(slot=rc.ODD | (1 << 40)))):
        lens, slot = tampered(k, **kw)
        rows = torch.full((want["n_even"], L + 3), CANARY, dtype=torch.uint8, device="cuda")
        odd_buf = torch.full((len(want["odd_seq"]) + 32,), CANARY, dtype=torch.uint8, device="cuda")
        bits, bad = ctx.fastq_ragged_rows(text, 1, L, lens, slot, rows, odd_buf[16:16 + len(want["odd_seq"])])
        assert bits == F_LENGTH and bad == k, (k, kw, bits, bad)
        b = odd_buf.cpu().numpy()
        assert (rows.cpu().numpy()[:, L:] == CANARY).all() and (b[:16] == CANARY).all() and (b[16 + len(want["odd_seq"]):] == CANARY).all()
        with pytest.raises(minicom_amd.McomError):
            ctx.fastq_emit_ragged(L, lens, slot, reads, odd_seq, quals, odd_qual)
    # name offsets that do not describe two lines per record
    nt, off = rc.name_text(recs)
    lens, slot = tampered(0)
    for bad_off in (off[:3] + [off[3] - 600] + off[4:], off[:-1] + [off[-1] + 1], [off[0]] + [off[1] - 1] * 1 + off[2:]):
        with pytest.raises(minicom_amd.McomError):
            ctx.fastq_emit_ragged(L, lens, slot, reads, odd_seq, quals, odd_qual, _dev(nt), torch.tensor(bad_off, dtype=torch.int64, device="cuda"))
    assert _host(ctx.fastq_emit_ragged(L, lens, slot, reads, odd_seq, quals, odd_qual, _dev(nt), torch.tensor(off, dtype=torch.int64, device="cuda"))) == rc.text_of(recs)


# ---- the file calls on the GPU: the host twin's bytes, whatever the piece size and the file form ----
MIN_PIECE = 1          # raised to the documented minimum of 2304 bytes: records straddle pieces, odd records lie on both sides of a cut


@pytest.mark.parametrize("name,recs", CASES, ids=rc.case_ids())
def test_file_calls_give_the_host_twins_bytes(tmp_path, name, recs):
    fq = tmp_path / "in.fastq"
    fq.write_bytes(rc.text_of(recs))
    (tmp_path / "gpu").mkdir()
    (tmp_path / "host").mkdir()
    got = rc.split_files(tmp_path / "gpu", fq, device=0, piece_bytes=MIN_PIECE)
    rc.check_against_python(recs, got)
    assert got == rc.split_files(tmp_path / "host", fq)


@pytest.mark.parametrize("form", ["no_final_newline", "gz_one_member", "gz_five_members", "bgzf"])
@pytest.mark.parametrize("name", ["last_odd", "n_17", "n_5000"])
def test_file_forms_on_the_gpu(tmp_path, name, form):
    """a missing last newline, gzip files of one and of several members (zlib's reader), and a BGZF file, which is inflated on the card"""
    from minicom_amd import pipeline
    recs = dict(CASES)[name]
    text = rc.text_of(recs, final_newline=form != "no_final_newline")
    fq = tmp_path / ("in.fastq" if form == "no_final_newline" else "in.fastq.gz")
    if form == "bgzf":
        (tmp_path / "plain").write_bytes(text)
        assert subprocess.run([os.path.join(ROOT, "bin", "mcomz"), "z", str(tmp_path / "plain"), str(fq)]).returncode == 0
    else:
        fq.write_bytes(text if form == "no_final_newline" else rc.gz_members(text, 1 if form == "gz_one_member" else 5))
    rc.check_against_python(recs, rc.split_files(tmp_path, fq, device=0, piece_bytes=MIN_PIECE if form != "bgzf" else 70000))


@pytest.mark.parametrize("name,text,first_bad", rc.bad_records(), ids=[c[0] for c in rc.bad_records()])
def test_file_call_refuses_with_the_host_twins_message(tmp_path, name, text, first_bad):
    from minicom_amd import McomError, pipeline
    fq = tmp_path / "bad.fastq"
    fq.write_bytes(rc.text_of(rc.make_records(3, [100] * 40)) + text)          # a few pieces in front of the bad record
    msgs = []
    for device in (None, 0):
        with pytest.raises(McomError, match=r"record %d is not" % (40 + first_bad)) as e:
            pipeline.fastq_lengths(str(fq), str(tmp_path / "len.bin"), device, MIN_PIECE)
        assert not (tmp_path / "len.bin").exists()
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]


# ---- through bin/minicom ----
MINICOM = os.path.join(ROOT, "bin", "minicom")


def _run(args, cwd):
    return subprocess.run([MINICOM] + [str(a) for a in args], cwd=str(cwd), capture_output=True, text=True)


def _trimmed_records(seed, n=2000, L=100):
    """2 000 reads of L = 100 from the synthetic genome, about one in ten trimmed to 30 .. 99 bases, a few of lengths 1 and 256"""
    import random
    from minicom_amd import synth
    reads = synth.synth_reads(seed, n, L)
    rng = random.Random(seed)
    lengths = [L if rng.random() >= 0.1 else rng.randrange(30, L) for _ in range(n)]
    for k, l in ((5, 1), (77, 256), (3 * n // 5, 1), (n - 1, 256)):
        lengths[k] = l
    recs = rc.make_records(seed, lengths, n_rate=0.0)
    for i, (nm, s, p, q) in enumerate(recs):
        row = reads[i].tobytes()
        recs[i] = (nm, row[:len(s)] if len(s) <= L else (row * 3)[:len(s)], p, q)
    return recs


@pytest.fixture(scope="module")
def archive(tmp_path_factory):
    """X.fastq and its archive made with -r X.fastq -p -V -Q -N -G"""
    d = tmp_path_factory.mktemp("ragged_cli")
    recs = _trimmed_records(41)
    (d / "X.fastq").write_bytes(rc.text_of(recs))
    p = _run(["-r", "X.fastq", "-p", "-V", "-Q", "-N", "-G"], d)
    assert p.returncode == 0 and (d / "X_comp_order.minicom").exists(), p.stdout + p.stderr
    return d, recs


@pytest.mark.parametrize("flags", [["-G"], ["-G", "-z"], []], ids=["gpu", "gpu_gz", "host"])
def test_round_trip_gives_the_input_file_back(archive, tmp_path, flags):
    """-d -G, -d -G -z after gzip -dc, and -d without -G: X_comp_order_dec.fastq is X.fastq byte for byte"""
    import gzip
    d, recs = archive
    p = _run(["-d", d / "X_comp_order.minicom"] + flags, tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    out = tmp_path / ("X_comp_order_dec.fastq" + (".gz" if "-z" in flags else ""))
    got = gzip.decompress(out.read_bytes()) if "-z" in flags else out.read_bytes()
    assert got == (d / "X.fastq").read_bytes()


@pytest.mark.parametrize("flags", [["-p", "-V", "-G"], ["-p", "-V", "-Q", "-G"]], ids=["reads_only", "numbered"])
def test_reads_only_and_numbered_records(tmp_path, flags):
    """-p -V alone: _dec.reads with one read per line in input order; -p -V -Q: records named @<i+1> with a bare '+'"""
    recs = _trimmed_records(43, n=600)
    name, want = ("X_comp_order_dec.fastq", rc.numbered(recs)) if "-Q" in flags else ("X_comp_order_dec.reads", rc.reads_only(recs))
    (tmp_path / "X.fastq").write_bytes(rc.text_of(recs))
    p = _run(["-r", "X.fastq"] + flags, tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    p = _run(["-d", "X_comp_order.minicom", "-G"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert (tmp_path / name).read_bytes() == want


@pytest.mark.parametrize("change", ["none", "base_in_an_odd_read", "quality_in_an_odd_record", "read_shortened", "records_swapped"])
def test_check_says_identical_and_finds_each_difference(archive, tmp_path, change):
    """-d -c X.fastq: exit status 0 for the input; 2 for one base changed in an odd read, one quality byte changed in an odd record, one read
    shortened by a base, two records of different length swapped"""
    d, recs = archive
    odd = next(i for i, r in enumerate(recs) if 30 <= len(r[1]) < 100)
    even = next(i for i, r in enumerate(recs) if len(r[1]) == 100)
    nm, s, pl, q = recs[odd]
    en, es, ep, eq = recs[even]
    v = list(recs)
    if change == "base_in_an_odd_read":
        v[odd] = (nm, s[:3] + (b"A" if s[3:4] != b"A" else b"C") + s[4:], pl, q)
    if change == "quality_in_an_odd_record":
        v[odd] = (nm, s, pl, q[:5] + (b"5" if q[5:6] != b"5" else b"6") + q[6:])
    if change == "read_shortened":
        v[even] = (en, es[:-1], ep, eq[:-1])
    if change == "records_swapped":
        v[odd], v[even] = v[even], v[odd]
    f = tmp_path / "check.fastq"
    f.write_bytes(rc.text_of(v))
    p = _run(["-d", d / "X_comp_order.minicom", "-c", f], tmp_path)
    assert p.returncode == (0 if change == "none" else 2), (change, p.stdout + p.stderr)
    assert ("DIFFERENT" in p.stdout) == (change != "none"), p.stdout
    assert sorted(x.name for x in tmp_path.iterdir()) == ["check.fastq"]       # -c leaves nothing behind


def _members(archive_path, work):
    """every file of an archive, the packed groups opened: name -> bytes (tar headers carry times, the members do not)"""
    import io
    import tarfile
    out = {}
    with tarfile.open(archive_path) as t:
        for m in t.getmembers():
            if not m.isfile():
                continue
            data, name = t.extractfile(m).read(), os.path.basename(m.name)
            if name.endswith(".rans"):
                (work / name).write_bytes(data)
                assert subprocess.run([os.path.join(ROOT, "bin", "mcomz"), "d", str(work / name), str(work / name[:-5])]).returncode == 0
                data, name = (work / name[:-5]).read_bytes(), name[:-5]
            if name.endswith(".tar"):
                with tarfile.open(fileobj=io.BytesIO(data)) as inner:
                    for im in inner.getmembers():
                        if im.isfile():
                            out[name + "/" + os.path.basename(im.name)] = inner.extractfile(im).read()
            else:
                out[name] = data
    return out


def test_a_file_of_one_length_gives_the_archive_made_without_V(tmp_path):
    recs = rc.make_records(47, [100] * 300, n_rate=0.0)
    from minicom_amd import synth
    reads = synth.synth_reads(47, 300, 100)
    recs = [(nm, reads[i].tobytes(), p, q) for i, (nm, s, p, q) in enumerate(recs)]
    got = {}
    for tag, flags in (("with", ["-V"]), ("without", [])):
        w = tmp_path / tag
        w.mkdir()
        (w / "X.fastq").write_bytes(rc.text_of(recs))
        p = _run(["-r", "X.fastq", "-p", "-Q", "-N", "-G"] + flags, w)
        assert p.returncode == 0, p.stdout + p.stderr
        (w / "open").mkdir()
        got[tag] = _members(w / "X_comp_order.minicom", w / "open")
    assert sorted(got["with"]) == sorted(got["without"]) and "len.bin" not in got["with"] and not any(k.startswith("odd.") for k in got["with"])
    assert got["with"] == got["without"]


@pytest.mark.parametrize("flags,words", [(["-r", "X.fastq", "-V"], "-V needs -p"), (["-r", "X.fastq", "-V", "-q"], "-V cannot be combined with -q"),
                                         (["-1", "X.fastq", "-2", "X.fastq", "-p", "-V"], "a pair of files"), (["-r", "X.fastq", "-p", "-V", "-Q", "-b", "ill8"], "-V cannot be combined with -b")],
                         ids=["without_p", "with_q", "with_a_pair", "with_b"])
def test_V_is_refused_outside_its_scope(tmp_path, flags, words):
    (tmp_path / "X.fastq").write_bytes(rc.text_of(rc.make_records(5, [100, 100, 37, 100])))
    p = _run(flags, tmp_path)
    assert p.returncode == 1 and words in p.stdout, p.stdout + p.stderr
    assert sorted(f.name for f in tmp_path.iterdir()) == ["X.fastq"]


def test_without_V_the_file_is_refused_as_ever(tmp_path):
    """reads of differing lengths without -V: the ingest's own refusal, and no archive"""
    (tmp_path / "X.fastq").write_bytes(rc.text_of(rc.make_records(5, [100, 100, 37, 100])))
    p = _run(["-r", "X.fastq", "-p", "-G"], tmp_path)
    assert p.returncode != 0 and "Length of reads are different" in p.stdout + p.stderr, p.stdout + p.stderr
    assert not (tmp_path / "X_comp_order.minicom").exists()


def test_python_container_round_trip_and_check(tmp_path):
    """container.compress_fastq(order=True, ragged=True, quality=True, names=True): decompress_file gives the input back on both routes,
    verify_file says identical, and says which part differs for a file with one base changed in an odd read"""
    from minicom_amd import container
    recs = _trimmed_records(53, n=500)
    fq = tmp_path / "X.fastq"
    fq.write_bytes(rc.text_of(recs))
    arc = str(tmp_path / "X.minicom")
    sizes = container.compress_fastq(str(fq), arc, order=True, ragged=True, quality=True, names=True, codec="rans")
    want = rc.split(recs)
    assert (sizes["n_reads"], sizes["n_records"]) == (want["n_even"], len(recs)) and "len.bin.rans" in sizes and "odd.seq.rans" in sizes and "odd.qual.rans" in sizes
    for k, device in enumerate((0, None)):
        out = tmp_path / ("out%d.fastq" % k)
        assert container.decompress_file(arc, str(out), device=device) == len(recs)
        assert out.read_bytes() == rc.text_of(recs)
    rep = container.verify_file(arc, str(fq))
    assert rep["identical"] and all(rep[k]["identical"] for k in ("len", "even_reads", "even_quals", "odd_seq", "odd_qual", "names"))
    odd = next(i for i, r in enumerate(recs) if 30 <= len(r[1]) < 100)
    nm, s, pl, q = recs[odd]
    recs[odd] = (nm, s[:3] + (b"A" if s[3:4] != b"A" else b"C") + s[4:], pl, q)
    (tmp_path / "Y.fastq").write_bytes(rc.text_of(recs))
    rep = container.verify_file(arc, str(tmp_path / "Y.fastq"))
    assert not rep["identical"] and not rep["odd_seq"]["identical"] and rep["odd_seq"]["first_diff"] == odd and rep["odd_seq"]["differing"] == 1
    assert all(rep[k]["identical"] for k in ("len", "even_reads", "even_quals", "odd_qual", "names"))
    with pytest.raises(ValueError):
        container.compress_fastq(str(fq), arc, ragged=True)
