"""A record range of a -p archive on the host (`minicom -d -R`): the plain C++ twins of the range decoders --
mcomh_decompress_order_range, mcomh_decompress_fastq_range (device = -1) and mcomh_qual_decode_rows -- against slices of what the full
decode gives.  No GPU anywhere in this file; the device side is tests/test_gpu_range.py."""
import os
import subprocess

import numpy as np
import pytest

import qual_cases as qc
import qual_reference as QR
import range_cases as rc
import rans_reference as RR

ROOT = rc.ROOT


def _lines(rows, first, count):
    return b"".join(r + b"\n" for r in rows[first:first + count])


@pytest.fixture(scope="module")
def golden_folder(tmp_path_factory):
    made = {}

    def get(tag):
        if tag not in made:
            d = tmp_path_factory.mktemp("range_" + tag)
            rc.write_golden_folder(tag, d)
            made[tag] = d
        return made[tag]
    return get


@pytest.mark.parametrize("tag", sorted(rc.TAGS))
def test_order_range_is_the_slice_of_the_full_decode(golden_folder, tmp_path, tag):
    from minicom_amd import McomError, pipeline
    d, rows, n = golden_folder(tag), rc.golden_reads(tag), rc.TAGS[tag]
    out = tmp_path / "part.reads"
    for first, count in rc.read_ranges(n, seed=n):
        got = pipeline.decompress_range(str(d), str(out), first, count)
        assert got == max(0, min(count, n - first)), (first, count)
        assert out.read_bytes() == _lines(rows, first, count), (first, count)
        out.unlink()
    whole = _lines(rows, 0, n)
    for tiling in rc.tilings(n, seed=n + 1):
        parts = []
        for first, count in tiling:
            pipeline.decompress_range(str(d), str(out), first, count)
            parts.append(out.read_bytes())
        assert b"".join(parts) == whole, tiling
    out.unlink()
    with pytest.raises(McomError):
        pipeline.decompress_range(str(d), str(out), n + 1, 1)
    assert not out.exists()
    # the command-line form: --range FIRST COUNT in front of the plain -p decode
    p = subprocess.run([os.path.join(ROOT, "bin", "decompress"), "--range", "15", "2", str(d), str(out), "false", "true", "1"], capture_output=True)
    assert p.returncode == 0 and p.stdout == b"2 reads\n" and out.read_bytes() == _lines(rows, 15, 2)
    out.unlink()
    p = subprocess.run([os.path.join(ROOT, "bin", "decompress"), "--range", str(n + 1), "2", str(d), str(out), "false", "true", "1"], capture_output=True)
    assert p.returncode == 1 and not out.exists()


# ---- quality rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,A,model", rc.qual_grid(), ids=["L%d-A%d-%s" % c for c in rc.qual_grid()])
def test_qual_rows_are_the_slice_of_the_reference_decode(L, A, model):
    """mcomh_qual_decode_rows against the independent reference's full decode, sliced; decoding into a pitched table leaves the gaps alone"""
    from minicom_amd import McomError, pipeline
    member = rc.qual_member(L, A, model)
    want = QR.ref_decode(member, rans_decode=RR.ref_decode)
    n = want.shape[0]
    assert np.array_equal(want, rc.qual_matrix(L, A))
    for first, count in rc.qual_ranges(L, n):
        got = pipeline.qual_decode_rows(member, first, count)
        assert got.shape == (min(count, n - first), L) and np.array_equal(got, want[first:first + count]), (first, count)
    got = pipeline.qual_decode_rows(member, 1, QR.default_rps(L) + 1, pitch=L + 3)
    assert np.array_equal(got, want[1:QR.default_rps(L) + 2]) and not got.base.reshape(-1, L + 3)[:, L:].any()
    assert pipeline.qual_decode_rows(member, n, 5).shape == (0, L)          # first == n: nothing, and no error
    with pytest.raises(McomError):
        pipeline.qual_decode_rows(member, n + 1, 1)


@pytest.mark.parametrize("model", [1, 2, 3, 4])
def test_qual_rows_check_the_touched_segments_only(model):
    """DOCUMENTED BEHAVIOUR: the CRC-32 of a `.mcq` member covers all rows and cannot be checked for a part.  One
    flipped payload byte inside the window's segments is refused by those segments' own checks; the same flip outside them is NOT noticed
    by a range -- and is still refused by the whole range, which takes the full path with its CRC."""
    from minicom_amd import McomError, pipeline
    L, A = 100, 41
    good, q = rc.qual_member(L, A, model), rc.qual_matrix(L, A)
    rps, n = QR.default_rps(L), q.shape[0]
    bad = rc.flip_in_segment(good, 1)                                       # segment 1 holds rows rps .. 2 rps - 1
    for first, count in ((rps, 1), (rps - 1, 2), (0, rps + 1), (2 * rps - 1, 3)):
        with pytest.raises(McomError):
            pipeline.qual_decode_rows(bad, first, count)
    for first, count in ((0, rps), (0, 1), (2 * rps, 3), (2 * rps, n)):      # the flip lies outside: accepted, and the rows are right
        assert np.array_equal(pipeline.qual_decode_rows(bad, first, count), q[first:first + count])
    for first, count in ((0, n), (0, n + 9)):
        with pytest.raises(McomError):
            pipeline.qual_decode_rows(bad, first, count)
    with pytest.raises(McomError):
        pipeline.qual_decode(bad)


def test_qual_rows_refuse_what_the_full_decoder_refuses_in_header_and_tables():
    """the hostile corpus of the quality coder: whatever the full decoder refuses before it reads a run -- and every truncation -- is refused
    for a part as well; nothing that is accepted gives other rows than the reference"""
    from minicom_amd import McomError, pipeline
    q, good = qc.small()
    for member in qc.truncations()[::7] + [good[:-1], good + b"\0"]:
        with pytest.raises(McomError):
            pipeline.qual_decode_rows(member, 0, 1)
    # one crafted member per refusal rule; the corpus member has three segments: rows 0 .. 3, 4 .. 7 and 8
    touched = {"run<4": (0, 1), "state": (0, 1), "exhausted": (8, 1), "end": (8, 1), "slot": (5, 1)}
    for name, rule, member in qc.crafted():
        if rule in ("header", "tables", "lengths", "embedded"):
            for first, count in ((0, 1), (4, 4), (9, 0)):
                with pytest.raises(McomError):
                    pipeline.qual_decode_rows(member, first, count)
        elif rule in touched:
            with pytest.raises(McomError):
                pipeline.qual_decode_rows(member, *touched[rule])
    before_a_run_is_read = ("header", "tables", "lengths", "embedded")
    for member in qc.bit_flips(120):
        try:
            got = pipeline.qual_decode_rows(member, 4, 4)                   # segment 1 alone
        except McomError:
            continue
        try:
            want = QR.ref_decode(member, rans_decode=RR.ref_decode)
        except QR.QualRefused as e:
            assert e.args[0] not in before_a_run_is_read, e.args             # (a flip in another segment, or in the CRC field)
            continue
        assert np.array_equal(got, want[4:8])


# ---- FASTQ ----------------------------------------------------------------------------------------------------------------------------
def _records(rows, quals, names, plus, first, count):
    out = []
    for i in range(first, min(first + count, len(rows))):
        head = b"@%d\n" % (i + 1) if names is None else b"@" + names[i] + b"\n"
        out.append(head + rows[i] + b"\n+" + (b"" if names is None else plus[i]) + b"\n" + quals[i].tobytes() + b"\n")
    return b"".join(out)


@pytest.mark.parametrize("named", [False, True], ids=["numbered", "named"])
def test_fastq_range_is_the_slice_of_the_full_decode(tmp_path, named):
    """the golden reads with a qual.mcq and a name.mcn made by the host encoders: slices, tilings, and `@<i+1>` where the digits change"""
    from minicom_amd import McomError, pipeline
    tag = "stages_L100"
    rows, n = rc.golden_reads(tag), rc.TAGS[tag]
    d = tmp_path / "arch"; d.mkdir()
    rc.write_golden_folder(tag, d)
    quals = qc.synth_quals(17, n, 100)
    (d / "qual.mcq").write_bytes(pipeline.qual_encode(quals))
    names = plus = None
    if named:
        names = [b"run7:%d:%d/1 len=%d" % (i // 97, i * 31 % 1009, 100) for i in range(n)]
        plus = [names[i] if i % 3 == 0 else b"" for i in range(n)]
        (d / "name.mcn").write_bytes(pipeline.name_encode(pipeline.name_text(names, plus), n))
    out, full = tmp_path / "part.fastq", tmp_path / "full.fastq"
    assert pipeline.decompress_fastq(str(d), str(full)) == n
    whole = full.read_bytes()
    assert whole == _records(rows, quals, names, plus, 0, n)
    for first, count in [(0, 0), (0, 1), (n - 1, 1), (n, 5), (0, n + 7), (8, 3), (98, 3), (998, 3), (19, 2), (20, 20), (21, n - 21)]:
        assert pipeline.decompress_range(str(d), str(out), first, count, fastq=True) == max(0, min(count, n - first))
        assert out.read_bytes() == _records(rows, quals, names, plus, first, count), (first, count)
    for tiling in rc.tilings(n, seed=5):
        parts = []
        for first, count in tiling:
            pipeline.decompress_range(str(d), str(out), first, count, fastq=True)
            parts.append(out.read_bytes())
        assert b"".join(parts) == whole, tiling
    out.unlink()
    with pytest.raises(McomError):
        pipeline.decompress_range(str(d), str(out), n + 1, 1, fastq=True)
    assert not out.exists()
    p = subprocess.run([os.path.join(ROOT, "bin", "decompress"), "--range", "998", "3", "--fastq", str(d), str(out)], capture_output=True)
    assert p.returncode == 0 and p.stdout == b"3 records\n" and out.read_bytes() == _records(rows, quals, names, plus, 998, 3)


def test_refused_folders_leave_no_file(tmp_path):
    """a default-mode folder, a ragged folder (len.bin), a `minicom -q` folder (rqual.mcq): refused with a message that says why, before
    any file is written -- by the library and by `decompress --range`"""
    from minicom_amd import McomError, pipeline
    import gzip
    import io
    import tarfile
    out = tmp_path / "o.reads"

    def refused(d, word):
        for fastq in (False, True):
            with pytest.raises(McomError):
                pipeline.decompress_range(str(d), str(out), 0, 5, fastq=fastq)
            assert not out.exists()
        p = subprocess.run([os.path.join(ROOT, "bin", "decompress"), "--range", "0", "5", str(d), str(out), "false", "true", "1"], capture_output=True)
        assert p.returncode == 1 and word in p.stderr and not out.exists(), p.stderr

    default = tmp_path / "default"; default.mkdir()
    with gzip.open(os.path.join(rc.GOLDEN, "streams_stages_L100.tar.gz"), "rb") as g:
        tf = tarfile.open(fileobj=io.BytesIO(g.read()))
        for m in tf.getmembers():
            (default / m.name).write_bytes(tf.extractfile(m).read())
    refused(default, b"not a -p archive")
    ragged = tmp_path / "ragged"; ragged.mkdir()
    rc.write_golden_folder("stages_L100", ragged)
    (ragged / "len.bin").write_bytes(bytes([99]) * rc.TAGS["stages_L100"])
    refused(ragged, b"-V")
    reordered = tmp_path / "reordered"; reordered.mkdir()
    rc.write_golden_folder("stages_L100", reordered)
    (reordered / "rqual.mcq").write_bytes(pipeline.qual_encode(qc.synth_quals(2, 5, 100)))
    refused(reordered, b"-q")
    refused(tmp_path / "nowhere", b"info.txt")
    # a pair range of a folder that is no pair kept in input order
    ok = tmp_path / "ok"; ok.mkdir()
    rc.write_golden_folder("stages_L100", ok)
    with pytest.raises(McomError):
        pipeline.decompress_range(str(ok), str(out), 0, 5, out_path2=str(tmp_path / "o2.reads"))
    assert not out.exists() and not (tmp_path / "o2.reads").exists()
    # `decompress --range` in front of a mode it does not go with, and with numbers that are none
    for argv in (["--range", "0", "5", "--verify", str(ok), "x.fastq", "false", "true", "1"], ["--range", "x", "5", str(ok), str(out), "false", "true", "1"],
                 ["--range", "0", "5", str(ok), str(out), "false", "false", "1"]):
        assert subprocess.run([os.path.join(ROOT, "bin", "decompress")] + argv, capture_output=True).returncode == 1 and not out.exists()


def test_the_surface_exists():
    import re
    import minicom_amd
    from minicom_amd import pipeline
    lib, host = minicom_amd.load_library(), pipeline.load_host_library()
    for name in ("mcom_range_check_dest", "mcom_range_decode_reads", "mcom_qual_decode_rows"):
        assert name in minicom_amd.ABI_SYMBOLS and hasattr(lib, name)
    for name in ("mcomh_decompress_order_range", "mcomh_decompress_fastq_range", "mcomh_decompress_order_pe_range", "mcomh_qual_decode_rows"):
        assert name in pipeline.HOST_ABI_SYMBOLS and hasattr(host, name)
    assert lib.mcom_range_check_dest(None, None, 0, 0, 0, None, None) == -1
    assert lib.mcom_range_decode_reads(None, None, 0, 100, None, 0, 0, 0, None, None) == -1
    assert lib.mcom_qual_decode_rows(None, None, 0, 0, 0, None, 0, None, None) == -1
    for name in ("decode_check_dest", "decode_reads_window", "qual_decode_rows"):
        assert callable(getattr(minicom_amd.Context, name))
    usage = subprocess.run([os.path.join(ROOT, "bin", "minicom"), "-h"], capture_output=True, text=True).stdout
    assert re.search(r"^\t-R \t\tFIRST:COUNT", usage, re.M)
    for doc, word in (("README.md", "-R FIRST:COUNT"), ("DESIGN.md", "### 3.19")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc


def test_minicom_refuses_a_range_that_is_none(tmp_path):
    """bin/minicom -d X -R ...: refused before the archive is opened -- a spec that is not FIRST:COUNT with FIRST >= 1, and -c, -C, -T beside it"""
    mc = os.path.join(ROOT, "bin", "minicom")
    arch = tmp_path / "x.minicom"; arch.write_bytes(b"")
    for spec in ("0:5", "x", "5", "1:", ":3", "01:2", "1:2:3", "-1:4"):
        p = subprocess.run([mc, "-d", str(arch), "-R", spec], capture_output=True, text=True, cwd=tmp_path)
        assert p.returncode == 1 and "-R takes FIRST:COUNT" in p.stdout, (spec, p.stdout)
    for extra in (["-c", "a.fastq"], ["-T"], ["-c", "a.fastq", "-C", "b.fastq"]):
        p = subprocess.run([mc, "-d", str(arch), "-R", "1:5"] + extra, capture_output=True, text=True, cwd=tmp_path)
        assert p.returncode == 1 and "-R decompresses a range" in p.stdout, (extra, p.stdout)
    assert sorted(x.name for x in tmp_path.iterdir()) == ["x.minicom"]
