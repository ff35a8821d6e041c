"""Lossy quality values on the host (`minicom -b SPEC`): the plain C++ twin of the kernels
(host/mcom_qual_lossy.cpp) against the independent reference (tests/qual_lossy_reference.py), bytes and report both.  No GPU anywhere in
this file; the device side is tests/test_gpu_qual_lossy.py."""
import functools
import os
import subprocess

import numpy as np
import pytest

import qual_cases as qc
import qual_lossy_reference as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MCOMZ = os.path.join(ROOT, "bin", "mcomz")
PS = (1, 2, 4, 47)


def _all_bytes():
    """a matrix that holds all 256 byte values, each beside every residue of the column"""
    q = (np.arange(40 * 37, dtype=np.int64) * 7 % 256).astype(np.uint8).reshape(40, 37)
    assert len(np.unique(q)) == 256
    return q


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert got[1] == want[1], (got[1], want[1])


@pytest.mark.parametrize("spec", ["ill8", "thr:20:6:37", "thr:1:0:93", "thr:93:92:93"])
def test_byte_maps_against_the_reference(spec):
    from minicom_amd import pipeline
    q = _all_bytes()
    want = LR.transform(q, spec)
    got = pipeline.qual_transform(q, spec)
    _same(got, want)
    assert not np.array_equal(want[0], q)
    # idempotent: a second pass changes nothing
    again = pipeline.qual_transform(got[0], spec)
    assert np.array_equal(again[0], got[0]) and again[1] == {"changed": 0, "sum_abs": 0, "sum_sq": 0, "max_abs": 0}
    # every byte outside 33 .. 126 stays
    outside = (q < 33) | (q > 126)
    assert np.array_equal(got[0][outside], q[outside])


def test_the_two_named_maps_are_what_the_text_says():
    lut = LR.ill8_lut()
    assert [int(lut[33 + p]) - 33 for p in (0, 1, 2, 9, 10, 19, 20, 24, 25, 29, 30, 34, 35, 39, 40, 93)] == [0, 1, 6, 6, 15, 15, 22, 22, 27, 27, 33, 33, 37, 37, 40, 40]
    assert LR.is_idempotent(lut) and LR.is_idempotent(LR.thr_lut(20, 6, 37))
    assert not LR.is_idempotent(LR.thr_lut(20, 20, 37)) and not LR.is_idempotent(LR.thr_lut(20, 6, 19))


def test_a_general_map_and_one_that_is_not_idempotent():
    from minicom_amd import McomError, pipeline
    from minicom_amd.hip import QualLossySpec
    q = _all_bytes()
    halve = (np.arange(256) // 16 * 16).astype(np.uint8)                  # idempotent: every value to the floor of its sixteen
    _same(pipeline.qual_transform(q, QualLossySpec.from_lut(halve)), LR.transform(q, ("lut", halve)))
    plus_one = ((np.arange(256) + 1) % 256).astype(np.uint8)
    with pytest.raises(LR.LossyRefused):
        LR.transform(q, ("lut", plus_one))
    with pytest.raises(McomError):
        pipeline.qual_transform(q, QualLossySpec.from_lut(plus_one))
    s = QualLossySpec(); s.kind = QualLossySpec.THR; s.p[0], s.p[1], s.p[2] = 20, 20, 37   # thr with LO >= T, past the parser
    with pytest.raises(McomError):
        pipeline.qual_transform(q, s)


@functools.lru_cache(maxsize=None)
def _pblock_cases():
    """(name, P, matrix): the five rows of the text at L = 1, 2, 37 and 256 stacked per P, and the coder's degenerate matrices"""
    out = []
    for P in PS:
        for L in (1, 2, 37, 256):
            rows = LR.pblock_rows(P, L)
            out.append(("rows L%d" % L, P, np.stack([rows[k] for k in sorted(rows)])))
        for name, q in qc.degenerate():
            out.append((name, P, q))
    return tuple(out)


@pytest.mark.parametrize("P", PS)
def test_pblock_against_the_reference(P):
    from minicom_amd import pipeline
    for name, p, q in _pblock_cases():
        if p != P:
            continue
        want = LR.transform(q, ("pblock", P))
        got = pipeline.qual_transform(q, "pblock:%d" % P)
        assert np.array_equal(got[0], want[0]), (name, P)
        assert got[1] == want[1], (name, P, got[1], want[1])
        assert got[1]["max_abs"] <= P, (name, P)
        assert got[0].shape == q.shape


@pytest.mark.parametrize("P", PS)
def test_pblock_rows_do_what_the_text_says(P):
    """the reference itself on the rows whose answer the text states"""
    L = 256
    rows = LR.pblock_rows(P, L)
    assert LR.pblock_row(rows["constant"], P) == [70] * L
    # 93 apart: every block one column -- except at P = 47, where 2 P = 94 takes the whole row as one block
    assert LR.pblock_row(rows["alternating"], P) == (rows["alternating"].tolist() if P < 47 else [33 + 93 // 2] * L)
    r = LR.pblock_row(rows["rising"][:94], P)                                          # one ramp 33 .. 126: blocks of 2 P + 1, the middle value each
    w = 2 * P + 1
    if w < 94:
        assert r[:w] == [33 + P] * w and r[w] != r[w - 1]
    else:
        assert r == [33 + 93 // 2] * 94                                                # P = 47: the whole ramp is one block
    assert LR.pblock_row(rows["range 2P"], P) == [40 + P] * L                           # one block
    assert len(set(LR.pblock_row(rows["range 2P+1"], P))) > 1                           # more than one


def test_pblock_is_not_idempotent():
    """0 2 4 at P = 1: blocks {0 2} {4} -> 1 1 4; again: one block?  No: 1 1 4 has range 3 -> {1 1} {4}.  But 0 2 3 5 -> 1 1 4 4 -> stays,
    while 10 12 13 11 at P = 1 -> {10 12} {13 11} -> 11 11 12 12 -> one block -> 11 11 11 11"""
    q = np.array([[50, 52, 53, 51]], np.uint8)
    once = LR.transform(q, "pblock:1")[0]
    twice = LR.transform(once, "pblock:1")[0]
    assert once.tolist() == [[51, 51, 52, 52]] and twice.tolist() == [[51, 51, 51, 51]]
    from minicom_amd import pipeline
    assert np.array_equal(pipeline.qual_transform(pipeline.qual_transform(q, "pblock:1")[0], "pblock:1")[0], twice)


def test_rows_at_a_pitch_keep_their_gaps():
    from minicom_amd import pipeline
    import ctypes as C
    q = qc.synth_quals(8, 50, 37)
    wide = np.full((50, 41), 255, np.uint8); wide[:, :37] = q
    for spec in ("ill8", "pblock:2"):
        buf = wide.copy()
        s = pipeline.qual_lossy_spec(spec); r = pipeline.QualLossyReport()
        assert pipeline.load_host_library().mcomh_qual_transform(buf.ctypes.data, 50, 37, 41, C.byref(s), C.byref(r)) == 0
        want = LR.transform(q, spec)
        assert np.array_equal(buf[:, :37], want[0]) and np.all(buf[:, 37:] == 255) and r.as_dict() == want[1]


def test_spec_texts():
    from minicom_amd import McomError, pipeline
    for text in ("ill8", "thr:20:6:37", "thr:1:0:1", "thr:93:0:93", "pblock:1", "pblock:47", "pblock:10"):
        assert pipeline.qual_lossy_text(text) == text == LR.canonical(LR.parse(text))
    for text in ("", "ill9", "pblock:0", "pblock:48", "thr:94:0:0", "pblock:01", "thr:020:6:37", "thr:20:06:37", "ill8 ", "ill8x", "pblock:2:3", "thr:20:6:37:1", "thr:20:6", "ILL8", " ill8",
                 "pblock:", "pblock:-1", "pblock:+1", "thr:20:20:37", "thr:20:6:19", "thr:0:0:0", "pblock:1000", "ill8\n"):
        with pytest.raises(LR.LossyRefused):
            LR.parse(text)
        with pytest.raises(McomError):
            pipeline.qual_lossy_spec(text)
        p = subprocess.run([MCOMZ, "--lossy-spec", text], capture_output=True, text=True)
        assert p.returncode == 1 and p.stdout == "", text


def test_mcomz_qual_lossy_round_trip(tmp_path):
    """mcomz e --qual L --lossy SPEC, then mcomz d: the reference's matrix; the report on stderr in its one fixed line"""
    q = qc.synth_quals(12, 300, 100)
    (tmp_path / "q.raw").write_bytes(q.tobytes())
    for spec in ("ill8", "thr:20:6:37", "pblock:2"):
        want, rep = LR.transform(q, spec)
        p = subprocess.run([MCOMZ, "e", "--qual", "100", "--lossy", spec, "q.raw", "q.mcq"], cwd=tmp_path, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        assert p.stderr == "lossy %s: changed %d sum_abs %d sum_sq %d max_abs %d\n" % (spec, rep["changed"], rep["sum_abs"], rep["sum_sq"], rep["max_abs"])
        assert subprocess.run([MCOMZ, "d", "q.mcq", "back.raw"], cwd=tmp_path).returncode == 0
        assert (tmp_path / "back.raw").read_bytes() == want.tobytes(), spec
        os.remove(tmp_path / "q.mcq")
    p = subprocess.run([MCOMZ, "e", "--qual", "100", "--lossy", "pblock:48", "q.raw", "q.mcq"], cwd=tmp_path, capture_output=True, text=True)
    assert p.returncode == 1 and not (tmp_path / "q.mcq").exists()
    p = subprocess.run([MCOMZ, "e", "--lossy", "ill8", "q.raw", "q.mcq"], cwd=tmp_path, capture_output=True, text=True)      # --lossy without a quality route
    assert p.returncode == 1 and not (tmp_path / "q.mcq").exists()


def test_host_fastq_route(tmp_path):
    """mcomh_fastq_quality_member_lossy with device -1 (`mcomz e --fastq-qual L --lossy SPEC`): the member of the reference's matrix, with
    and without an order; a bad record is refused as without --lossy, the same record named, no member left"""
    from minicom_amd import McomError, pipeline
    reads, quals, text = qc.tricky_fastq()
    (tmp_path / "t.fastq").write_bytes(text)
    order = np.random.default_rng(3).permutation(120).astype("<u4")
    (tmp_path / "order.bin").write_bytes(order.tobytes())
    for spec in ("ill8", "pblock:2"):
        want, rep = LR.transform(quals, spec)
        assert pipeline.fastq_quality_member(str(tmp_path / "t.fastq"), 37, str(tmp_path / "m.mcq"), lossy=spec) == (120, rep)
        assert (tmp_path / "m.mcq").read_bytes() == pipeline.qual_encode(want), spec
        assert np.array_equal(pipeline.qual_decode((tmp_path / "m.mcq").read_bytes()), want)
        want_o, rep_o = LR.transform(quals[order], spec)
        assert pipeline.fastq_quality_member(str(tmp_path / "t.fastq"), 37, str(tmp_path / "o.mcq"), order_path=str(tmp_path / "order.bin"), lossy=spec) == (120, rep_o)
        assert (tmp_path / "o.mcq").read_bytes() == pipeline.qual_encode(want_o), spec
        assert np.array_equal(want_o, want[order]) and rep_o == rep                    # row-local: it commutes with the gather
        p = subprocess.run([MCOMZ, "e", "--fastq-qual", "37", "--order", "order.bin", "--lossy", spec, "t.fastq", "cli.mcq"], cwd=tmp_path, capture_output=True, text=True)
        assert p.returncode == 0 and p.stdout.split() == ["120"] and (tmp_path / "cli.mcq").read_bytes() == pipeline.qual_encode(want_o), p.stderr
        assert p.stderr == "lossy %s: changed %d sum_abs %d sum_sq %d max_abs %d\n" % (spec, rep["changed"], rep["sum_abs"], rep["sum_sq"], rep["max_abs"])
    for name, t in qc.bad_fastqs().items():
        (tmp_path / "bad.fastq").write_bytes(t)
        with pytest.raises(McomError, match=r"record 18 ") as plain:
            pipeline.fastq_quality_member(str(tmp_path / "bad.fastq"), 37, str(tmp_path / "bad.mcq"))
        with pytest.raises(McomError, match=r"record 18 ") as lossy:
            pipeline.fastq_quality_member(str(tmp_path / "bad.fastq"), 37, str(tmp_path / "bad.mcq"), lossy="ill8")
        assert str(plain.value) == str(lossy.value), name
        assert not (tmp_path / "bad.mcq").exists(), name
        p = subprocess.run([MCOMZ, "e", "--fastq-qual", "37", "--lossy", "pblock:2", "bad.fastq", "bad.mcq"], cwd=tmp_path, capture_output=True, text=True)
        assert p.returncode == 1 and "record 18 " in p.stderr and not (tmp_path / "bad.mcq").exists(), (name, p.stderr)
    with pytest.raises(McomError):
        pipeline.fastq_quality_member(str(tmp_path / "t.fastq"), 37, str(tmp_path / "x.mcq"), lossy="pblock:48")
    assert not (tmp_path / "x.mcq").exists()


@pytest.mark.parametrize("L", [100, 150])
def test_lossy_members_are_smaller(L):
    """the condition of section 3.13's table: on the project's own generator the `.mcq` member of the ill8, pblock:2 and pblock:4
    matrices is strictly smaller than the member of the untouched matrix (host twins)"""
    from minicom_amd import pipeline
    q = qc.synth_quals(7, 2000, L)
    plain = len(pipeline.qual_encode(q))
    for spec in ("ill8", "pblock:2", "pblock:4"):
        got = len(pipeline.qual_encode(pipeline.qual_transform(q, spec)[0]))
        print(L, spec, got, plain)
        assert got < plain, (L, spec, got, plain)


def test_minicom_b_is_refused_without_quality_values_and_with_a_bad_spec(tmp_path):
    """-b without -Q / -q, and -b with a spec the parser refuses: a message, exit 1, nothing left behind -- asked before anything is run"""
    (tmp_path / "x.fastq").write_bytes(b"@1\nACGT\n+\nIIII\n")
    (tmp_path / "y_2.fastq").write_bytes(b"@1\nACGT\n+\nIIII\n")
    exe = os.path.join(ROOT, "bin", "minicom")
    for args in (["-r", "x.fastq", "-b", "ill8"], ["-r", "x.fastq", "-p", "-b", "ill8"], ["-1", "x.fastq", "-2", "y_2.fastq", "-b", "pblock:2"],
                 ["-r", "x.fastq", "-p", "-Q", "-b", "ill9"], ["-r", "x.fastq", "-q", "-b", "pblock:0"], ["-r", "x.fastq", "-q", "-b", "thr:20:20:37"]):
        p = subprocess.run(["bash", exe] + args, cwd=tmp_path, capture_output=True, text=True)
        assert p.returncode == 1 and "minicom: -b " in p.stdout, (args, p.stdout, p.stderr)
        assert sorted(os.listdir(tmp_path)) == ["x.fastq", "y_2.fastq"], args
    p = subprocess.run(["bash", exe, "-h"], capture_output=True, text=True)
    assert "\t-b \t" in p.stdout and "NOT idempotent" in p.stdout


def test_marker_file(tmp_path):
    from minicom_amd import McomError, pipeline
    assert pipeline.qual_lossy_marker(str(tmp_path)) is None
    for text in ("ill8", "thr:20:6:37", "pblock:47"):
        (tmp_path / "qual_lossy.txt").write_bytes(text.encode() + b"\n")
        assert pipeline.qual_lossy_marker(str(tmp_path)) == text
    for bad in (b"ill8", b"ill8\n\n", b"ill9\n", b"\n", b"", b"pblock:02\n", b"ill8\r\n", b"x" * 100 + b"\n", b"ill8\0\n"):
        (tmp_path / "qual_lossy.txt").write_bytes(bad)
        with pytest.raises(McomError):
            pipeline.qual_lossy_marker(str(tmp_path))
