"""Self-checking archives on the host (host/mcom_digest.cpp): the plain C++ twin against the definition in plain
Python integers (tests/digest_reference.py) element for element and byte for byte, the parser's refusals, what the digest notices and what
it does not, the check of the host decoders' output over the golden -p stream files, and the fuzz program under the sanitizers."""
import gzip
import io
import os
import subprocess
import tarfile

import numpy as np
import pytest

import digest_reference as dr
import ragged_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = dr.cases()


def _rows(a):
    return [tuple(int(v) for v in row) for row in a]


@pytest.mark.parametrize("name,recs", CASES, ids=dr.case_ids())
def test_twin_gives_the_reference_hashes_and_sums(name, recs):
    from minicom_amd import pipeline
    hS, hQ, hN, bits, first = pipeline.fastq_record_hashes_host(rc.text_of(recs))
    want = [dr.record_hashes(r) for r in recs]
    assert (bits, first) == (0, None)
    assert _rows(hS) == [w[0] for w in want] and _rows(hQ) == [w[1] for w in want] and _rows(hN) == [w[2] for w in want]
    assert pipeline.digest_reduce_host(hS, hQ, hN) == dr.sums16(dr.sums(recs))
    assert pipeline.digest_reduce_host(hS) == dr.sums16(dr.sums(recs, with_qual=False, with_names=False))
    mate = dr.mate_of(recs)
    mS, mQ, mN, _, _ = pipeline.fastq_record_hashes_host(rc.text_of(mate))
    assert pipeline.digest_reduce_host(hS, hQ, hN, mS, mQ, mN) == dr.sums16(dr.sums(recs, mate))
    # one read per line: the sequence hashes alone, the same words
    rS, rQ, rN, bits, _ = pipeline.fastq_record_hashes_host(rc.reads_only(recs), lines_per_record=1)
    assert bits == 0 and rQ is None and rN is None and _rows(rS) == [w[0] for w in want]


def test_twin_writes_into_the_rows_of_its_records_only():
    """records first_record .. of arrays that cover more: the rows around them keep what they held"""
    from minicom_amd import pipeline
    recs = dict(CASES)["n_17"]
    hS, hQ, hN, bits, _ = pipeline.fastq_record_hashes_host(rc.text_of(recs), first_record=3, n_total=25)
    want = [dr.record_hashes(r) for r in recs]
    assert bits == 0 and _rows(hS[3:20]) == [w[0] for w in want] and _rows(hN[3:20]) == [w[2] for w in want]
    for a in (hS, hQ, hN):
        assert not a[:3].any() and not a[20:].any()


@pytest.mark.parametrize("name,text,first_bad,bits", dr.bad_records(), ids=[c[0] for c in dr.bad_records()])
def test_twin_flags_the_first_bad_record_and_the_file_call_names_it(tmp_path, name, text, first_bad, bits):
    from minicom_amd import McomError, pipeline
    hS, _, _, got_bits, first = pipeline.fastq_record_hashes_host(text)
    assert (got_bits, first) == (bits, first_bad - 1)
    assert not hS[first_bad - 1].any() and hS[first_bad % 6].any()                  # no hash for it, one for its neighbour
    fq = tmp_path / "bad.fastq"
    fq.write_bytes(text)
    with pytest.raises(McomError, match=r"record %d is not a four-line FASTQ record" % first_bad):
        pipeline.fastq_digest(str(fq), out_path=str(tmp_path / "digest.txt"))
    assert not (tmp_path / "digest.txt").exists()


@pytest.mark.parametrize("name,recs", CASES, ids=dr.case_ids())
def test_digest_txt_bytes(tmp_path, name, recs):
    """one file, a pair, without the quality keys, one read per line; plain, gzip in several members, without the last newline"""
    from minicom_amd import pipeline
    fq, fq2 = tmp_path / "in_1.fastq", tmp_path / "in_2.fastq.gz"
    mate = dr.mate_of(recs)
    fq.write_bytes(rc.text_of(recs, final_newline=False))
    fq2.write_bytes(rc.gz_members(rc.text_of(mate), 3))
    assert pipeline.fastq_digest(str(fq)) == dr.digest_text(recs)
    assert pipeline.fastq_digest(str(fq2)) == dr.digest_text(mate)
    assert pipeline.fastq_digest(str(fq), with_qual=False) == dr.digest_text(recs, with_qual=False)
    assert pipeline.fastq_digest(str(fq), str(fq2)) == dr.digest_text(recs, mate)
    assert pipeline.fastq_digest(str(fq), str(fq2), with_qual=False) == dr.digest_text(recs, mate, with_qual=False)
    (tmp_path / "in.reads").write_bytes(rc.reads_only(recs))
    assert pipeline.fastq_digest(str(tmp_path / "in.reads"), lines_per_record=1) == dr.digest_text(recs, with_qual=False, with_names=False)
    d = pipeline.digest_parse(dr.digest_text(recs, mate))
    assert d["files"] == 2 and d["n"] == len(recs) and d["rec.multiset"] == dr.sums(recs, mate)["rec.multiset"]


def test_file_call_refusals(tmp_path):
    """a file that ends inside a record, an empty one, a pair of different record counts, a multi-line record: said, and no file written"""
    from minicom_amd import McomError, pipeline
    recs = dict(CASES)["n_17"]
    out = tmp_path / "digest.txt"
    t = rc.text_of(recs)
    (tmp_path / "cut.fastq").write_bytes(t[:t.rindex(b"\n+")])
    (tmp_path / "empty.fastq").write_bytes(b"")
    (tmp_path / "a.fastq").write_bytes(t)
    (tmp_path / "b.fastq").write_bytes(rc.text_of(recs[:-1]))
    n, s, p, q = recs[4]
    (tmp_path / "multi.fastq").write_bytes(rc.text_of(recs[:4]) + b"@" + n + b"\n" + s[:20] + b"\n" + s[20:] + b"\n+\n" + q[:20] + b"\n" + q[20:] + b"\n")
    for path, path2, msg in (("cut.fastq", None, "ends inside record 17"), ("empty.fastq", None, "holds no record"), ("a.fastq", "b.fastq", "different numbers of records: 17 and 16"),
                             ("multi.fastq", None, "record 5 is not a four-line FASTQ record"), ("absent.fastq", None, "cannot open")):
        with pytest.raises(McomError, match=msg):
            pipeline.fastq_digest(str(tmp_path / path), None if path2 is None else str(tmp_path / path2), out_path=str(out))
        assert not out.exists(), path
    with pytest.raises(McomError, match=r"record 2 is not a line of 1 \.\. 256 bases"):
        (tmp_path / "x.reads").write_bytes(b"ACGT\n\nACGT\n")
        pipeline.fastq_digest(str(tmp_path / "x.reads"), lines_per_record=1, out_path=str(out))
    assert not out.exists()


def test_parser_refuses_what_the_printer_does_not_write():
    from minicom_amd import McomError, pipeline
    recs = dict(CASES)["n_16"]
    good = dr.digest_text(recs)
    pair = dr.digest_text(recs, dr.mate_of(recs))
    assert pipeline.digest_parse(good)["n"] == 16 and pipeline.digest_parse(pair)["files"] == 2
    lines = good.split("\n")[:-1]

    def text(ls):
        return "\n".join(ls) + "\n"

    bad = {
        "no newline at the end": good[:-1],
        "an unknown key": good + "seq.sorted 0000000000000000 0000000000000000\n",
        "a key given twice": text(lines + [lines[-1]]),
        "not in their order": text(lines[:3] + [lines[4], lines[3]] + lines[5:]),
        "sixteen lower-case hexadecimal digits": text(lines[:-1] + [lines[-1][:-1]]),
        "sixteen lower-case hexadecimal digits ": text(lines[:-1] + [lines[-1] + "0"]),
        "sixteen lower-case hexadecimal digits  ": text(lines[:-1] + [lines[-1][:-1] + "F"]),
        "sixteen lower-case hexadecimal digits   ": text(lines[:-1] + [lines[-1].replace(" ", "  ", 1)]),
        "the first line": good.replace("minicom-digest 1", "minicom-digest 2"),
        "the second line": good.replace("files 1", "files 3"),
        "without leading zeros": good.replace("n 16", "n 016"),
        "without leading zeros ": good.replace("n 16", "n 4294967296"),
        "not those of a digest of this many files": good.replace("files 1", "files 2"),
        "not those of a digest of this many files ": text(lines[:-1]),                       # rec.multiset gone, qual.ordered.1 still there
        "not those of a digest of this many files  ": text([l for l in lines if not l.startswith("seq.multiset")]),
        "not those of a digest of this many files   ": text([l for l in pair.split("\n")[:-1] if not l.startswith("name.ordered.2")]),
        "no `n` line": "minicom-digest 1\nfiles 1\n",
        "a zero byte": good[:-1] + "\0\n",
        "longer than any digest": good + "\n" * 1024,
    }
    for why, t in bad.items():
        with pytest.raises(McomError, match=why.strip()):
            pipeline.digest_parse(t)


# ---- what the digest notices ----
def _digest(tmp_path, recs, recs2=None, **kw):
    from minicom_amd import pipeline
    (tmp_path / "s_1.fastq").write_bytes(rc.text_of(recs))
    if recs2 is not None:
        (tmp_path / "s_2.fastq").write_bytes(rc.text_of(recs2))
    d = pipeline.digest_parse(pipeline.fastq_digest(str(tmp_path / "s_1.fastq"), None if recs2 is None else str(tmp_path / "s_2.fastq"), **kw))
    assert {k: v for k, v in d.items() if k not in ("files", "n")} == dr.sums(recs, recs2)       # (the twin is the reference, here too)
    return d


def _changed(a, b):
    return {k for k in a if a[k] != b[k]}


def test_two_records_swapped_changes_the_ordered_sums_only(tmp_path):
    recs = dict(CASES)["n_17"]
    other = list(recs)
    other[3], other[11] = other[11], other[3]
    assert _changed(_digest(tmp_path, recs), _digest(tmp_path, other)) == {"seq.ordered.1", "qual.ordered.1", "name.ordered.1"}


def test_one_byte_changed_changes_both_kinds(tmp_path):
    recs = dict(CASES)["n_17"]
    n, s, p, q = recs[5]
    other = list(recs)
    other[5] = (n, s[:-1] + (b"A" if s[-1:] != b"A" else b"C"), p, q)
    assert _changed(_digest(tmp_path, recs), _digest(tmp_path, other)) == {"seq.ordered.1", "seq.multiset", "rec.multiset"}
    other[5] = (n, s, p, q[:3] + bytes([q[3] ^ 1]) + q[4:])
    assert _changed(_digest(tmp_path, recs), _digest(tmp_path, other)) == {"qual.ordered.1", "rec.multiset"}
    other[5] = (n + b"x", s, p, q)
    assert _changed(_digest(tmp_path, recs), _digest(tmp_path, other)) == {"name.ordered.1"}
    other[5] = (n, s, p + b"x", q)
    assert _changed(_digest(tmp_path, recs), _digest(tmp_path, other)) == {"name.ordered.1"}


def test_quality_lines_swapped_between_records_changes_rec_multiset_only_among_the_multisets(tmp_path):
    recs = rc.make_records(50, [100] * 12)
    other = list(recs)
    other[2], other[9] = (recs[2][0], recs[2][1], recs[2][2], recs[9][3]), (recs[9][0], recs[9][1], recs[9][2], recs[2][3])
    assert _changed(_digest(tmp_path, recs), _digest(tmp_path, other)) == {"qual.ordered.1", "rec.multiset"}


def test_last_byte_moved_to_the_front_of_the_next_line_changes_the_digest(tmp_path):
    """the bytes of the file stay in their order and only a line boundary moves: the line length is part of H"""
    recs = rc.make_records(51, [100] * 6)
    n, s, p, q = recs[2]
    n2, s2, p2, q2 = recs[3]
    other = list(recs)
    other[2], other[3] = (n, s[:-1], p, q[:-1]), (n2, s[-1:] + s2, p2, q[-1:] + q2)
    assert {"seq.ordered.1", "qual.ordered.1", "seq.multiset", "rec.multiset"} <= _changed(_digest(tmp_path, recs), _digest(tmp_path, other))
    other = list(recs)
    other[2] = (n[:-1], s, n[-1:] + p, q)                                           # from the name to the '+' text of one record
    assert _changed(_digest(tmp_path, recs), _digest(tmp_path, other)) == {"name.ordered.1"}


def test_mates_swapped_between_the_files_of_a_pair_changes_seq_multiset(tmp_path):
    recs = dict(CASES)["n_17"]
    mate = dr.mate_of(recs)
    a, b = list(recs), list(mate)
    a[7], b[7] = mate[7], recs[7]
    changed = _changed(_digest(tmp_path, recs, mate), _digest(tmp_path, a, b))
    assert {"seq.multiset", "rec.multiset", "seq.ordered.1", "seq.ordered.2"} <= changed
    # ... and the same pairs in another order leave both multisets
    a, b = list(recs), list(mate)
    a[2], a[8], b[2], b[8] = a[8], a[2], b[8], b[2]
    assert _changed(_digest(tmp_path, recs, mate), _digest(tmp_path, a, b)) == {"seq.ordered.1", "qual.ordered.1", "name.ordered.1", "seq.ordered.2", "qual.ordered.2", "name.ordered.2"}


# ---- the check over the decoder's output files ----
@pytest.fixture(scope="module")
def order_folder(golden_dir, tmp_path_factory):
    """the golden -p stream files of stages_L100 with host-coded qual.mcq and name.mcn, and the records they stand for"""
    import qual_cases as qc
    from minicom_amd import pipeline
    d = tmp_path_factory.mktemp("digest") / "arch"
    d.mkdir()
    with gzip.open(os.path.join(golden_dir, "streams_order_stages_L100.tar.gz"), "rb") as g:
        tf = tarfile.open(fileobj=io.BytesIO(g.read()))
        for m in tf.getmembers():
            (d / m.name).write_bytes(tf.extractfile(m).read())
    with gzip.open(os.path.join(golden_dir, "stages_L100.reads.gz"), "rb") as f:
        rows = f.read().split(b"\n")[:-1]
    quals = np.resize(qc.synth_quals(23, 2000, 100), (len(rows), 100))
    recs = [(b"read.%d/1" % i, rows[i], b"" if i % 5 else b"read.%d" % i, quals[i].tobytes()) for i in range(len(rows))]
    (d / "qual.mcq").write_bytes(pipeline.qual_encode(quals))
    (d / "name.mcn").write_bytes(pipeline.name_encode(rc.name_text(recs)[0], len(recs)))
    return d, recs


def _folder(order_folder, tmp_path, recs=None, keep=("qual.mcq", "name.mcn"), **kw):
    import shutil
    from minicom_amd import pipeline
    d = tmp_path / "arch"
    shutil.copytree(order_folder[0], d)
    for m in ("qual.mcq", "name.mcn"):
        if m not in keep:
            (d / m).unlink()
    fq = tmp_path / "in.fastq"
    fq.write_bytes(rc.text_of(order_folder[1] if recs is None else recs))
    pipeline.fastq_digest(str(fq), out_path=str(d / "digest.txt"), **kw)
    return d


def test_check_of_the_host_decoders_output(order_folder, tmp_path):
    """-p -Q -N: reads, quality lines and names; -p -Q: no names (the records are numbered); -p: the reads file -- decoded by the host decoders"""
    from minicom_amd import pipeline
    recs = order_folder[1]
    exe = os.path.join(ROOT, "bin", "decompress")
    d = _folder(order_folder, tmp_path)
    out = tmp_path / "out_dec.fastq"
    assert pipeline.decompress_fastq(str(d), str(out)) == len(recs) and out.read_bytes() == rc.text_of(recs)
    rep = pipeline.digest_check(str(d), str(out))
    assert rep["identical"] and rep["compared"] == ["seq.ordered.1", "qual.ordered.1", "name.ordered.1"] and rep["n_stored"] == rep["n_output"] == len(recs)
    p = subprocess.run([exe, "--check-digest", str(d), str(out)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout == "verified: reads, quality lines and names identical to the compressed input of %d records\n" % len(recs), p.stdout + p.stderr
    (d / "name.mcn").unlink()
    assert pipeline.decompress_fastq(str(d), str(out)) == len(recs) and out.read_bytes() == rc.numbered(recs)
    rep = pipeline.digest_check(str(d), str(out))
    assert rep["identical"] and rep["compared"] == ["seq.ordered.1", "qual.ordered.1"]
    (d / "qual.mcq").unlink()
    out = tmp_path / "out_dec.reads"
    assert pipeline.decompress(str(d), str(out), order=True) == len(recs)
    rep = pipeline.digest_check(str(d), str(out))
    assert rep["identical"] and rep["compared"] == ["seq.ordered.1"]
    p = subprocess.run([exe, "--check-digest", str(d), str(out)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout == "verified: reads identical to the compressed input of %d records\n" % len(recs), p.stdout + p.stderr


def test_check_with_hand_made_outputs(order_folder, tmp_path):
    """what differs is named; the quality keys left out (`--no-qual`) are not compared; .gz outputs; an archive in its own order asks the multiset"""
    from minicom_amd import McomError, pipeline
    recs = order_folder[1]
    exe = os.path.join(ROOT, "bin", "decompress")
    d = _folder(order_folder, tmp_path)
    out = tmp_path / "out.fastq.gz"

    def check(rs):
        out.write_bytes(rc.gz_members(rc.text_of(rs), 4))
        return pipeline.digest_check(str(d), str(out))

    assert check(recs)["identical"]
    other = list(recs)
    other[10], other[20] = other[20], other[10]
    rep = check(other)
    assert not rep["identical"] and rep["differing"] == ["seq.ordered.1", "qual.ordered.1", "name.ordered.1"] and rep["first_diff"] == "seq.ordered.1"
    n, s, p, q = recs[100]
    other = list(recs)
    other[100] = (n, s, p, q[:50] + bytes([q[50] ^ 2]) + q[51:])
    rep = check(other)
    assert not rep["identical"] and rep["differing"] == ["qual.ordered.1"]
    pr = subprocess.run([exe, "--check-digest", str(d), str(out)], capture_output=True, text=True)
    assert pr.returncode == 2 and "quality lines differ" in pr.stdout, pr.stdout + pr.stderr
    other[100] = (n[:-1], s, p, q)
    assert check(other)["differing"] == ["name.ordered.1"]
    rep = check(recs[:-1])
    assert not rep["identical"] and rep["first_diff"] == "n" and (rep["n_stored"], rep["n_output"]) == (len(recs), len(recs) - 1)
    # made beside -b / -a: the quality lines of the output are not the file's, and are not asked
    d = _folder(order_folder, tmp_path / "nq", with_qual=False)
    other = [(n, s, p, bytes(33 + (v - 33) // 2 for v in q)) for n, s, p, q in recs]
    rep = check(other)
    assert rep["identical"] and rep["compared"] == ["seq.ordered.1", "name.ordered.1"]
    # an archive in its own order (no list of ids): the reads as a multiset, with rqual.mcq the records
    for f in os.listdir(d):
        if f.endswith("ids.bin") or f.startswith("ids.bin."):
            (d / f).unlink()
    d2 = _folder((d, recs), tmp_path / "own", keep=())
    (d2 / "rqual.mcq").write_bytes(b"x")
    shuffled = recs[1::2] + recs[0::2]
    rep = check(shuffled)
    assert rep["identical"] and rep["compared"] == ["seq.multiset"]                 # (d: stored without the quality keys)
    d = d2
    rep = check(shuffled)
    assert rep["identical"] and rep["compared"] == ["rec.multiset"]
    other = list(shuffled)
    other[0], other[1] = (other[0][0], other[0][1], other[0][2], other[1][3]), (other[1][0], other[1][1], other[1][2], other[0][3])
    assert check(other)["differing"] == ["rec.multiset"]
    (d / "rqual.mcq").unlink()
    out = tmp_path / "out.reads.gz"
    out.write_bytes(gzip.compress(rc.reads_only(shuffled)))
    rep = pipeline.digest_check(str(d), str(out))
    assert rep["identical"] and rep["compared"] == ["seq.multiset"]
    # refusals: two files for the digest of one, a digest that does not parse, none at all
    for damage, why in ((None, "that of one file"), (lambda t: t[:-2] + "\n", "not a digest"), (lambda t: None, "no digest.txt")):
        t = (d / "digest.txt").read_text()
        if damage is not None:
            (d / "digest.txt").write_text(damage(t)) if damage(t) is not None else (d / "digest.txt").unlink()
        with pytest.raises(McomError, match=why):
            pipeline.digest_check(str(d), str(out), str(out) if damage is None else None)
    pr = subprocess.run([exe, "--check-digest", str(d), str(out)], capture_output=True, text=True)
    assert pr.returncode == 1 and "no digest.txt" in pr.stderr, pr.stdout + pr.stderr


def test_mcomz_fastq_digest(tmp_path):
    """the executable: the twin's bytes, the record count on stdout, --no-qual, a pair, the refusal with its reason and status 1"""
    recs = dict(CASES)["n_17"]
    mate = dr.mate_of(recs)
    exe = os.path.join(ROOT, "bin", "mcomz")
    (tmp_path / "a_1.fastq").write_bytes(rc.text_of(recs))
    (tmp_path / "a_2.fastq").write_bytes(rc.text_of(mate))
    out = tmp_path / "digest.txt"
    for args, want in (([str(tmp_path / "a_1.fastq")], dr.digest_text(recs)), (["--no-qual", str(tmp_path / "a_1.fastq")], dr.digest_text(recs, with_qual=False)),
                       ([str(tmp_path / "a_1.fastq"), str(tmp_path / "a_2.fastq")], dr.digest_text(recs, mate))):
        p = subprocess.run([exe, "e", "--fastq-digest"] + args + [str(out)], capture_output=True, text=True)
        assert p.returncode == 0 and p.stdout == "17\n" and out.read_text() == want, p.stdout + p.stderr
        out.unlink()
    (tmp_path / "b.fasta").write_bytes(b">r1\nACGT\n>r2\nACGT\n")
    p = subprocess.run([exe, "e", "--fastq-digest", str(tmp_path / "b.fasta"), str(out)], capture_output=True, text=True)
    assert p.returncode == 1 and "record 1 is not a four-line FASTQ record" in p.stderr and not out.exists(), p.stdout + p.stderr


def test_fuzz_program_under_the_sanitizers(tmp_path):
    """tests/fuzz_digest.cpp built with -fsanitize=address,undefined and run on the CPU"""
    exe = tmp_path / "fuzz_digest"
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "minicom_amd", "host"), "fuzz_digest", "FUZZ_DIGEST_OUT=" + str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    p = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and "fuzz_digest ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
