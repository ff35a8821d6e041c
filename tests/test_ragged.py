"""Reads of differing lengths on the host (host/mcom_ragged.cpp): the plain C++ twins against the split in plain
Python (tests/ragged_cases.py) byte for byte, the refusals with the first bad record named, the host decoders over a ragged folder built
on the golden -p stream files, their refusals of a folder whose parts disagree, and the fuzz program under the sanitizers."""
import gzip
import io
import os
import shutil
import subprocess
import tarfile

import numpy as np
import pytest

import ragged_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = rc.cases()


@pytest.mark.parametrize("name,recs", CASES, ids=rc.case_ids())
def test_host_twins_give_the_python_split(tmp_path, name, recs):
    fq = tmp_path / "in.fastq"
    fq.write_bytes(rc.text_of(recs))
    rc.check_against_python(recs, rc.split_files(tmp_path, fq))


@pytest.mark.parametrize("form", ["no_final_newline", "gz_one_member", "gz_five_members"])
@pytest.mark.parametrize("name", ["last_odd", "first_odd", "n_17"])
def test_host_twins_take_the_file_forms(tmp_path, name, form):
    recs = dict(CASES)[name]
    text = rc.text_of(recs, final_newline=form != "no_final_newline")
    fq = tmp_path / ("in.fastq" if form == "no_final_newline" else "in.fastq.gz")
    fq.write_bytes(text if form == "no_final_newline" else rc.gz_members(text, 1 if form == "gz_one_member" else 5))
    rc.check_against_python(recs, rc.split_files(tmp_path, fq))


@pytest.mark.parametrize("name,text,first_bad", rc.bad_records(), ids=[c[0] for c in rc.bad_records()])
def test_host_twin_names_the_first_bad_record(tmp_path, name, text, first_bad):
    from minicom_amd import McomError, pipeline
    fq = tmp_path / "bad.fastq"
    fq.write_bytes(text)
    with pytest.raises(McomError, match=r"record %d is not" % first_bad):
        pipeline.fastq_lengths(str(fq), str(tmp_path / "len.bin"))
    assert not (tmp_path / "len.bin").exists()


def test_split_refuses_a_length_file_that_is_not_the_files(tmp_path):
    """another length for a record, a record too few, a record too many: the first record that disagrees is named, nothing is written"""
    from minicom_amd import McomError, pipeline
    recs = dict(CASES)["odd_neighbours"]
    fq = tmp_path / "in.fastq"
    fq.write_bytes(rc.text_of(recs))
    want = rc.split(recs)
    for tag, lb, msg in (("length", want["len_bin"][:3] + bytes([41]) + want["len_bin"][4:], "record 4 is not what the length file says"),
                         ("short", want["len_bin"][:-1], "more records than the length file"), ("long", want["len_bin"] + b"\x63", "the length file 8")):
        (tmp_path / "len.bin").write_bytes(lb)
        with pytest.raises(McomError, match=msg):
            pipeline.fastq_ragged_files(str(fq), 1, want["L"], str(tmp_path / "len.bin"), str(tmp_path / "rows"), str(tmp_path / "odd"))
        assert not (tmp_path / "rows").exists() and not (tmp_path / "odd").exists(), tag


# ---- the host decoders over a ragged folder: the golden -p stream files hold the reads of the modal length ----
def ragged_archive(golden_dir, d, with_qual=True, with_names=True, every=9):
    """folder d: the golden -p stream files of stages_L100 as the even reads, an odd record in front of every `every`-th of them and one at
    the end, host-coded qual.mcq / name.mcn, len.bin, odd.seq, odd.qual.  Returns the records the archive stands for."""
    import qual_cases as qc
    from minicom_amd import pipeline
    d.mkdir()
    with gzip.open(os.path.join(golden_dir, "streams_order_stages_L100.tar.gz"), "rb") as g:
        tf = tarfile.open(fileobj=io.BytesIO(g.read()))
        for m in tf.getmembers():
            (d / m.name).write_bytes(tf.extractfile(m).read())
    with gzip.open(os.path.join(golden_dir, "stages_L100.reads.gz"), "rb") as f:
        rows = f.read().split(b"\n")[:-1]
    quals = np.resize(qc.synth_quals(21, 2000, 100), (len(rows), 100))
    odd_lengths = [1, 256, 99, 101, 15, 16, 17, 30, 64]
    lengths = []
    for i in range(len(rows)):
        if i % every == 0:
            lengths.append(odd_lengths[(i // every) % len(odd_lengths)])
        lengths.append(100)
    lengths.append(57)
    recs = rc.make_records(77, lengths)
    it = iter(range(len(rows)))
    for k, (nm, s, p, q) in enumerate(recs):
        if len(s) == 100:
            j = next(it)
            recs[k] = (nm, rows[j], p, quals[j].tobytes())
    want = rc.split(recs)
    assert want["L"] == 100 and want["n_even"] == len(rows)
    (d / "len.bin").write_bytes(want["len_bin"])
    (d / "odd.seq").write_bytes(want["odd_seq"])
    if with_qual:
        (d / "qual.mcq").write_bytes(pipeline.qual_encode(quals))
        (d / "odd.qual").write_bytes(want["odd_qual"])
        if with_names:
            (d / "name.mcn").write_bytes(pipeline.name_encode(rc.name_text(recs)[0], len(recs)))
    return recs


def test_host_decoders_give_the_records_back(golden_dir, tmp_path):
    """-p -V -Q -N: the input byte for byte; -p -V -Q: records named @<i+1>; -p -V: one read per line -- library and executable"""
    from minicom_amd import pipeline
    exe = os.path.join(ROOT, "bin", "decompress")
    recs = ragged_archive(golden_dir, tmp_path / "named")
    out = tmp_path / "out.fastq"
    assert pipeline.decompress_fastq(str(tmp_path / "named"), str(out)) == len(recs)
    assert out.read_bytes() == rc.text_of(recs)
    p = subprocess.run([exe, "--fastq", str(tmp_path / "named"), str(tmp_path / "out2.fastq")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.split()[0] == str(len(recs)), p.stdout + p.stderr
    assert (tmp_path / "out2.fastq").read_bytes() == rc.text_of(recs)
    recs = ragged_archive(golden_dir, tmp_path / "numbered", with_names=False)
    assert pipeline.decompress_fastq(str(tmp_path / "numbered"), str(out)) == len(recs)
    assert out.read_bytes() == rc.numbered(recs)
    recs = ragged_archive(golden_dir, tmp_path / "reads", with_qual=False)
    assert pipeline.decompress(str(tmp_path / "reads"), str(tmp_path / "out.reads"), order=True) == len(recs)
    assert (tmp_path / "out.reads").read_bytes() == rc.reads_only(recs)
    p = subprocess.run([exe, str(tmp_path / "reads"), str(tmp_path / "out2.reads"), "false", "true", "1"], capture_output=True, text=True)
    assert p.returncode == 0 and (tmp_path / "out2.reads").read_bytes() == rc.reads_only(recs), p.stdout + p.stderr


def _refused(d, out, fastq=True):
    from minicom_amd import McomError, pipeline
    with pytest.raises(McomError):
        if fastq:
            pipeline.decompress_fastq(str(d), str(out))
        else:
            pipeline.decompress(str(d), str(out), order=True)
    assert not out.exists()


@pytest.fixture(scope="module")
def good_folder(golden_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("ragged") / "arch"
    recs = ragged_archive(golden_dir, d)
    return d, recs


def _copy(good_folder, tmp_path):
    d = tmp_path / "arch"
    shutil.copytree(good_folder[0], d)
    return d, rc.split(good_folder[1])


def test_decoder_refuses_another_count_of_modal_lengths(good_folder, tmp_path):
    """the bytes of len.bin equal to L - 1 do not number the archive's reads: one more, one fewer"""
    d, want = _copy(good_folder, tmp_path)
    lb = bytearray(want["len_bin"])
    for change in ("more", "fewer"):
        b = bytearray(lb)
        k = b.index(99) if change == "fewer" else next(i for i, v in enumerate(b) if v != 99)
        b[k] = 98 if change == "fewer" else 99
        (d / "len.bin").write_bytes(bytes(b))
        _refused(d, tmp_path / "never.fastq")
        _refused(d, tmp_path / "never.reads", fastq=False)


def test_decoder_refuses_lengths_that_do_not_add_up_to_odd_seq(good_folder, tmp_path):
    d, want = _copy(good_folder, tmp_path)
    for odd in (want["odd_seq"][:-1], want["odd_seq"] + b"A"):
        (d / "odd.seq").write_bytes(odd)
        _refused(d, tmp_path / "never.fastq")
        _refused(d, tmp_path / "never.reads", fastq=False)
    (d / "odd.seq").unlink()
    _refused(d, tmp_path / "never.fastq")


def test_decoder_refuses_lengths_that_do_not_add_up_to_odd_qual(good_folder, tmp_path):
    d, want = _copy(good_folder, tmp_path)
    for odd in (want["odd_qual"][:-1], want["odd_qual"] + b"I"):
        (d / "odd.qual").write_bytes(odd)
        _refused(d, tmp_path / "never.fastq")


def test_decoder_refuses_members_of_another_record_count(good_folder, tmp_path):
    """qual.mcq states the reads of the modal length, name.mcn every record: one row fewer, one record fewer"""
    import qual_cases as qc
    from minicom_amd import pipeline
    d, want = _copy(good_folder, tmp_path)
    keep = (d / "qual.mcq").read_bytes()
    (d / "qual.mcq").write_bytes(pipeline.qual_encode(np.resize(qc.synth_quals(21, 2000, 100), (want["n_even"] - 1, 100))))
    _refused(d, tmp_path / "never.fastq")
    (d / "qual.mcq").write_bytes(keep)
    recs = good_folder[1]
    (d / "name.mcn").write_bytes(pipeline.name_encode(rc.name_text(recs[:-1])[0], len(recs) - 1))
    _refused(d, tmp_path / "never.fastq")
    _refused(d, tmp_path / "never.reads", fastq=False)


def test_decoder_refuses_odd_qual_without_qual_mcq_and_the_reverse(good_folder, tmp_path):
    d, want = _copy(good_folder, tmp_path)
    (d / "odd.qual").unlink()
    _refused(d, tmp_path / "never.fastq")
    _refused(d, tmp_path / "never.reads", fastq=False)
    (d / "odd.qual").write_bytes(want["odd_qual"])
    (d / "qual.mcq").unlink()
    _refused(d, tmp_path / "never.fastq")
    _refused(d, tmp_path / "never.reads", fastq=False)


def test_fuzz_program_under_the_sanitizers(good_folder, tmp_path):
    """tests/fuzz_ragged.cpp built with -fsanitize=address,undefined and run on the CPU over the good folder and its FASTQ"""
    exe = tmp_path / "fuzz_ragged"
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "minicom_amd", "host"), "fuzz_ragged", "FUZZ_RAGGED_OUT=" + str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    shutil.copytree(good_folder[0], tmp_path / "arch")
    (tmp_path / "in.fastq").write_bytes(rc.text_of(good_folder[1]))
    p = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and "fuzz_ragged ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
