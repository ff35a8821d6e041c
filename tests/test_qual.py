"""Quality values as `.mcq` members on the host: the plain C++ twin of the GPU coder (host/mcom_qual.cpp)
against the independent reference (tests/qual_reference.py).  No GPU anywhere in this file; the device side is tests/test_gpu_qual.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import qual_cases as qc
import qual_reference as QR
import rans_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = 64


def _rans(q) -> bytes:
    """the `.rans` member of the flat bytes, hint 0"""
    from minicom_amd import pipeline
    return pipeline.rans_encode(np.ascontiguousarray(q).tobytes())


def _host_refuses(member) -> bool:
    from minicom_amd import McomError, pipeline
    try:
        pipeline.qual_decode(member)
    except McomError:
        return True
    return False


@pytest.mark.parametrize("name,q", qc.degenerate(), ids=[c[0] for c in qc.degenerate()])
def test_host_twin_emits_the_reference_bytes(name, q):
    """every degenerate matrix under the choice and under every forced model id: the same bytes, and both decoders give the matrix"""
    from minicom_amd import pipeline
    rans = _rans(q)
    for model in (None, 0, 1, 2, 3, 4, "rans"):
        want = QR.ref_encode(q, model=model, rans_member=rans)
        got = pipeline.qual_encode(q, model)
        assert got == want, (name, model, len(got), len(want))
        assert np.array_equal(pipeline.qual_decode(got), q), (name, model)
        assert np.array_equal(QR.ref_decode(got, rans_decode=RR.ref_decode), q), (name, model)
        assert pipeline.qual_info(got) == q.shape
        if q.shape[0] and model in (1, 2, 3, 4):
            assert got[5] == 0 and got[6] == model


def test_rows_at_a_pitch():
    """rows that are not back to back: the same member, and a decode into a pitched table leaves the gaps alone"""
    from minicom_amd import pipeline
    q = qc.synth_quals(8, 50, 37)
    wide = np.full((50, 41), 255, np.uint8); wide[:, :37] = q
    for model in (None, 0, 3, "rans"):
        m = pipeline.qual_encode(wide[:, :37], model)
        assert m == pipeline.qual_encode(q, model)
        assert np.array_equal(pipeline.qual_decode(m, pitch=41), q)


@pytest.mark.parametrize("rps", [1, 3, 20, 64, 327])
def test_host_decodes_reference_members_at_other_rows_per_seg(rps):
    from minicom_amd import pipeline
    q = qc.synth_quals(9, 330, 100)
    for model in (2, 4):
        m = QR.ref_encode(q, model=model, rows_per_seg=rps)
        assert int.from_bytes(m[26:28], "little") == rps
        assert np.array_equal(pipeline.qual_decode(m), q), (rps, model)


def test_one_crafted_member_per_refusal_rule():
    """the reference names the rule, the host twin refuses the member"""
    q, base = qc.small()
    assert np.array_equal(QR.ref_decode(base), q) and not _host_refuses(base)
    for name, rule, member in qc.crafted():
        with pytest.raises(QR.QualRefused) as e:
            QR.ref_decode(member, rans_decode=RR.ref_decode)
        assert e.value.rule == rule, (name, e.value.rule)
        assert _host_refuses(member), name
    # kind 1: an embedded member of another length, with another CRC, and a damaged one
    from minicom_amd import pipeline
    good = pipeline.qual_encode(q, "rans")
    assert np.array_equal(QR.ref_decode(good, rans_decode=RR.ref_decode), q) and not _host_refuses(good)
    other = QR.ref_header(1, 0, len(_rans(q[:-1])), int.from_bytes(good[12:16], "little"), q.shape[0], q.shape[1], 55, 0, bytes(32)) + _rans(q[:-1])
    flipped = bytearray(good); flipped[-1] ^= 0x10
    for name, member in (("embedded length", other), ("embedded crc", good[:12] + bytes(4) + good[16:]), ("embedded damage", bytes(flipped))):
        with pytest.raises(QR.QualRefused) as e:
            QR.ref_decode(member, rans_decode=RR.ref_decode)
        assert e.value.rule == "embedded", name
        assert _host_refuses(member), name


def test_hostile_corpus_is_refused_or_exact():
    """every truncation and 200 bit flips of a small member: refused, or decoded to exactly what the reference decodes; never a crash.
    The host twin and the reference take the same decision for every member."""
    from minicom_amd import pipeline
    q, base = qc.small()
    for member in qc.truncations() + qc.bit_flips():
        try:
            want = QR.ref_decode(member, rans_decode=RR.ref_decode)
        except QR.QualRefused:
            want = None
        if want is None:
            assert _host_refuses(member)
        else:
            assert np.array_equal(pipeline.qual_decode(member), want)


@pytest.mark.parametrize("name,q", qc.degenerate(), ids=[c[0] for c in qc.degenerate()])
def test_size_bound_against_the_rans_member(name, q):
    """.mcq <= the `.rans` member of the flat bytes + the header"""
    from minicom_amd import pipeline
    assert len(pipeline.qual_encode(q)) <= len(_rans(q)) + HEADER


def test_size_gain_on_binned_qualities():
    """synth_quals(5, 8000, 100, binned=True): strictly below the `.rans` member of the same bytes.  (An empirical-entropy estimate
    made before the coder existed gave 54.0 KB for model 3 against 58.7 KB for order-1; the coders give 56218 bytes (model 3) against
    60201 for `.rans`: profiles/r10_qual_sizes.json.)"""
    from minicom_amd import pipeline
    q = qc.synth_quals(5, 8000, 100, binned=True)
    mcq, rans = pipeline.qual_encode(q), _rans(q)
    print("mcq %d bytes (kind %d, model %d), rans %d bytes" % (len(mcq), mcq[5], mcq[6], len(rans)))
    assert len(mcq) < len(rans)
    assert np.array_equal(pipeline.qual_decode(mcq), q)


def test_model_choice_is_the_minimum_estimate():
    from minicom_amd import pipeline
    for name, q in qc.degenerate():
        est = pipeline.qual_estimate(q)
        assert est == QR.ref_estimates(q), name
        m = pipeline.qual_encode(q)
        if m[5] == 0:
            assert m[6] == (0 if q.shape[0] == 0 else min(range(5), key=lambda k: (est[k], k))), name
        for k in range(1, 5):                                                 # the coded size stays within its estimate
            if q.shape[0]:
                assert len(pipeline.qual_encode(q, k)) <= est[k], (name, k)


# ---- surface ----------------------------------------------------------------------------------------------------------------------------
def test_the_headers_declare_and_the_libraries_export_the_new_entries():
    import minicom_amd
    from minicom_amd import pipeline
    strip = lambda p: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", p)).read(), flags=re.S)
    dev, host, hooks = strip("mcom.h"), strip("mcom_host.h"), strip("mcom_test.h")
    lib, hl = minicom_amd.load_library(), pipeline.load_host_library()
    for name in ("mcom_qual_bound", "mcom_qual_encode", "mcom_qual_info", "mcom_qual_decode"):
        assert re.search(r"\b%s\s*\(" % name, dev) and hasattr(lib, name), name
    assert re.search(r"\bmcom_test_qual_hist\s*\(", hooks) and hasattr(lib, "mcom_test_qual_hist")
    for name in ("mcomh_qual_bound", "mcomh_qual_encode", "mcomh_qual_decode", "mcomh_qual_info"):
        assert re.search(r"\b%s\s*\(" % name, host) and hasattr(hl, name) and name in pipeline.HOST_ABI_SYMBOLS, name
    for name in ("qual_encode", "qual_decode"):
        assert callable(getattr(pipeline, name)) and callable(getattr(minicom_amd.Context, name)), name


def test_info_and_bound():
    from minicom_amd import McomError, pipeline
    lib = pipeline.load_host_library()
    assert lib.mcomh_qual_bound(10, 0) == 0 and lib.mcomh_qual_bound(10, 257) == 0
    q = qc.synth_quals(2, 30, 64)
    for model in (None, 0, 1, 2, 3, 4, "rans"):
        assert len(pipeline.qual_encode(q, model)) <= lib.mcomh_qual_bound(30, 64)
    with pytest.raises(McomError):
        pipeline.qual_info(b"MCRS" + bytes(60))
    with pytest.raises(McomError):
        pipeline.qual_info(pipeline.qual_encode(q)[:63])


def test_the_gpu_entries_fail_loudly_without_a_gpu():
    import torch
    import minicom_amd
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(minicom_amd.McomError):
        minicom_amd.Context(0)
    lib = minicom_amd.load_library()
    assert lib.mcom_qual_encode(None, None, 0, 100, 100, None, 0, None, 0) == -1
    assert lib.mcom_qual_decode(None, None, 0, None, 0, 0, None, None) == -1


# ---- surface of `minicom -Q` (no GPU) -------------------------------------------------------------------------------------------------
NO_GPU = 99                                                   # a device number no box has: the same answer with and without a card


def _order_archive(golden_dir, d, quals):
    """the golden -p stream files of stages_L100 in folder d, plus a host-coded qual.mcq; returns the reads as a uint8 matrix"""
    import gzip
    import io
    import tarfile
    from minicom_amd import pipeline
    d.mkdir()
    with gzip.open(os.path.join(golden_dir, "streams_order_stages_L100.tar.gz"), "rb") as g:
        tf = tarfile.open(fileobj=io.BytesIO(g.read()))
        for m in tf.getmembers():
            (d / m.name).write_bytes(tf.extractfile(m).read())
    with gzip.open(os.path.join(golden_dir, "stages_L100.reads.gz"), "rb") as f:
        rows = f.read().split(b"\n")[:-1]
    reads = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), 100)
    if quals is not None:
        (d / "qual.mcq").write_bytes(pipeline.qual_encode(quals(len(rows))))
    return reads


def test_host_route_gives_the_fastq_back(golden_dir, tmp_path):
    """golden -p streams + a host-coded qual.mcq -> mcomh_decompress_fastq -> the input FASTQ byte for byte (names @1 .., third line +),
    through the library, the `decompress --fastq` executable and container.decompress_file"""
    import tarfile
    from minicom_amd import container, pipeline
    quals = qc.synth_quals(21, 2000, 100)
    d = tmp_path / "arch"
    reads = _order_archive(golden_dir, d, lambda n: np.resize(quals, (n, 100)))
    n = reads.shape[0]
    want = qc.fastq_bytes(reads, np.resize(quals, (n, 100)))
    out = tmp_path / "out.fastq"
    assert pipeline.decompress_fastq(str(d), str(out)) == n
    assert out.read_bytes() == want
    p = subprocess.run([os.path.join(ROOT, "bin", "decompress"), "--fastq", str(d), str(tmp_path / "out2.fastq")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.split()[0] == str(n), p.stdout + p.stderr
    assert (tmp_path / "out2.fastq").read_bytes() == want
    # the container keeps qual.mcq as it is, reports it, and decodes such an archive to FASTQ
    arc = str(tmp_path / "a.minicom")
    sizes = container.pack(str(d), arc, codec="rans")
    assert sizes["qual.mcq"] == (d / "qual.mcq").stat().st_size
    with tarfile.open(arc) as t:
        assert t.extractfile("qual.mcq").read() == (d / "qual.mcq").read_bytes()
    kinds = container.unpack(arc, str(tmp_path / "back"))
    assert kinds == {"order": True, "paired": False, "quality": True}
    assert container.decompress_file(arc, str(tmp_path / "out3.fastq")) == n
    assert (tmp_path / "out3.fastq").read_bytes() == want


def test_host_route_refuses_what_does_not_fit(golden_dir, tmp_path):
    """no qual.mcq, one of another n, one of another L, a damaged one, and a folder that is not a -p archive: an error, no output file"""
    import gzip
    import io
    import tarfile
    from minicom_amd import McomError, pipeline
    cases = {"none": None, "n": lambda n: qc.synth_quals(1, n - 1, 100), "L": lambda n: qc.synth_quals(1, n, 99)}
    for name, quals in cases.items():
        d = tmp_path / name
        _order_archive(golden_dir, d, quals)
        with pytest.raises(McomError):
            pipeline.decompress_fastq(str(d), str(tmp_path / (name + ".fastq")))
        assert not (tmp_path / (name + ".fastq")).exists(), name
    d = tmp_path / "damaged"
    _order_archive(golden_dir, d, lambda n: qc.synth_quals(1, n, 100))
    b = bytearray((d / "qual.mcq").read_bytes()); b[len(b) // 2] ^= 4; (d / "qual.mcq").write_bytes(bytes(b))
    with pytest.raises(McomError):
        pipeline.decompress_fastq(str(d), str(tmp_path / "damaged.fastq"))
    assert not (tmp_path / "damaged.fastq").exists()
    d = tmp_path / "default"; d.mkdir()
    with gzip.open(os.path.join(golden_dir, "streams_stages_L100.tar.gz"), "rb") as g:
        tf = tarfile.open(fileobj=io.BytesIO(g.read()))
        for m in tf.getmembers():
            (d / m.name).write_bytes(tf.extractfile(m).read())
    (d / "qual.mcq").write_bytes(pipeline.qual_encode(qc.synth_quals(1, 10, 100)))
    with pytest.raises(McomError):
        pipeline.decompress_fastq(str(d), str(tmp_path / "default.fastq"))
    assert not (tmp_path / "default.fastq").exists()


def test_Q_is_refused_without_p_and_with_paired_files(tmp_path):
    (tmp_path / "x.fastq").write_bytes(b"@1\nACGT\n+\nIIII\n")
    for args in (["-r", "x.fastq", "-Q"], ["-1", "x.fastq", "-2", "x.fastq", "-Q"]):
        p = subprocess.run(["bash", os.path.join(ROOT, "bin", "minicom")] + args, cwd=tmp_path, capture_output=True, text=True)
        assert p.returncode == 1 and "-Q needs -p" in p.stdout, (args, p.stdout + p.stderr)
        assert not list(tmp_path.glob("*.minicom")) and not list(tmp_path.glob("*_comp*"))
    usage = subprocess.run(["bash", os.path.join(ROOT, "bin", "minicom"), "-h"], capture_output=True, text=True).stdout
    assert "-Q" in usage and "names" in usage
    from minicom_amd import container
    for kw in ({"order": False}, {"order": True, "path2": "y.fastq"}):
        with pytest.raises(ValueError):
            container.compress_fastq(str(tmp_path / "x.fastq"), str(tmp_path / "x.minicom"), quality=True, **kw)


def test_the_fastq_surface_exists_and_fails_loudly_without_a_gpu(golden_dir, tmp_path):
    import ctypes as C
    import minicom_amd
    from minicom_amd import McomError, container, pipeline
    strip = lambda p: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", p)).read(), flags=re.S)
    dev, host = strip("mcom.h"), strip("mcom_host.h")
    lib, hl = minicom_amd.load_library(), pipeline.load_host_library()
    for name in ("mcom_fastq_quality_rows", "mcom_fastq_emit"):
        assert re.search(r"\b%s\s*\(" % name, dev) and hasattr(lib, name), name
    for name in ("mcomh_fastq_qualities_to_device", "mcomh_decompress_fastq", "mcomh_decompress_fastq_gpu", "mcomh_verify_quality_gpu", "mcomh_qual_pack_file", "mcomh_qual_unpack_file"):
        assert re.search(r"\b%s\s*\(" % name, host) and hasattr(hl, name) and name in pipeline.HOST_ABI_SYMBOLS, name
    for name in ("fastq_qualities", "decompress_fastq", "verify_quality"):
        assert callable(getattr(pipeline, name)), name
    for name in ("fastq_qualities", "fastq_emit", "qual_test_hist"):
        assert callable(getattr(minicom_amd.Context, name)), name
    assert "quality" in container.compress_fastq.__code__.co_varnames
    # no such GPU: an error, never the host route, no output file
    d = tmp_path / "arch"
    reads = _order_archive(golden_dir, d, lambda n: qc.synth_quals(1, n, 100))
    fq = tmp_path / "in.fastq"
    fq.write_bytes(qc.fastq_bytes(reads, qc.synth_quals(1, reads.shape[0], 100)))
    with pytest.raises(McomError):
        pipeline.decompress_fastq(str(d), str(tmp_path / "o.fastq"), device=NO_GPU)
    assert not (tmp_path / "o.fastq").exists()
    with pytest.raises(McomError):
        pipeline.verify_quality(str(d), str(fq), device=NO_GPU)
    err = C.create_string_buffer(320); dp, n = C.c_void_p(), C.c_size_t()
    assert hl.mcomh_fastq_qualities_to_device(os.fsencode(str(fq)), NO_GPU, 100, 0, C.byref(dp), C.byref(n), err, 320) != 0 and b"GPU" in err.value
    raw = tmp_path / "q.raw"; raw.write_bytes(qc.synth_quals(1, 50, 100).tobytes())
    assert hl.mcomh_qual_pack_file(os.fsencode(str(raw)), os.fsencode(str(tmp_path / "q.mcq")), 100, NO_GPU) != 0 and not (tmp_path / "q.mcq").exists()
    assert lib.mcom_fastq_emit(None, None, 0, None, 0, 0, 0, 100, None, None) == -1


def test_mcomz_qual_round_trip_and_corrupt_member(tmp_path):
    """mcomz e --qual L IN OUT on the host, d by the magic; the member is the library's; a damaged one leaves no output file"""
    from minicom_amd import pipeline
    q = qc.synth_quals(4, 300, 75)
    exe = os.path.join(ROOT, "bin", "mcomz")
    (tmp_path / "q.raw").write_bytes(q.tobytes())
    assert subprocess.run([exe, "e", "--qual", "75", "q.raw", "q.mcq"], cwd=tmp_path).returncode == 0
    assert (tmp_path / "q.mcq").read_bytes() == pipeline.qual_encode(q)
    assert subprocess.run([exe, "d", "q.mcq", "q.back"], cwd=tmp_path).returncode == 0
    assert (tmp_path / "q.back").read_bytes() == q.tobytes()
    b = bytearray((tmp_path / "q.mcq").read_bytes()); b[-3] ^= 1; (tmp_path / "bad.mcq").write_bytes(bytes(b))
    p = subprocess.run([exe, "d", "bad.mcq", "bad.back"], cwd=tmp_path, capture_output=True, text=True)
    assert p.returncode == 1 and ".mcq" in p.stderr and not (tmp_path / "bad.back").exists()
    assert subprocess.run([exe, "e", "--qual", "76", "q.raw", "x.mcq"], cwd=tmp_path, capture_output=True).returncode == 1 and not (tmp_path / "x.mcq").exists()


def test_fastq_to_member_on_the_host_checks_every_record(tmp_path):
    """mcomh_fastq_quality_member without a GPU (what `minicom -Q` runs without -G, `mcomz e --fastq-qual L`): the member is the coder's
    for the file's quality lines (plain, without the last newline, gzip); a CRLF line, a short line balanced by a long one, a byte 127,
    a missing '@' or '+' and a file that ends inside a record are errors that name the record and leave no output file"""
    import gzip
    from minicom_amd import McomError, pipeline
    reads, quals, text = qc.tricky_fastq()
    want = pipeline.qual_encode(quals)
    (tmp_path / "t.fastq").write_bytes(text)
    (tmp_path / "nonl.fastq").write_bytes(text[:-1])
    with gzip.open(tmp_path / "t.fastq.gz", "wb") as f:
        f.write(text)
    for name in ("t.fastq", "nonl.fastq", "t.fastq.gz"):
        assert pipeline.fastq_quality_member(str(tmp_path / name), 37, str(tmp_path / "m.mcq")) == 120
        assert (tmp_path / "m.mcq").read_bytes() == want, name
    exe = os.path.join(ROOT, "bin", "mcomz")
    p = subprocess.run([exe, "e", "--fastq-qual", "37", "t.fastq", "cli.mcq"], cwd=tmp_path, capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.split() == ["120"] and (tmp_path / "cli.mcq").read_bytes() == want, p.stdout + p.stderr
    for name, t in qc.bad_fastqs().items():
        (tmp_path / "bad.fastq").write_bytes(t)
        with pytest.raises(McomError, match=r"record 18 "):
            pipeline.fastq_quality_member(str(tmp_path / "bad.fastq"), 37, str(tmp_path / "bad.mcq"))
        assert not (tmp_path / "bad.mcq").exists(), name
        p = subprocess.run([exe, "e", "--fastq-qual", "37", "bad.fastq", "bad.mcq"], cwd=tmp_path, capture_output=True, text=True)
        assert p.returncode == 1 and "record 18 " in p.stderr and not (tmp_path / "bad.mcq").exists(), (name, p.stderr)
    (tmp_path / "cut.fastq").write_bytes(text[:-60])
    with pytest.raises(McomError, match=r"ends inside record 120"):
        pipeline.fastq_quality_member(str(tmp_path / "cut.fastq"), 37, str(tmp_path / "cut.mcq"))
    with pytest.raises(McomError):
        pipeline.fastq_quality_member(str(tmp_path / "t.fastq"), 37, str(tmp_path / "x.mcq"), device=NO_GPU)
    assert not (tmp_path / "cut.mcq").exists() and not (tmp_path / "x.mcq").exists()
