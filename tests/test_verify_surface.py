"""The verifier's public surface, checked where there is no GPU: the entry points exist in the headers and both libraries, the Python
wrappers exist, every way of asking without a usable GPU or with bad arguments is an error (never a verdict, never a host comparison),
and the command lines know --verify and -c."""
import ctypes as C
import gzip
import io
import os
import re
import subprocess
import tarfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_GPU = 99                                                   # a device number no box has: the same answer with and without a card


def _streams(golden_dir, d):
    d.mkdir()
    with gzip.open(os.path.join(golden_dir, "streams_stages_L100.tar.gz"), "rb") as g:
        tf = tarfile.open(fileobj=io.BytesIO(g.read()))
        for m in tf.getmembers():
            (d / m.name).write_bytes(tf.extractfile(m).read())


def _fastq(golden_dir, path):
    with gzip.open(os.path.join(golden_dir, "stages_L100.reads.gz"), "rb") as f:
        rows = f.read().split(b"\n")[:-1]
    with open(path, "wb") as f:
        for i, r in enumerate(rows):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))


def test_headers_declare_and_libraries_export_the_verifier():
    import minicom_amd
    from minicom_amd import pipeline
    host = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcom_host.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mcomh_verify_gpu\s*\(", host) and "mcomh_verify_report" in host
    assert "mcomh_verify_gpu" in pipeline.HOST_ABI_SYMBOLS
    getattr(pipeline.load_host_library(), "mcomh_verify_gpu")
    lib = minicom_amd.load_library()
    for name in ("mcom_verify_ordered", "mcom_verify_multiset", "mcom_verify_room", "mcom_set_verify_hash_bits"):
        assert name in minicom_amd.ABI_SYMBOLS, name
        getattr(lib, name)
    test_h = open(os.path.join(ROOT, "include", "mcom_test.h")).read()
    assert "mcom_set_verify_hash_bits" in test_h and "mcom_set_verify_hash_bits" not in open(os.path.join(ROOT, "include", "mcom.h")).read()


def test_python_wrappers_exist():
    from minicom_amd import container, pipeline
    from minicom_amd.hip import Context
    assert callable(pipeline.verify) and callable(container.verify_file)
    for name in ("verify_multiset", "verify_ordered", "set_verify_hash_bits"):
        assert callable(getattr(Context, name)), name


def test_room_grows_with_the_records():
    import minicom_amd
    lib = minicom_amd.load_library()
    assert lib.mcom_verify_room(0, 0) > 0
    assert lib.mcom_verify_room(20_000_000, 20_000_000) >= 2 * 20_000_000 * (16 + 8) + 20_000_000 * 16     # records, partners, the sort's buffer


def test_no_such_gpu_is_an_error_not_a_verdict(golden_dir, tmp_path):
    from minicom_amd import container, pipeline
    from minicom_amd.hip import McomError
    d = tmp_path / "s"
    _streams(golden_dir, d)
    fq = str(tmp_path / "s.fastq")
    _fastq(golden_dir, fq)
    with pytest.raises(McomError):
        pipeline.verify(str(d), fq, device=NO_GPU)
    arch = str(tmp_path / "s.minicom")
    container.pack(str(d), arch, codec="xz")
    with pytest.raises(McomError):
        container.verify_file(arch, fq, device=NO_GPU)
    with pytest.raises(McomError):
        container.verify_file(str(tmp_path / "absent.minicom"), fq, device=NO_GPU)
    assert sorted(os.listdir(tmp_path)) == ["s", "s.fastq", "s.minicom"]                # no working directory left behind


def test_bad_arguments_are_errors(golden_dir, tmp_path):
    from minicom_amd import pipeline
    from minicom_amd.hip import McomError
    lib = pipeline.load_host_library()
    rep = pipeline.VerifyReport()
    d = tmp_path / "s"
    _streams(golden_dir, d)
    fq = str(tmp_path / "s.fastq")
    _fastq(golden_dir, fq)
    D, F = str(d).encode(), fq.encode()
    for args in ((None, 0, F, None), (D, 0, None, None), (D, -1, F, None), (D, 3, F, None), (D, 2, F, None), (D, 0, F, F), (D, 1, F, F)):
        assert lib.mcomh_verify_gpu(args[0], args[1], args[2], args[3], 0, C.byref(rep)) == -1, args
    assert lib.mcomh_verify_gpu(D, 0, F, None, 0, None) == -1
    # missing paths: an error on any box (no such GPU, or no such file)
    for folder, fastq in ((str(tmp_path / "absent"), fq), (str(d), str(tmp_path / "absent.fastq"))):
        with pytest.raises(McomError):
            pipeline.verify(folder, fastq, device=0)
    with pytest.raises(McomError):
        pipeline.verify(str(d), fq, fastq2=fq, order=True)


def test_command_lines_know_verify(tmp_path):
    exe = os.path.join(ROOT, "bin", "decompress")
    r = subprocess.run([exe, "--verify"], capture_output=True, text=True)
    assert r.returncode == 1 and "decompress --verify DIR IN.fastq" in r.stderr, r.stderr
    r = subprocess.run([exe, "--verify", str(tmp_path / "absent"), str(tmp_path / "absent.fastq"), "false", "false", "1"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.strip() and "verified" not in r.stdout, (r.stdout, r.stderr)
    r = subprocess.run([exe, "--verify", str(tmp_path / "absent"), str(tmp_path / "absent.fastq"), "true", "false", "1"], capture_output=True, text=True)
    assert r.returncode == 1 and "IN_2.fastq" in r.stderr, r.stderr
    r = subprocess.run([os.path.join(ROOT, "bin", "minicom"), "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and re.search(r"^\s*-c\s", r.stdout, flags=re.M) and re.search(r"^\s*-C\s", r.stdout, flags=re.M), r.stdout


def test_minicom_c_with_a_missing_fastq_fails_and_leaves_nothing(golden_dir, tmp_path):
    from minicom_amd import container
    d = tmp_path / "s"
    _streams(golden_dir, d)
    work = tmp_path / "work"; work.mkdir()
    arch = str(work / "x.minicom")
    container.pack(str(d), arch, codec="xz")
    script = os.path.join(ROOT, "bin", "minicom")
    for archive in (arch, str(work / "absent.minicom")):
        r = subprocess.run([script, "-d", archive, "-c", str(work / "missing.fastq")], capture_output=True, text=True, cwd=str(work))
        assert r.returncode != 0, (r.stdout, r.stderr)
        assert sorted(os.listdir(work)) == ["x.minicom"], os.listdir(work)
    # ... and neither does an archive that cannot be unpacked
    fq = str(tmp_path / "s.fastq")
    _fastq(golden_dir, fq)
    r = subprocess.run([script, "-d", str(work / "absent.minicom"), "-c", fq], capture_output=True, text=True, cwd=str(work))
    assert r.returncode != 0 and sorted(os.listdir(work)) == ["x.minicom"], (r.stdout, r.stderr, os.listdir(work))
