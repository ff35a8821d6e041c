"""Quality values in an archive's own order (`minicom -q`), the parts that need no GPU: the host twin of the row
gather against numpy and its refusals, the two host decoders over the golden default and paired-end stream files, the invariance of the
quality coder's choices under a permutation of the rows, and the command line's and the Python surface's refusals."""
import gzip
import io
import os
import re
import subprocess
import tarfile

import numpy as np
import pytest

import qual_cases as qc
import qual_reference as QR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_GPU = 99                                                   # a device number no box has: the same answer with and without a card
L100 = 100


# ---- the host gather ---------------------------------------------------------------------------------------------------------------------
def _host_gather(rows, pitch_in, order, pitch_out, n_src=None):
    """mcomh_qual_gather_rows on a matrix laid out at pitch_in, into canary bytes at pitch_out; returns (rc, flag, out buffer)"""
    import ctypes as C
    from minicom_amd import pipeline
    n, L = rows.shape
    n_src = n if n_src is None else n_src
    src = np.full(max(n, 1) * pitch_in + 8, 0xEE, dtype=np.uint8)
    for i in range(n):
        src[i * pitch_in:i * pitch_in + L] = rows[i]
    o = np.asarray(order, dtype=np.uint32)
    out = np.full(max(len(o), 1) * pitch_out + 8, 0xA5, dtype=np.uint8)
    flag = C.c_uint32(0)
    rc = pipeline.load_host_library().mcomh_qual_gather_rows(src.ctypes.data, n_src, L, pitch_in, o.ctypes.data if len(o) else None, len(o), out.ctypes.data, pitch_out, C.byref(flag))
    return rc, flag.value, out


@pytest.mark.parametrize("L", [1, 15, 16, 17, 100, 256])
@pytest.mark.parametrize("n", [0, 1, 17])
def test_host_gather_is_numpy_fancy_indexing(n, L):
    from minicom_amd import pipeline
    rng = np.random.default_rng(1000 * n + L)
    rows = rng.integers(33, 127, (n, L), dtype=np.uint8)
    order = rng.permutation(n).astype(np.uint32)
    assert np.array_equal(pipeline.qual_gather(rows, order), rows[order])
    assert np.array_equal(pipeline.qual_gather(rows, order.astype("<u4").tobytes()), rows[order])        # the bytes of a read_order.bin
    for pitch_in, pitch_out in ((L, L), (L + 1, L), (L, L + 1), (L + 1, L + 1)):
        rc, flag, out = _host_gather(rows, pitch_in, order, pitch_out)
        assert rc == 0 and flag == 0
        img = out[:max(n, 1) * pitch_out].reshape(max(n, 1), pitch_out)
        assert np.array_equal(img[:n, :L], rows[order])
        assert (img[:n, L:] == 0xA5).all() and (out[n * pitch_out:] == 0xA5).all()                      # nothing beside the rows is written


def test_host_gather_refusals(tmp_path):
    from minicom_amd import McomError, pipeline
    rng = np.random.default_rng(3)
    n, L = 17, 37
    rows = rng.integers(33, 127, (n, L), dtype=np.uint8)
    good = rng.permutation(n).astype(np.uint32)
    dup = good.copy(); dup[5] = dup[11]
    beyond = good.copy(); beyond[3] = n
    for bad, word in ((dup, "twice"), (beyond, "beyond")):
        with pytest.raises(McomError, match=word):
            pipeline.qual_gather(rows, bad)
    with pytest.raises(McomError, match="entries"):
        pipeline.qual_gather(rows, good[:-1])                                                           # a count mismatch
    with pytest.raises(McomError, match="multiple of 4"):
        pipeline.qual_gather(rows, good.astype("<u4").tobytes() + b"\0")                                # an order file of 4 k + 1 bytes
    (tmp_path / "o.bin").write_bytes(good.astype("<u4").tobytes()[:-3])
    with pytest.raises(McomError, match="multiple of 4"):
        pipeline.qual_gather(rows, str(tmp_path / "o.bin"))
    # the flags themselves: the rows of good indices are still right, the row of a bad index is not touched
    rc, flag, out = _host_gather(rows, L, dup, L)
    assert rc == 0 and flag == 2 and np.array_equal(out[:n * L].reshape(n, L), rows[dup])
    rc, flag, out = _host_gather(rows, L, beyond, L)
    img = out[:n * L].reshape(n, L)
    keep = np.arange(n) != 3
    assert rc == 0 and flag == 1 and np.array_equal(img[keep], rows[beyond[keep]]) and (img[3] == 0xA5).all()
    both = dup.copy(); both[0] = 2 ** 32 - 1
    assert _host_gather(rows, L, both, L)[:2] == (0, 3)
    # the arguments the device call refuses
    assert _host_gather(rows, L - 1, good, L)[0] == -1 and _host_gather(rows, L, good, L - 1)[0] == -1
    lib = pipeline.load_host_library()
    assert lib.mcomh_qual_gather_rows(None, 0, 0, 0, None, 0, None, 0, None) == -1
    assert lib.mcomh_qual_gather_rows(rows.ctypes.data, n, 257, 257, good.ctypes.data, n, rows.ctypes.data, 257, None) == -1


def _write_fastq(path, reads, quals):
    path.write_bytes(qc.fastq_bytes(reads, quals))


def test_mcomz_order_on_the_host(tmp_path):
    """mcomz e --fastq-qual L --order FILE: the member of the permuted rows; every bad order file is exit status 1, a message, no member"""
    from minicom_amd import pipeline
    rng = np.random.default_rng(8)
    n, L = 200, 51
    reads = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, L))]
    quals = qc.synth_quals(5, n, L)
    _write_fastq(tmp_path / "in.fastq", reads, quals)
    order = rng.permutation(n).astype("<u4")
    (tmp_path / "ok.bin").write_bytes(order.tobytes())
    exe = os.path.join(ROOT, "bin", "mcomz")
    p = subprocess.run([exe, "e", "--fastq-qual", str(L), "--order", "ok.bin", "in.fastq", "ok.mcq"], cwd=tmp_path, capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.split() == [str(n)], p.stdout + p.stderr
    assert (tmp_path / "ok.mcq").read_bytes() == pipeline.qual_encode(quals[order])
    assert pipeline.fastq_quality_member(str(tmp_path / "in.fastq"), L, str(tmp_path / "lib.mcq"), order_path=str(tmp_path / "ok.bin")) == n
    assert (tmp_path / "lib.mcq").read_bytes() == (tmp_path / "ok.mcq").read_bytes()
    dup = order.copy(); dup[7] = dup[8]
    beyond = order.copy(); beyond[0] = n
    bad = {"short": order[:-1].tobytes(), "long": order.tobytes() + (0).to_bytes(4, "little"), "ragged": order.tobytes() + b"\1", "dup": dup.tobytes(), "beyond": beyond.tobytes()}
    words = {"short": "entries", "long": "entries", "ragged": "multiple of 4", "dup": "twice", "beyond": "beyond"}
    for name, data in bad.items():
        (tmp_path / (name + ".bin")).write_bytes(data)
        p = subprocess.run([exe, "e", "--fastq-qual", str(L), "--order", name + ".bin", "in.fastq", name + ".mcq"], cwd=tmp_path, capture_output=True, text=True)
        assert p.returncode == 1 and words[name] in p.stderr and not (tmp_path / (name + ".mcq")).exists(), (name, p.stderr)
    p = subprocess.run([exe, "e", "--qual", str(L), "--order", "ok.bin", "in.fastq", "x.mcq"], cwd=tmp_path, capture_output=True, text=True)
    assert p.returncode == 1 and "usage" in p.stderr and not (tmp_path / "x.mcq").exists()           # --order goes with --fastq-qual only


# ---- the host decoders over the golden stream files --------------------------------------------------------------------------------------
def _extract(golden_dir, name, d):
    d.mkdir()
    with gzip.open(os.path.join(golden_dir, name), "rb") as g:
        tf = tarfile.open(fileobj=io.BytesIO(g.read()))
        for m in tf.getmembers():
            (d / m.name).write_bytes(tf.extractfile(m).read())


def _rows_of(path, L):
    lines = path.read_bytes().split(b"\n")[:-1]
    return np.frombuffer(b"".join(lines), dtype=np.uint8).reshape(len(lines), L)


def _row_quals(seed, n, L):
    """a quality row derived from its row number j: column j % L holds one value, the rest is synthetic -- no two rows alike"""
    q = qc.synth_quals(seed, n, L).copy()
    j = np.arange(n)
    q[j, j % L] = 33 + (j // L) % 94
    return q


@pytest.fixture(scope="module")
def default_archive(golden_dir, tmp_path_factory):
    """the golden default-mode stream files of stages_L100 with a host-coded rqual.mcq; (folder, rows in the decoder's order, qualities)"""
    from minicom_amd import pipeline
    base = tmp_path_factory.mktemp("rq_default")
    d = base / "arch"
    _extract(golden_dir, "streams_stages_L100.tar.gz", d)
    n = pipeline.decompress(str(d), str(base / "rows.txt"))
    rows = _rows_of(base / "rows.txt", L100)
    assert rows.shape[0] == n
    quals = _row_quals(31, n, L100)
    (d / "rqual.mcq").write_bytes(pipeline.qual_encode(quals))
    return d, rows, quals


@pytest.fixture(scope="module")
def paired_archive(golden_dir, tmp_path_factory):
    from minicom_amd import pipeline
    base = tmp_path_factory.mktemp("rq_pe")
    d = base / "arch"
    _extract(golden_dir, "streams_pe_stages_L100.tar.gz", d)
    n = pipeline.decompress_pe(str(d), str(base / "r1.txt"), str(base / "r2.txt"))
    r1, r2 = _rows_of(base / "r1.txt", L100), _rows_of(base / "r2.txt", L100)
    assert r1.shape[0] == r2.shape[0] == n
    q1, q2 = _row_quals(32, n, L100), _row_quals(33, n, L100)
    (d / "rqual_1.mcq").write_bytes(pipeline.qual_encode(q1))
    (d / "rqual_2.mcq").write_bytes(pipeline.qual_encode(q2))
    return d, (r1, r2), (q1, q2)


def test_host_decoder_of_the_default_mode(default_archive, tmp_path):
    """rows of the default decoder + rqual.mcq -> records `@<j+1>`, read, `+`, qualities: library, executable, container"""
    from minicom_amd import container, pipeline
    d, rows, quals = default_archive
    n = rows.shape[0]
    want = qc.fastq_bytes(rows, quals)
    assert pipeline.decompress_fastq_reordered(str(d), str(tmp_path / "a.fastq")) == n
    assert (tmp_path / "a.fastq").read_bytes() == want
    p = subprocess.run([os.path.join(ROOT, "bin", "decompress"), "--fastq-reordered", str(d), str(tmp_path / "b.fastq")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.split()[0] == str(n), p.stdout + p.stderr
    assert (tmp_path / "b.fastq").read_bytes() == want
    arc = str(tmp_path / "a.minicom")
    sizes = container.pack(str(d), arc, codec="rans")
    assert sizes["rqual.mcq"] == (d / "rqual.mcq").stat().st_size and "read_order.bin" not in sizes
    assert container.unpack(arc, str(tmp_path / "back")) == {"order": False, "paired": False, "quality_reordered": True}
    assert (tmp_path / "back" / "rqual.mcq").read_bytes() == (d / "rqual.mcq").read_bytes()
    assert container.decompress_file(arc, str(tmp_path / "c.fastq")) == n
    assert (tmp_path / "c.fastq").read_bytes() == want
    # what mcomh_decompress_fastq refused before, it still refuses: this is not a -p archive
    with pytest.raises(pipeline.McomError):
        pipeline.decompress_fastq(str(d), str(tmp_path / "no.fastq"))
    assert not (tmp_path / "no.fastq").exists()


def test_host_decoder_of_the_paired_end_mode(paired_archive, tmp_path):
    from minicom_amd import container, pipeline
    d, (r1, r2), (q1, q2) = paired_archive
    n = r1.shape[0]
    want = (qc.fastq_bytes(r1, q1), qc.fastq_bytes(r2, q2))
    assert pipeline.decompress_fastq_pe(str(d), str(tmp_path / "a1.fastq"), str(tmp_path / "a2.fastq")) == n
    assert ((tmp_path / "a1.fastq").read_bytes(), (tmp_path / "a2.fastq").read_bytes()) == want
    p = subprocess.run([os.path.join(ROOT, "bin", "decompress"), "--fastq-pe", str(d), str(tmp_path / "b1.fastq"), str(tmp_path / "b2.fastq")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.split()[0] == str(n), p.stdout + p.stderr
    assert ((tmp_path / "b1.fastq").read_bytes(), (tmp_path / "b2.fastq").read_bytes()) == want
    arc = str(tmp_path / "a.minicom")
    sizes = container.pack(str(d), arc, codec="rans")
    assert sizes["rqual_1.mcq"] == (d / "rqual_1.mcq").stat().st_size and sizes["rqual_2.mcq"] == (d / "rqual_2.mcq").stat().st_size
    assert container.unpack(arc, str(tmp_path / "back")) == {"order": False, "paired": True, "quality_reordered": True}
    with pytest.raises(ValueError):
        container.decompress_file(arc, str(tmp_path / "c1.fastq"))
    assert container.decompress_file(arc, str(tmp_path / "c1.fastq"), str(tmp_path / "c2.fastq")) == n
    assert ((tmp_path / "c1.fastq").read_bytes(), (tmp_path / "c2.fastq").read_bytes()) == want


def _copy(src, dst):
    dst.mkdir()
    for f in src.iterdir():
        (dst / f.name).write_bytes(f.read_bytes())


def _refused(tmp_path, d, paired, device=None):
    from minicom_amd import McomError, pipeline
    outs = [tmp_path / (d.name + "_1.fastq"), tmp_path / (d.name + "_2.fastq")]
    with pytest.raises(McomError):
        if paired:
            pipeline.decompress_fastq_pe(str(d), str(outs[0]), str(outs[1]), device=device)
        else:
            pipeline.decompress_fastq_reordered(str(d), str(outs[0]), device=device)
    return not outs[0].exists() and not outs[1].exists()


def test_host_decoders_refuse_what_does_not_fit(golden_dir, default_archive, paired_archive, tmp_path):
    """a -p archive, an archive of the other kind, a missing member, a member of another n or L, a damaged member, a pair with one member:
    an error and no output file -- of two outputs, neither"""
    from minicom_amd import pipeline
    d0, rows, quals = default_archive
    dp, (r1, r2), (q1, q2) = paired_archive
    n, npair = rows.shape[0], r1.shape[0]
    # a -p archive, whatever members it carries
    d = tmp_path / "order"
    _extract(golden_dir, "streams_order_stages_L100.tar.gz", d)
    for name in ("rqual.mcq", "rqual_1.mcq", "rqual_2.mcq"):
        (d / name).write_bytes(pipeline.qual_encode(qc.synth_quals(1, n, L100)))
    assert _refused(tmp_path, d, False) and _refused(tmp_path, d, True)
    # the other kind
    d = tmp_path / "pe_as_default"; _copy(dp, d); (d / "rqual.mcq").write_bytes(pipeline.qual_encode(qc.synth_quals(1, 2 * npair, L100)))
    assert _refused(tmp_path, d, False)
    d = tmp_path / "default_as_pe"; _copy(d0, d)
    for name in ("rqual_1.mcq", "rqual_2.mcq"):
        (d / name).write_bytes(pipeline.qual_encode(qc.synth_quals(1, n // 2, L100)))
    assert _refused(tmp_path, d, True)
    # the member
    cases = {"none": None, "n": qc.synth_quals(1, n - 1, L100), "L": qc.synth_quals(1, n, L100 - 1)}
    for name, q in cases.items():
        d = tmp_path / ("d_" + name); _copy(d0, d); (d / "rqual.mcq").unlink()
        if q is not None:
            (d / "rqual.mcq").write_bytes(pipeline.qual_encode(q))
        assert _refused(tmp_path, d, False), name
    d = tmp_path / "d_damaged"; _copy(d0, d)
    b = bytearray((d / "rqual.mcq").read_bytes()); b[len(b) // 2] ^= 4; (d / "rqual.mcq").write_bytes(bytes(b))
    assert _refused(tmp_path, d, False)
    for which in ("rqual_1.mcq", "rqual_2.mcq"):
        for name, q in {"none": None, "n": qc.synth_quals(1, npair + 1, L100), "L": qc.synth_quals(1, npair, L100 + 1)}.items():
            d = tmp_path / ("p_%s_%s" % (which[6], name)); _copy(dp, d); (d / which).unlink()
            if q is not None:
                (d / which).write_bytes(pipeline.qual_encode(q))
            assert _refused(tmp_path, d, True), (which, name)
        d = tmp_path / ("p_%s_damaged" % which[6]); _copy(dp, d)
        b = bytearray((d / which).read_bytes()); b[len(b) // 2] ^= 4; (d / which).write_bytes(bytes(b))
        assert _refused(tmp_path, d, True), which
    # a stream file is missing
    d = tmp_path / "d_nostream"; _copy(d0, d); (d / "single.seq").unlink()
    assert _refused(tmp_path, d, False)


# ---- the coder's choices do not depend on the row order ----------------------------------------------------------------------------------
def test_row_order_does_not_change_what_the_coder_chooses():
    """The counts the model choice and the tables are made of are sums over rows (section 3.9: the context of a column is row-local), so a
    permutation of the rows changes neither; section 3.9 bounds a member by the estimate of its model."""
    from minicom_amd import pipeline
    q = qc.synth_quals(11, 4000, L100)
    perm = np.random.default_rng(11).permutation(4000)
    a, b = pipeline.qual_encode(q), pipeline.qual_encode(q[perm])
    ha, hb = QR.parse_header(a), QR.parse_header(b)
    assert (ha["kind"], ha["model"], ha["table_bytes"]) == (hb["kind"], hb["model"], hb["table_bytes"])
    assert a[QR.HEADER:QR.HEADER + ha["table_bytes"]] == b[QR.HEADER:QR.HEADER + hb["table_bytes"]] and ha["map"] == hb["map"]
    ea, eb = pipeline.qual_estimate(q), pipeline.qual_estimate(q[perm])
    assert ea == eb
    assert ha["kind"] == 0                                                          # (the context model wins on this input: the estimate below is its model's)
    assert len(a) <= ea[ha["model"]] and len(b) <= eb[hb["model"]]
    for model in (1, 2, 3, 4):
        fa, fb = pipeline.qual_encode(q, model), pipeline.qual_encode(q[perm], model)
        t = QR.parse_header(fa)["table_bytes"]
        assert t == QR.parse_header(fb)["table_bytes"] and fa[QR.HEADER:QR.HEADER + t] == fb[QR.HEADER:QR.HEADER + t], model
        assert len(fa) <= ea[model] and len(fb) <= ea[model], model
    assert np.array_equal(pipeline.qual_decode(b), q[perm])


# ---- the command line and the Python surface --------------------------------------------------------------------------------------------
def test_q_is_refused_with_p_Q_and_N(tmp_path):
    (tmp_path / "x.fastq").write_bytes(b"@1\nACGT\n+\nIIII\n")
    cases = (["-r", "x.fastq", "-q", "-p"], ["-r", "x.fastq", "-q", "-Q"], ["-r", "x.fastq", "-q", "-N"], ["-r", "x.fastq", "-p", "-Q", "-N", "-q"],
             ["-1", "x.fastq", "-2", "x.fastq", "-q", "-Q"], ["-1", "x.fastq", "-2", "x.fastq", "-N", "-q"], ["-1", "x.fastq", "-2", "x.fastq", "-q", "-p"])
    for args in cases:
        p = subprocess.run(["bash", os.path.join(ROOT, "bin", "minicom")] + args, cwd=tmp_path, capture_output=True, text=True)
        out = p.stdout + p.stderr
        assert p.returncode == 1 and "-q" in out and "-p -Q" in out, (args, out)
        assert "-Q needs -p" not in out and "-N needs" not in out, (args, out)
        assert not list(tmp_path.glob("*.minicom")) and not list(tmp_path.glob("*_comp*")), args
    usage = subprocess.run(["bash", os.path.join(ROOT, "bin", "minicom"), "-h"], capture_output=True, text=True).stdout
    assert re.search(r"^\s*-q\s", usage, flags=re.M) and "own order" in usage
    from minicom_amd import container
    for kw in ({"order": True}, {"quality": True, "order": True}, {"names": True, "quality": True, "order": True}):
        with pytest.raises(ValueError):
            container.compress_fastq(str(tmp_path / "x.fastq"), str(tmp_path / "x.minicom"), quality_reordered=True, **kw)
    assert not list(tmp_path.glob("*.minicom"))


def test_the_surface_exists_and_fails_loudly_without_a_gpu(default_archive, paired_archive, tmp_path):
    import ctypes as C
    import minicom_amd
    from minicom_amd import McomError, container, pipeline
    strip = lambda p: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", p)).read(), flags=re.S)
    dev, host = strip("mcom.h"), strip("mcom_host.h")
    lib, hl = minicom_amd.load_library(), pipeline.load_host_library()
    for name in ("mcom_dump_read_order", "mcom_qual_gather_rows", "mcom_verify_multiset_parts"):
        assert re.search(r"\b%s\s*\(" % name, dev) and hasattr(lib, name) and name in minicom_amd.ABI_SYMBOLS, name
    for name in ("mcomh_keep_read_order", "mcomh_qual_gather_rows", "mcomh_fastq_quality_member_ordered", "mcomh_decompress_fastq_reordered", "mcomh_decompress_fastq_reordered_gpu",
                 "mcomh_decompress_fastq_pe", "mcomh_decompress_fastq_pe_gpu", "mcomh_verify_records_gpu"):
        assert re.search(r"\b%s\s*\(" % name, host) and hasattr(hl, name) and name in pipeline.HOST_ABI_SYMBOLS, name
    for name in ("qual_gather", "decompress_fastq_reordered", "decompress_fastq_pe", "verify_records"):
        assert callable(getattr(pipeline, name)), name
    for name in ("dump_read_order", "qual_gather_rows", "verify_multiset_parts"):
        assert callable(getattr(minicom_amd.Context, name)), name
    assert callable(pipeline.Pipeline.keep_read_order) and "quality_reordered" in container.compress_fastq.__code__.co_varnames
    # no such GPU: an error, never the host route, no output file
    d0, rows, quals = default_archive
    dp, (r1, r2), (q1, q2) = paired_archive
    assert _refused(tmp_path, d0, False, device=NO_GPU) and _refused(tmp_path, dp, True, device=NO_GPU)
    _write_fastq(tmp_path / "in.fastq", rows, quals)
    with pytest.raises(McomError):
        pipeline.verify_records(str(d0), str(tmp_path / "in.fastq"), device=NO_GPU)
    with pytest.raises(McomError):
        pipeline.qual_gather(quals[:5], np.arange(5), device=NO_GPU)
    (tmp_path / "o.bin").write_bytes(np.arange(rows.shape[0], dtype="<u4").tobytes())
    with pytest.raises(McomError, match="GPU"):
        pipeline.fastq_quality_member(str(tmp_path / "in.fastq"), L100, str(tmp_path / "m.mcq"), device=NO_GPU, order_path=str(tmp_path / "o.bin"))
    assert not (tmp_path / "m.mcq").exists()
    assert lib.mcom_qual_gather_rows(None, None, 0, 100, 100, None, 0, None, 100, None) == -1
    assert lib.mcom_dump_read_order(None, None, 0, None, 0, 0, None, None) == -1
    assert lib.mcom_verify_multiset_parts(None, None, None, 100, None) == -1
    r = pipeline.VerifyReport()
    assert hl.mcomh_verify_records_gpu(os.fsencode(str(d0)), 1, os.fsencode(str(tmp_path / "in.fastq")), None, 0, C.byref(r)) == -1          # mode 1 is not a mode of this call
    assert hl.mcomh_keep_read_order(None, 1) != 0
