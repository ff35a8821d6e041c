"""Lossy quality values on the device (`minicom -b SPEC`): k_qual_lut and k_qual_pblock behind
mcom_qual_transform against the independent reference (tests/qual_lossy_reference.py), bytes and report exactly, at the smallest shapes
at which they can go wrong; the file routes against the host twin; one end-to-end run per archive kind."""
import ctypes as C
import functools
import io
import os
import subprocess
import tarfile

import numpy as np
import pytest

import name_cases as nc
import qual_cases as qc
import qual_lossy_reference as LR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MCOMZ = os.path.join(ROOT, "bin", "mcomz")
CANARY = 0xA5


@pytest.fixture(scope="module")
def ctx():
    import minicom_amd
    return minicom_amd.Context(0)


@functools.lru_cache(maxsize=None)
def _tile_rows():
    import minicom_amd
    return minicom_amd.Context.qual_pblock_tile_rows()


def _matrix(seed, n, L):
    """quality lines on the even rows (blocks of every length), bytes of the whole range 0 .. 255 on the odd ones"""
    q = qc.synth_quals(seed, max(n, 1), L)[:n].copy()
    q[1::2] = np.random.default_rng(seed).integers(0, 256, q[1::2].shape, dtype=np.uint8)
    return q


def _on_device(q, pitch, offset):
    """(buffer, view): q at byte `offset` of a device buffer of canaries, rows `pitch` apart, 64 canaries in front and behind"""
    import torch
    n, L = q.shape
    buf = torch.full((64 + offset + n * pitch + 64,), CANARY, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(buf, (n, L), (pitch, 1), 64 + offset)
    if n:
        view.copy_(torch.from_numpy(q).cuda())
    return buf, view


def _check(ctx, q, spec, pitch, offset, tag):
    n, L = q.shape
    buf, view = _on_device(q, pitch, offset)
    want, rep = LR.transform(q, spec)
    out, got = ctx.qual_transform(view, spec, in_place=True)
    img = buf.cpu().numpy()
    body = img[64 + offset:64 + offset + n * pitch].reshape(n, pitch) if n else np.zeros((0, pitch), np.uint8)
    assert np.array_equal(body[:, :L], want), tag
    assert got == rep, (tag, got, rep)
    assert np.all(body[:, L:] == CANARY), tag                                              # every gap between two rows
    assert np.all(img[:64 + offset] == CANARY) and np.all(img[64 + offset + n * pitch:] == CANARY), tag
    if spec.startswith("pblock"):
        assert got["max_abs"] <= int(spec.split(":")[1]), tag


@pytest.mark.parametrize("spec", ["ill8", "pblock:2"])
@pytest.mark.parametrize("L", [1, 2, 15, 16, 17, 37, 255, 256])
def test_shapes_pitches_and_addresses(ctx, L, spec):
    """n = 0, 1, R - 1, R, R + 1, 3 R + 1 for R the rows of a P-block tile; rows back to back and a byte apart; even, odd and 16-byte
    aligned base addresses; canaries in front, behind and in every gap"""
    R = _tile_rows()
    assert R >= 2
    for n in (0, 1, R - 1, R, R + 1, 3 * R + 1):
        q = _matrix(100 + L, n, L)
        for pitch, offset in ((L, 0), (L, 1), (L + 1, 3), (L + 1, 16)):
            _check(ctx, q, spec, pitch, offset, (n, L, pitch, offset, spec))


@pytest.mark.parametrize("spec", ["thr:20:6:37", "thr:1:0:93"])
def test_thr_and_a_general_map(ctx, spec):
    from minicom_amd.hip import QualLossySpec
    q = _matrix(5, 300, 37)
    _check(ctx, q, spec, 37, 1, spec)
    floor16 = (np.arange(256) // 16 * 16).astype(np.uint8)
    out, rep = ctx.qual_transform(__import__("torch").from_numpy(q).cuda(), QualLossySpec.from_lut(floor16))
    want = LR.transform(q, ("lut", floor16))
    assert np.array_equal(out.cpu().numpy(), want[0]) and rep == want[1]


@pytest.mark.parametrize("P", [1, 2, 4, 47])
def test_pblock_rows_at_the_edges_of_a_tile(ctx, P):
    """the rows whose answer the text states, as the first and as the last row of a tile (and of the matrix)"""
    R = _tile_rows()
    for L in (37, 256):
        special = LR.pblock_rows(P, L)
        for name in sorted(special):
            q = qc.synth_quals(60 + P, 2 * R, L).copy()
            for at in (0, R - 1, R, 2 * R - 1):
                q[at] = special[name]
            _check(ctx, q, "pblock:%d" % P, L, 1, (name, P, L))
    for name, q in qc.degenerate():
        _check(ctx, np.array(q), "pblock:%d" % P, q.shape[1], 0, (name, P))


def test_a_refused_spec_touches_nothing(ctx):
    import minicom_amd
    from minicom_amd.hip import QualLossyReport, QualLossySpec
    q = _matrix(9, 200, 37)
    plus_one = QualLossySpec.from_lut(((np.arange(256) + 1) % 256).astype(np.uint8))
    thr = QualLossySpec(); thr.kind = QualLossySpec.THR; thr.p[0], thr.p[1], thr.p[2] = 20, 20, 37
    p0 = QualLossySpec(); p0.kind = QualLossySpec.PBLOCK; p0.p[0] = 0
    p48 = QualLossySpec(); p48.kind = QualLossySpec.PBLOCK; p48.p[0] = 48
    none = QualLossySpec()
    for s in (plus_one, thr, p0, p48, none):
        buf, view = _on_device(q, 38, 1)
        before = buf.cpu().numpy().copy()
        rep = QualLossyReport(11, 12, 13, 14)
        rc = ctx.lib.mcom_qual_transform(ctx._h, view.data_ptr(), 200, 37, 38, C.byref(s), C.byref(rep))
        assert rc == -1                                                                    # MCOM_E_ARG
        assert np.array_equal(buf.cpu().numpy(), before)
        assert rep.as_dict() == {"changed": 11, "sum_abs": 12, "sum_sq": 13, "max_abs": 14}
        with pytest.raises(minicom_amd.McomError):
            ctx.qual_transform(view, s, in_place=True)


def test_report_over_many_workgroups(ctx):
    """40 tiles and a few rows; the byte maps against numpy's own indexing, the P-block against the reference"""
    import torch
    R = _tile_rows()
    q = qc.synth_quals(7, 40 * R + 5, 100)
    d = torch.from_numpy(q).cuda()
    for spec in ("ill8", "thr:20:6:37", "pblock:2", "pblock:4"):
        out, rep = ctx.qual_transform(d, spec)
        want, wrep = LR.transform(q, spec)
        assert np.array_equal(out.cpu().numpy(), want)
        diff = np.abs(q.astype(np.int64) - want.astype(np.int64))
        assert rep == wrep == {"changed": int((diff != 0).sum()), "sum_abs": int(diff.sum()), "sum_sq": int((diff ** 2).sum()), "max_abs": int(diff.max())}
        assert rep["changed"] > 1000
    assert np.array_equal(d.cpu().numpy(), q)                                              # without in_place the input stays
    from minicom_amd import pipeline
    got = pipeline.qual_transform(q, "pblock:2", device=0)
    assert np.array_equal(got[0], LR.transform(q, "pblock:2")[0])


def test_mcomz_gpu_route_writes_the_host_member(tmp_path):
    """mcomz e --fastq-qual L --lossy SPEC --gpu: the member of the host route, with and without --order; e --qual likewise"""
    reads, quals, text = qc.tricky_fastq()
    (tmp_path / "t.fastq").write_bytes(text)
    (tmp_path / "q.raw").write_bytes(quals.tobytes())
    order = np.random.default_rng(3).permutation(120).astype("<u4")
    (tmp_path / "order.bin").write_bytes(order.tobytes())
    from minicom_amd import pipeline
    for spec in ("ill8", "pblock:2"):
        for extra, rows in (([], quals), (["--order", "order.bin"], quals[order])):
            want, rep = LR.transform(rows, spec)
            line = "lossy %s: changed %d sum_abs %d sum_sq %d max_abs %d\n" % (spec, rep["changed"], rep["sum_abs"], rep["sum_sq"], rep["max_abs"])
            out = {}
            for tag, gpu in (("host", []), ("gpu", ["--gpu"])):
                p = subprocess.run([MCOMZ, "e", "--fastq-qual", "37"] + extra + ["--lossy", spec] + gpu + ["t.fastq", tag + ".mcq"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
                assert p.returncode == 0 and p.stdout.split() == ["120"] and p.stderr == line, (tag, p.stderr)
                out[tag] = (tmp_path / (tag + ".mcq")).read_bytes()
            assert out["gpu"] == out["host"] == pipeline.qual_encode(want), (spec, extra)
        p = subprocess.run([MCOMZ, "e", "--qual", "37", "--lossy", spec, "--gpu", "q.raw", "raw.mcq"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and (tmp_path / "raw.mcq").read_bytes() == pipeline.qual_encode(LR.transform(quals, spec)[0]), p.stderr
    (tmp_path / "bad.fastq").write_bytes(qc.bad_fastqs()["shifted"])
    p = subprocess.run([MCOMZ, "e", "--fastq-qual", "37", "--lossy", "ill8", "--gpu", "bad.fastq", "bad.mcq"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "record 18 " in p.stderr and not (tmp_path / "bad.mcq").exists(), p.stderr


# ---- end to end: one run per archive kind -------------------------------------------------------------------------------------------------
N_READS, L100 = 400, 100


def _minicom(args, cwd):
    p = subprocess.run(["bash", os.path.join(ROOT, "bin", "minicom")] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    return p.returncode, p.stdout.decode(errors="replace")


def _named_fastq(reads, quals, names, plus) -> bytes:
    return b"".join(b"@" + names[i] + b"\n" + reads[i].tobytes() + b"\n+" + plus[i] + b"\n" + quals[i].tobytes() + b"\n" for i in range(reads.shape[0]))


def _retar(src, dst, marker):
    """the archive with qual_lossy.txt dropped (marker None) or holding `marker`"""
    with tarfile.open(src) as t:
        items = [(m.name, t.extractfile(m).read()) for m in t.getmembers() if m.isfile()]
    assert any(os.path.basename(n) == "qual_lossy.txt" for n, _ in items)
    with tarfile.open(dst, "w", format=tarfile.GNU_FORMAT) as t:
        for name, data in items:
            if os.path.basename(name) == "qual_lossy.txt":
                if marker is None:
                    continue
                data = marker
            ti = tarfile.TarInfo(name); ti.size = len(data); ti.mode = 0o644
            t.addfile(ti, io.BytesIO(data))


def _marker_of(archive) -> bytes:
    with tarfile.open(archive) as t:
        for m in t.getmembers():
            if os.path.basename(m.name) == "qual_lossy.txt":
                return t.extractfile(m).read()
    return b""


@functools.lru_cache(maxsize=None)
def _inputs():
    from minicom_amd import synth
    reads = synth.synth_reads(1002, N_READS, L100)
    quals = qc.synth_quals(51, N_READS, L100)
    names = nc.illumina(5, N_READS)
    plus = nc.mixed_plus(names)
    return reads, quals, names, plus


ROUTES = {
    # name: (compress flags without -b, spec, archive, check arguments)
    "order": (["-r", "X.fastq", "-p", "-Q", "-N"], "ill8", "X_comp_order.minicom"),
    "reordered": (["-r", "X.fastq", "-q"], "pblock:2", "X_comp.minicom"),
    "pair": (["-1", "A_1.fastq", "-2", "A_2.fastq", "-p", "-Q"], "thr:20:6:37", "A_comp_pe_order.minicom"),
}


@pytest.fixture(scope="module", params=sorted(ROUTES))
def route(request, tmp_path_factory):
    """the inputs of a route, its archive made with -b SPEC -G, and in plain/ the archive made without -b"""
    name = request.param
    flags, spec, archive = ROUTES[name]
    d = tmp_path_factory.mktemp("lossy_" + name)
    reads, quals, names, plus = _inputs()
    half = N_READS // 2
    if name == "order":
        (d / "X.fastq").write_bytes(_named_fastq(reads, quals, names, plus))
    elif name == "reordered":
        (d / "X.fastq").write_bytes(qc.fastq_bytes(reads, quals))
    else:
        (d / "A_1.fastq").write_bytes(qc.fastq_bytes(reads[:half], quals[:half]))
        (d / "A_2.fastq").write_bytes(qc.fastq_bytes(reads[half:], quals[half:]))
    rc, out = _minicom(flags + ["-b", spec, "-G", "-t", "2"], d)
    assert rc == 0, out[-3000:]
    check = ["-c", "X.fastq"] if name != "pair" else ["-c", "A_1.fastq", "-C", "A_2.fastq"]
    return name, d, flags, spec, archive, check


def test_minicom_b_decodes_to_the_transformed_file(route):
    name, d, flags, spec, archive, check = route
    reads, quals, names, plus = _inputs()
    half = N_READS // 2
    want_q = LR.transform(quals, spec)[0]
    assert _marker_of(d / archive) == spec.encode() + b"\n"
    rc, out = _minicom(["-d", archive, "-G"], d)
    assert rc == 0 and ("the quality values of this archive are lossy: stored under %s\n" % spec) in out, out[-3000:]
    stem = archive[:-len(".minicom")]
    if name == "order":
        assert (d / (stem + "_dec.fastq")).read_bytes() == _named_fastq(reads, want_q, names, plus)      # byte for byte with -N
    elif name == "reordered":
        text = (d / (stem + "_dec.fastq")).read_bytes()
        ln = text.split(b"\n")
        got = sorted((ln[4 * j + 1], ln[4 * j + 3]) for j in range(N_READS))
        assert len(ln) == 4 * N_READS + 1 and got == sorted((reads[i].tobytes(), want_q[i].tobytes()) for i in range(N_READS))
    else:
        assert (d / (stem + "_dec_1.fastq")).read_bytes() == qc.fastq_bytes(reads[:half], want_q[:half])
        assert (d / (stem + "_dec_2.fastq")).read_bytes() == qc.fastq_bytes(reads[half:], want_q[half:])


def test_minicom_b_check_names_the_spec(route):
    name, d, flags, spec, archive, check = route
    rc, out = _minicom(["-d", archive] + check, d)
    assert rc == 0 and ("identical under %s" % spec) in out and "DIFFERENT" not in out, out[-3000:]


def test_minicom_b_check_without_the_marker_is_different(route):
    name, d, flags, spec, archive, check = route
    (d / "t").mkdir(exist_ok=True)
    _retar(d / archive, d / "t" / archive, None)
    rc, out = _minicom(["-d", "t/" + archive] + check, d)
    assert rc == 2 and "DIFFERENT" in out, out[-3000:]


def test_minicom_b_check_under_another_spec_is_different(route):
    name, d, flags, spec, archive, check = route
    (d / "t").mkdir(exist_ok=True)
    _retar(d / archive, d / "t" / archive, b"pblock:7\n")
    rc, out = _minicom(["-d", "t/" + archive] + check, d)
    assert rc == 2 and "DIFFERENT" in out, out[-3000:]


def test_minicom_b_check_with_garbage_in_the_marker_is_refused(route):
    name, d, flags, spec, archive, check = route
    (d / "t").mkdir(exist_ok=True)
    _retar(d / archive, d / "t" / archive, b"ill8 or so\n")
    rc, out = _minicom(["-d", "t/" + archive] + check, d)
    assert rc == 1 and "qual_lossy.txt" in out, out[-3000:]


@pytest.fixture(scope="module")
def plain(route):
    """the route's archive made without -b, in plain/"""
    name, d, flags, spec, archive, check = route
    (d / "plain").mkdir(exist_ok=True)
    for f in d.glob("*.fastq"):
        if "_dec" not in f.name:
            (d / "plain" / f.name).write_bytes(f.read_bytes())
    rc, out = _minicom(flags + ["-G", "-t", "2"], d / "plain")
    assert rc == 0, out[-3000:]
    return d / "plain"


def test_an_archive_without_b_verifies_as_before(route, plain):
    name, d, flags, spec, archive, check = route
    assert _marker_of(plain / archive) == b""
    rc, out = _minicom(["-d", archive] + check, plain)
    assert rc == 0 and "identical" in out and " under " not in out and "lossy" not in out, out[-3000:]


def test_minicom_b_without_quality_values_leaves_nothing(route):
    name, d, flags, spec, archive, check = route
    (d / "bare").mkdir(exist_ok=True)
    inputs = [f.name for f in d.glob("*.fastq") if "_dec" not in f.name]
    for f in inputs:
        (d / "bare" / f).write_bytes((d / f).read_bytes())
    bare = [a for a in flags if a not in ("-Q", "-q", "-N")]
    rc, out = _minicom(bare + ["-b", spec, "-G"], d / "bare")
    assert rc == 1 and "minicom: -b " in out, out[-3000:]
    assert sorted(os.listdir(d / "bare")) == sorted(inputs)


def test_container_routes(route, tmp_path):
    """container.compress_fastq / compress_fastq_pair with quality_lossy, unpack and verify_file on the same inputs"""
    from minicom_amd import McomError, container
    name, d, flags, spec, archive, check = route
    reads, quals, names, plus = _inputs()
    out = str(tmp_path / "py.minicom")
    if name == "order":
        container.compress_fastq(str(d / "X.fastq"), out, order=True, quality=True, names=True, codec="rans", device=0, threads=2, quality_lossy=spec)
        files = (str(d / "X.fastq"),)
    elif name == "reordered":
        container.compress_fastq(str(d / "X.fastq"), out, codec="rans", device=0, threads=2, quality_reordered=True, quality_lossy=spec)
        files = (str(d / "X.fastq"),)
    else:
        container.compress_fastq_pair(str(d / "A_1.fastq"), str(d / "A_2.fastq"), out, quality=True, codec="rans", device=0, threads=2, quality_lossy=spec)
        files = (str(d / "A_1.fastq"), str(d / "A_2.fastq"))
    kinds = container.unpack(out, str(tmp_path / "un"))
    assert kinds["quality_lossy"] == spec and (tmp_path / "un" / "qual_lossy.txt").read_bytes() == spec.encode() + b"\n"
    rep = container.verify_file(out, *files)
    assert rep["identical"] and rep["quality_lossy"] == spec
    # the members are those of the command line's archive
    with tarfile.open(out) as a, tarfile.open(d / archive) as b:
        for m in a.getmembers():
            if m.name.endswith(".mcq"):
                assert a.extractfile(m).read() == b.extractfile("./" + m.name).read(), m.name
    _retar(out, str(tmp_path / "no.minicom"), None)
    assert not container.verify_file(str(tmp_path / "no.minicom"), *files)["identical"]
    _retar(out, str(tmp_path / "bad.minicom"), b"garbage\n")
    with pytest.raises(McomError):
        container.verify_file(str(tmp_path / "bad.minicom"), *files)
    with pytest.raises(ValueError):
        container.compress_fastq(files[0], str(tmp_path / "x.minicom"), quality_lossy=spec)
    with pytest.raises(ValueError):
        container.compress_fastq(files[0], str(tmp_path / "x.minicom"), order=True, quality=True, quality_lossy="ill9")
    assert not (tmp_path / "x.minicom").exists()
