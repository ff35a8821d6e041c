"""BGZF output on the device (csrc/bgzf.hip): mcom_bgzf_encode writes the bytes of the host twin on every input
of tests/bgzf_cases.py at unaligned addresses, refuses a buffer one byte short, and what it writes comes back through the member-parallel
FASTQ ingest."""
import gzip

import numpy as np
import pytest
import torch

import bgzf_cases as BC
import minicom_amd
from minicom_amd import pipeline

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return minicom_amd.Context(0)


def _device_encode(ctx, data: bytes, in_off: int, out_off: int, eof: bool = True, short_by: int = 0):
    n = len(data)
    src = torch.zeros(n + 16, dtype=torch.uint8, device="cuda:0")
    if n:
        src[in_off:in_off + n] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    cap = BC.bound(n) - (0 if eof else 28)
    room = torch.full((cap + 16,), 0xAA, dtype=torch.uint8, device="cuda:0")
    got = ctx.bgzf_encode(src[in_off:in_off + n], eof=eof, out=room[out_off:out_off + cap - short_by])
    return bytes(got.cpu().numpy()), room


@pytest.mark.parametrize("name", sorted(BC.cases()))
def test_device_writes_the_twins_bytes_at_unaligned_addresses(ctx, name):
    data = BC.cases()[name]
    want = pipeline.bgzf_encode(data)
    for in_off, out_off in ((0, 0), (1, 3), (3, 1)):
        got, room = _device_encode(ctx, data, in_off, out_off)
        assert got == want, (name, in_off, out_off)
        edge = room.cpu().numpy()
        assert (edge[:out_off] == 0xAA).all() and (edge[out_off + len(want):] == 0xAA).all()          # nothing outside the member bytes
    assert gzip.decompress(want) == data


def test_a_piece_of_a_stream_has_no_last_member(ctx):
    data = BC.cases()["len130561"]
    got, _ = _device_encode(ctx, data, 1, 1, eof=False)
    assert got == pipeline.bgzf_encode(data, eof=False) and got + BC.EOF == pipeline.bgzf_encode(data)


@pytest.mark.parametrize("name", ["len0", "len1", "random", "fastq", "len130561"])
def test_room_one_byte_short_is_overflow(ctx, name):
    data = BC.cases()[name]
    exact = len(pipeline.bgzf_encode(data))
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda:0")
    assert len(ctx.bgzf_encode(src, out=torch.empty(exact, dtype=torch.uint8, device="cuda:0"))) == exact
    with pytest.raises(minicom_amd.McomError):
        ctx.bgzf_encode(src, out=torch.empty(exact - 1, dtype=torch.uint8, device="cuda:0"))


def test_pipeline_route_and_file_form(ctx, tmp_path):
    data = BC.cases()["fastq"]
    want = pipeline.bgzf_encode(data)
    assert pipeline.bgzf_encode(data, device=0) == want
    (tmp_path / "a.fastq").write_bytes(data)
    pipeline.bgzf_file(str(tmp_path / "a.fastq"), str(tmp_path / "a.fastq.gz"), device=0)
    assert (tmp_path / "a.fastq.gz").read_bytes() == want


# ---- the decoders' tails with a `.gz` path ------------------------------------------------------------------------------------------
N_REC, L_REC = 2000, 100


def _set_piece(nbytes: int):
    import ctypes as C
    lib = pipeline.load_host_library()
    lib.mcomh_test_decoder_piece_bytes.restype = C.c_int; lib.mcomh_test_decoder_piece_bytes.argtypes = [C.c_size_t]
    assert lib.mcomh_test_decoder_piece_bytes(nbytes) == 0


@pytest.fixture(scope="module")
def archives(tmp_path_factory):
    """one archive per decoder tail, made once from two small FASTQ files: name -> (archive, number of output files)"""
    from minicom_amd import container
    d = tmp_path_factory.mktemp("bgzf_archives")
    f1, f2 = str(d / "a_1.fastq"), str(d / "a_2.fastq")
    open(f1, "wb").write(BC.synthetic_fastq(41, N_REC, L_REC)); open(f2, "wb").write(BC.synthetic_fastq(42, N_REC, L_REC))
    made = {}
    for name, kw, two in (("default", {}, False), ("order", {"order": True}, False), ("paired", {"path2": f2}, True),
                          ("fastq", {"order": True, "quality": True}, False), ("fastq_names", {"order": True, "quality": True, "names": True}, False),
                          ("fastq_reordered", {"quality_reordered": True}, False)):
        container.compress_fastq(f1, str(d / (name + ".minicom")), **kw)
        made[name] = (str(d / (name + ".minicom")), 2 if two else 1)
    container.compress_fastq_pair(f1, f2, str(d / "fastq_order_pe.minicom"), quality=True, names=True)
    made["fastq_order_pe"] = (str(d / "fastq_order_pe.minicom"), 2)
    return made


@pytest.mark.parametrize("name", ["default", "order", "paired", "fastq", "fastq_names", "fastq_reordered", "fastq_order_pe"])
def test_decoder_tails_write_the_twins_file(archives, tmp_path, name):
    """every tail with a `.gz` path, at the default piece size, at three blocks and at an odd size: the file is the twin's coding of the
    plain output of the same call byte for byte, so block k holds the bytes [65280 k, ...) whatever the piece size"""
    from minicom_amd import container
    arch, n_files = archives[name]
    plain = [str(tmp_path / ("plain_%d" % k)) for k in range(n_files)]
    n = container.decompress_file(arch, plain[0], plain[1] if n_files == 2 else None, device=0)
    want = [pipeline.bgzf_encode(open(p, "rb").read()) for p in plain]
    assert n == N_REC and all(len(open(p, "rb").read()) > 3 * BC.BLOCK for p in plain)
    try:
        for piece in (0, 3 * BC.BLOCK, 100003):
            _set_piece(piece)
            outs = [str(tmp_path / ("out_%d_%d.gz" % (piece, k))) for k in range(n_files)]
            assert container.decompress_file(arch, outs[0], outs[1] if n_files == 2 else None, device=0, gzip=True) == n
            for o, w in zip(outs, want):
                assert open(o, "rb").read() == w, (name, piece)
    finally:
        _set_piece(0)
    assert gzip.decompress(want[0]) == open(plain[0], "rb").read()


@pytest.mark.parametrize("fixture,mode", [("streams_stages_L100", "default"), ("streams_order_stages_L100", "order"), ("streams_pe_stages_L150", "pe")])
def test_decoder_tails_on_the_golden_stream_files(golden_dir, tmp_path, fixture, mode):
    """the three read tails on the stream folders kept under tests/golden (the FASTQ tails have no fixture: their archives are made above),
    at an odd piece size: the `.gz` file is the twin's coding of the plain output of the same call"""
    import io
    import os
    import tarfile
    d = tmp_path / "streams"; d.mkdir()
    with gzip.open(os.path.join(golden_dir, fixture + ".tar.gz"), "rb") as g:
        tarfile.open(fileobj=io.BytesIO(g.read())).extractall(str(d))

    def run(tag):
        outs = [str(tmp_path / ("%d_%s" % (k, tag))) for k in range(2 if mode == "pe" else 1)]
        n = pipeline.decompress_pe(str(d), outs[0], outs[1], device=0) if mode == "pe" else pipeline.decompress(str(d), outs[0], order=mode == "order", device=0)
        assert n > 0
        return [open(o, "rb").read() for o in outs]
    plain = run("plain")
    try:
        _set_piece(100003)
        packed = run("packed.gz")
    finally:
        _set_piece(0)
    assert all(len(p) > BC.BLOCK for p in plain) and packed == [pipeline.bgzf_encode(p) for p in plain]


def test_a_refused_archive_leaves_no_gz(golden_dir, tmp_path):
    import io
    import os
    import tarfile
    d = tmp_path / "streams"; d.mkdir()
    with gzip.open(os.path.join(golden_dir, "streams_stages_L100.tar.gz"), "rb") as g:
        tarfile.open(fileobj=io.BytesIO(g.read())).extractall(str(d))
    good = str(tmp_path / "good.reads.gz")
    assert pipeline.decompress(str(d), good, device=0) > 0 and len(gzip.decompress(open(good, "rb").read())) > 0
    ref = d / "ref.bin.0"
    ref.write_bytes(ref.read_bytes()[: ref.stat().st_size // 2])
    with pytest.raises(minicom_amd.McomError):
        pipeline.decompress(str(d), str(tmp_path / "bad.reads.gz"), device=0)
    assert not (tmp_path / "bad.reads.gz").exists()


def test_decoded_fastq_gz_feeds_the_pipeline(archives, tmp_path):
    """the round trip through the BGZF ingest: Pipeline.from_fastq of X_dec.fastq.gz is the pipeline of the plain file"""
    from minicom_amd import container
    from minicom_amd.pipeline import Pipeline
    container.decompress_file(archives["fastq_names"][0], str(tmp_path / "x_dec.fastq"), device=0)
    container.decompress_file(archives["fastq_names"][0], str(tmp_path / "x_dec.fastq.gz"), device=0)           # the suffix decides
    assert gzip.decompress((tmp_path / "x_dec.fastq.gz").read_bytes()) == (tmp_path / "x_dec.fastq").read_bytes()
    p = Pipeline.from_fastq(str(tmp_path / "x_dec.fastq.gz"), host_threads=4); q = Pipeline.from_fastq(str(tmp_path / "x_dec.fastq"), host_threads=4)
    assert (p.n, p.L) == (q.n, q.L) == (N_REC, L_REC)
    p.pre_process(); q.pre_process()
    assert p.result_digest() == q.result_digest()
    p.close(); q.close()


def test_members_come_back_through_the_parallel_ingest(ctx, tmp_path):
    """a FASTQ file written by the device encoder is read by the member-parallel route (it finds the BC fields) with the plain file's rows"""
    import ctypes as C
    data = BC.synthetic_fastq(33, 3000)
    assert len(data) > 4 * BC.BLOCK
    (tmp_path / "r.fastq").write_bytes(data)
    pipeline.bgzf_file(str(tmp_path / "r.fastq"), str(tmp_path / "r.fastq.gz"), device=0)
    plain = pipeline.read_fastq(str(tmp_path / "r.fastq"))
    packed = pipeline.read_fastq(str(tmp_path / "r.fastq.gz"))
    lib = pipeline.load_host_library(); lib.mcomh_test_gz_items.restype = C.c_long
    assert lib.mcomh_test_gz_items() > 0                                                      # the parallel route, not the sequential reader
    assert np.array_equal(plain, packed) and plain.shape == (3000, 100)
