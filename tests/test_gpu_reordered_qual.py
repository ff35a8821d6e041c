"""Quality values in an archive's own order on the GPU (`minicom -q`): the row gather of csrc/qual.hip against numpy
with its two validity flags, the read order of csrc/streams.hip against the host decoders' rows, the multiset comparison over records of
several parts, and the command line end to end for one file and for a pair."""
import os
import subprocess

import numpy as np
import pytest

import qual_cases as qc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5
L100 = 100


@pytest.fixture(scope="module")
def ctx():
    import minicom_amd
    return minicom_amd.Context(0)


# ---- mcom_qual_gather_rows -------------------------------------------------------------------------------------------------------------
def _pitched(q, pitch, offset, fill=CANARY):
    """(buffer, view): the matrix on the device with rows `pitch` apart, the first one `offset` bytes into a buffer of canary bytes"""
    import torch
    n, L = q.shape
    buf = torch.full((offset + max(n, 1) * pitch + 64,), fill, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + max(n, 1) * pitch].view(max(n, 1), pitch)[:n, :L]
    if n:
        view.copy_(torch.from_numpy(np.array(q, dtype=np.uint8)).cuda())
    return buf, view


def _image(buf, n, L, pitch, offset):
    """(the rows, everything else) of an output buffer as numpy"""
    h = buf.cpu().numpy()
    mask = np.zeros(h.shape[0], dtype=bool)
    for i in range(n):
        mask[offset + i * pitch:offset + i * pitch + L] = True
    return h[mask].reshape(n, L), h[~mask]


@pytest.mark.parametrize("L", [1, 15, 16, 17, 100, 256])
@pytest.mark.parametrize("n", [0, 1, 17])
def test_gather_is_numpy_fancy_indexing(ctx, n, L):
    """every shape of the host test, at pitch L and L + 1 on either side and at odd base addresses; the bytes around the output rows stay"""
    import torch
    rng = np.random.default_rng(1000 * n + L)
    rows = rng.integers(33, 127, (n, L), dtype=np.uint8)
    order = rng.permutation(n).astype(np.int32)
    d_order = torch.from_numpy(order).cuda()
    for pitch_in, off_in, pitch_out, off_out in ((L, 0, L, 0), (L + 1, 1, L, 3), (L, 5, L + 1, 1), (L + 1, 7, L + 1, 13), (L + 19, 2, L + 16, 16)):
        _, src = _pitched(rows, pitch_in, off_in, fill=0xEE)
        buf, dst = _pitched(np.zeros((n, L), dtype=np.uint8), pitch_out, off_out)
        if n:
            dst.fill_(CANARY)
        out, flags = ctx.qual_gather_rows(src, d_order, out=dst)
        got, rest = _image(buf, n, L, pitch_out, off_out)
        assert flags == 0 and np.array_equal(got, rows[order]), (pitch_in, off_in, pitch_out, off_out)
        assert (rest == CANARY).all(), (pitch_in, off_in, pitch_out, off_out)
    out, flags = ctx.qual_gather_rows(torch.from_numpy(rows).cuda(), d_order)
    assert flags == 0 and np.array_equal(out.cpu().numpy(), rows[order])


def test_gather_of_many_rows_and_a_subset(ctx):
    """more than one workgroup; fewer output rows than source rows; the GPU route of pipeline.qual_gather"""
    import torch
    from minicom_amd import pipeline
    rng = np.random.default_rng(5)
    n, L = 5000, 151
    rows = rng.integers(33, 127, (n, L), dtype=np.uint8)
    order = rng.permutation(n).astype(np.int32)
    d_rows = torch.from_numpy(rows).cuda()
    out, flags = ctx.qual_gather_rows(d_rows, torch.from_numpy(order).cuda())
    assert flags == 0 and np.array_equal(out.cpu().numpy(), rows[order])
    out, flags = ctx.qual_gather_rows(d_rows, torch.from_numpy(order[:777].copy()).cuda())
    assert flags == 0 and np.array_equal(out.cpu().numpy(), rows[order[:777]])
    assert np.array_equal(pipeline.qual_gather(rows, order, device=0), rows[order])
    assert np.array_equal(pipeline.qual_gather(rows, order, device=0), pipeline.qual_gather(rows, order))


def test_gather_flags_a_bad_order_and_still_copies_the_good_rows(ctx):
    import torch
    from minicom_amd import McomError, pipeline
    rng = np.random.default_rng(6)
    n, L = 100, 37
    rows = rng.integers(33, 127, (n, L), dtype=np.uint8)
    good = rng.permutation(n).astype(np.int64)
    dup = good.copy(); dup[40] = dup[77]
    beyond = good.copy(); beyond[[3, 99]] = [n, 2 ** 32 - 1]
    both = dup.copy(); both[0] = n + 5
    _, src = _pitched(rows, L, 1)
    for order, want, skipped in ((dup, ctx.GATHER_F_DUP, []), (beyond, ctx.GATHER_F_BOUNDS, [3, 99]), (both, ctx.GATHER_F_DUP | ctx.GATHER_F_BOUNDS, [0])):
        buf, dst = _pitched(np.zeros((n, L), dtype=np.uint8), L + 3, 5)
        dst.fill_(CANARY)
        out, flags = ctx.qual_gather_rows(src, torch.from_numpy(order.astype(np.uint32).view(np.int32)).cuda(), out=dst)
        got, rest = _image(buf, n, L, L + 3, 5)
        keep = np.ones(n, dtype=bool); keep[skipped] = False
        assert flags == want
        assert np.array_equal(got[keep], rows[order[keep]]) and (got[~keep] == CANARY).all() and (rest == CANARY).all()
        with pytest.raises(McomError):
            pipeline.qual_gather(rows, order.astype(np.uint32), device=0)
    # an empty source table: every index is beyond it
    out, flags = ctx.qual_gather_rows(torch.empty((0, L), dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"))
    assert flags == ctx.GATHER_F_BOUNDS


# ---- mcom_dump_read_order ----------------------------------------------------------------------------------------------------------------
def _special_reads():
    """3000 synthetic reads of 100 bases and, spread among them, the kinds that go into the decoder's lists: (reads, {kind: row numbers})"""
    from minicom_amd import synth
    rng = np.random.default_rng(77)
    base = synth.synth_reads(1002, 3000, L100)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    extra, kind = [], []
    for _ in range(3):
        extra.append(np.full(L100, ord("A"), dtype=np.uint8)); kind.append("allA")
    for _ in range(2):
        extra.append(np.full(L100, ord("T"), dtype=np.uint8)); kind.append("allT")
    for q in range(2):
        r = np.full(L100, ord("A"), dtype=np.uint8); r[[11 + q, 70]] = [ord("C"), ord("G")]
        extra.append(r); kind.append("nearA")
    for q in range(3):
        r = acgt[rng.integers(0, 4, L100)].copy(); r[20 + 7 * q] = ord("N")                # random sequence: nothing to cluster with
        extra.append(r); kind.append("N")
    dup_of = rng.choice(3000, 20, replace=False)
    for s in dup_of:
        extra.append(base[s].copy()); kind.append("dup")
    reads = np.concatenate([base, np.array(extra)])
    perm = rng.permutation(reads.shape[0])                                                 # the added reads are not the last ones of a file
    reads = np.ascontiguousarray(reads[perm])
    where = {}
    inv = np.argsort(perm)
    for q, k in enumerate(kind):
        where.setdefault(k, []).append(int(inv[3000 + q]))
    where["dup_of"] = [int(inv[s]) for s in dup_of]
    return reads, where


@pytest.fixture(scope="module")
def special():
    return _special_reads()


def _lines(path):
    return path.read_bytes().split(b"\n")[:-1]


def _dump_with_order(reads, d, paired, stream_sets=1, host_dump=0):
    from minicom_amd.pipeline import Pipeline
    d.mkdir()
    p = Pipeline(reads, host_threads=4, stream_sets=stream_sets, host_dump=host_dump)
    try:
        p.pre_process()
        p.keep_read_order(True)
        p.cluster_dump(str(d), paired=paired)
    finally:
        p.close()
    raw = (d / "read_order.bin").read_bytes()
    assert len(raw) % 4 == 0
    return np.frombuffer(raw, dtype="<u4").astype(np.int64)


@pytest.mark.parametrize("stream_sets", [1, 3])
@pytest.mark.parametrize("paired", [False, True])
def test_read_order_names_the_read_of_every_decoded_row(special, tmp_path, paired, stream_sets):
    """row j of the HOST decoder's output is input read order[j] (paired end: of both files); the order is a permutation; every added kind of
    read lies in the list it was made for"""
    from minicom_amd import pipeline
    reads, where = special
    n = reads.shape[0]
    half = n // 2
    d = tmp_path / "dump"
    order = _dump_with_order(reads, d, paired, stream_sets=stream_sets)
    rows = half if paired else n
    assert order.shape[0] == rows and np.array_equal(np.sort(order), np.arange(rows))
    info = (d / "info.txt").read_text().split()
    assert int(info[1]) == stream_sets
    n_all = [int(v) for v in (info[3:6] if paired else info[2:5])]
    assert n_all == [3, 2, 0]
    near, with_n = _lines(d / "AA.txt"), _lines(d / "single_N.seq")
    assert len(near) == 2 and sorted(with_n) == sorted(reads[i].tobytes() for i in where["N"])
    assert len(_lines(d / "TT.txt")) == 0 and len(_lines(d / "NN.txt")) == 0
    n_single = (d / "single.seq").stat().st_size * 4 // L100
    n_lists = 3 + 2 + 2 + 3 + n_single
    members = sum(len(_lines(d / ("dif_char.txt.%d" % t))) for t in range(stream_sets))
    assert n_lists + members == n
    assert any(any((d / ("dir.bin.%d" % t)).read_bytes()) for t in range(stream_sets))    # at least one reverse-complemented member
    if not paired:
        # where the kinds land in the decoder's sequence
        assert sorted(order[:3]) == sorted(where["allA"]) and sorted(order[3:5]) == sorted(where["allT"])
        assert sorted(order[5:7]) == sorted(where["nearA"]) and sorted(order[7:10]) == sorted(where["N"])
        place = np.argsort(order)
        for a, b in zip(where["dup"], where["dup_of"]):                                    # exact duplicates of clustered reads are members, both of them
            assert place[a] >= n_lists and place[b] >= n_lists, (a, b)
        assert pipeline.decompress(str(d), str(tmp_path / "rows.txt")) == n
        got = np.frombuffer(b"".join(_lines(tmp_path / "rows.txt")), dtype=np.uint8).reshape(n, L100)
        assert np.array_equal(got, reads[order])
    else:
        first = [i for k in ("allA", "allT", "nearA", "N") for i in where[k] if i < half]
        assert set(first) <= set(order[:len(first) + n_single].tolist())
        assert pipeline.decompress_pe(str(d), str(tmp_path / "r1.txt"), str(tmp_path / "r2.txt")) == half
        r1 = np.frombuffer(b"".join(_lines(tmp_path / "r1.txt")), dtype=np.uint8).reshape(half, L100)
        r2 = np.frombuffer(b"".join(_lines(tmp_path / "r2.txt")), dtype=np.uint8).reshape(half, L100)
        assert np.array_equal(r1, reads[order]) and np.array_equal(r2, reads[half + order])


@pytest.mark.parametrize("paired", [False, True])
def test_the_host_dump_route_writes_the_same_read_order(special, tmp_path, paired):
    reads, _ = special
    dev = _dump_with_order(reads, tmp_path / "dev", paired)
    host = _dump_with_order(reads, tmp_path / "host", paired, host_dump=1)
    assert (tmp_path / "dev" / "read_order.bin").read_bytes() == (tmp_path / "host" / "read_order.bin").read_bytes() and np.array_equal(dev, host)


def test_the_order_preserving_dump_refuses_the_flag_and_the_flag_can_be_dropped(special, tmp_path):
    from minicom_amd import McomError
    from minicom_amd.pipeline import Pipeline
    reads, _ = special
    p = Pipeline(reads[:600], host_threads=2)
    try:
        p.pre_process()
        p.keep_read_order(True)
        (tmp_path / "o").mkdir()
        with pytest.raises(McomError):
            p.cluster_dump(str(tmp_path / "o"), order=True)
        p.keep_read_order(False)
        p.cluster_dump(str(tmp_path / "o"), order=True)
        assert not (tmp_path / "o" / "read_order.bin").exists()
    finally:
        p.close()


def test_dump_read_order_on_crafted_lists(ctx):
    """mcom_dump_read_order itself: the lists, then the members' read ids; paired end: the first-file entries in their order"""
    import torch
    lists = np.array([9, 2, 7, 4], dtype=np.int32)
    rid = np.array([1, 8, 0, 5, 3, 6], dtype=np.int64)
    mem = (rid << 32) | np.array([5, 12, 7, 1, 0, 3], dtype=np.int64)                       # (position and direction bits below the id)
    d_l, d_m = torch.from_numpy(lists).cuda(), torch.from_numpy(mem).cuda()
    assert ctx.dump_read_order(d_l, d_m).cpu().tolist() == [9, 2, 7, 4, 1, 8, 0, 5, 3, 6]
    assert ctx.dump_read_order(d_l, d_m, half=5).cpu().tolist() == [2, 4, 1, 0, 3]
    assert ctx.dump_read_order(d_l[:0], d_m).cpu().tolist() == rid.tolist()
    assert ctx.dump_read_order(d_l, d_m[:0]).cpu().tolist() == lists.tolist()
    assert ctx.dump_read_order(d_l, d_m, half=3).cpu().tolist() == [2, 1, 0]               # (more first-file reads than half would be cut, fewer are reported)
    assert ctx.dump_read_order(d_l, d_m, half=8).cpu().tolist() == [2, 7, 4, 1, 0, 5, 3, 6]


# ---- mcom_verify_multiset_parts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_parts", [2, 4])
@pytest.mark.parametrize("n", [0, 1, 1000])
def test_verify_multiset_parts(ctx, n, n_parts):
    """side b holds the records of side a in another order, at another pitch and other addresses; one other byte in the last column of the
    last part is one record missing and one extra, and both are named"""
    L = 75
    rng = np.random.default_rng(10 * n + n_parts)
    parts = [rng.integers(33, 127, (n, L), dtype=np.uint8) for _ in range(n_parts)]
    if n > 10:
        for p in parts[:-1]:
            p[5] = p[3]                                                                    # two records that differ in their last part only
        parts[0][8] = parts[0][2]; parts[-1][8] = parts[-1][2]                             # ... and two that differ in a middle part only (2 parts: not at all)
    perm = rng.permutation(n)
    a = [_pitched(p, L, 1 + q)[1] for q, p in enumerate(parts)]
    b = [_pitched(p[perm], L + 1, 3 * q)[1] for q, p in enumerate(parts)]
    flat = lambda views, pitch: [v.as_strided((max((n - 1) * pitch + L, 0),), (1,)) if n else None for v in views]
    rep = ctx.verify_multiset_parts((flat(a, L), L, n), (flat(b, L + 1), L + 1, n), L)
    assert rep["identical"] and rep["missing"] == rep["extra"] == 0 and rep["n_a"] == rep["n_b"] == n
    if not n:
        return
    k = int(np.nonzero(perm > 10)[0][0]) if n > 10 else 0                                 # (not one of the records made alike above)
    other = parts[-1][perm].copy()
    other[k, L - 1] = 33 if other[k, L - 1] != 33 else 34
    b[-1] = _pitched(other, L + 1, 2)[1]
    rep = ctx.verify_multiset_parts((flat(a, L), L, n), (flat(b, L + 1), L + 1, n), L)
    assert not rep["identical"] and rep["missing"] == rep["extra"] == 1
    assert rep["missing_examples"] == [int(perm[k])] and rep["extra_examples"] == [k]
    # one part more on one side is an error, not a verdict
    from minicom_amd import McomError
    with pytest.raises(McomError):
        ctx.verify_multiset_parts((flat(a, L)[:-1], L, n), (flat(b, L + 1), L + 1, n), L)


def test_verify_multiset_parts_settles_hash_collisions_in_full(ctx):
    """with two hash bits nearly every run of equal hashes holds unequal records: the verdict is still exact, over all parts"""
    L, n = 40, 300
    rng = np.random.default_rng(4)
    parts = [rng.integers(33, 127, (n, L), dtype=np.uint8) for _ in range(4)]
    perm = rng.permutation(n)
    a = [_pitched(p, L, 0)[1].as_strided(((n - 1) * L + L,), (1,)) for p in parts]
    other = [p[perm].copy() for p in parts]
    other[2][17, 0] ^= 1
    b = [_pitched(p, L + 1, 1)[1].as_strided(((n - 1) * (L + 1) + L,), (1,)) for p in other]
    ctx.set_verify_hash_bits(2)
    try:
        rep = ctx.verify_multiset_parts((a, L, n), (b, L + 1, n), L)
    finally:
        ctx.set_verify_hash_bits(64)
    assert rep["missing"] == rep["extra"] == 1 and rep["missing_examples"] == [int(perm[17])] and rep["extra_examples"] == [17] and rep["exact_runs"] > 0


# ---- `minicom -q` end to end ---------------------------------------------------------------------------------------------------------------
def _minicom(args, cwd):
    p = subprocess.run(["bash", os.path.join(ROOT, "bin", "minicom")] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    return p.returncode, p.stdout.decode(errors="replace")


def _numbered_quals(seed, n, L):
    """quality lines that spell their record number in their first three columns (base 90): two records of one sequence still differ"""
    q = qc.synth_quals(seed, n, L).copy()
    i = np.arange(n)
    for c in range(3):
        q[:, c] = 33 + (i // 90 ** c) % 90
    return q


def _records(text: bytes):
    ln = text.split(b"\n")
    assert ln[-1] == b"" and (len(ln) - 1) % 4 == 0
    n = (len(ln) - 1) // 4
    assert all(ln[4 * j] == b"@%d" % (j + 1) and ln[4 * j + 2] == b"+" for j in range(n))
    return [(ln[4 * j + 1], ln[4 * j + 3]) for j in range(n)]


def _members(archive):
    import tarfile
    with tarfile.open(archive) as t:
        return [os.path.basename(m.name) for m in t.getmembers() if m.isfile()]


@pytest.fixture(scope="module")
def single_q(special, tmp_path_factory):
    d = tmp_path_factory.mktemp("q_single")
    reads, where = special
    quals = _numbered_quals(41, reads.shape[0], L100)
    (d / "X.fastq").write_bytes(qc.fastq_bytes(reads, quals))
    rc, out = _minicom(["-r", "X.fastq", "-q", "-G", "-t", "2"], d)
    assert rc == 0, out[-3000:]
    return d, reads, quals, where


def test_minicom_q_single_file(single_q):
    d, reads, quals, _ = single_q
    names = _members(d / "X_comp.minicom")
    assert "rqual.mcq" in names and "read_order.bin" not in names and not any(n.startswith("idsbin") for n in names)
    assert not list(d.glob("*.order")) and not (d / "X_comp").exists()
    rc, out = _minicom(["-d", "X_comp.minicom", "-G"], d)
    assert rc == 0, out[-3000:]
    gpu = (d / "X_comp_dec.fastq").read_bytes()
    (d / "X_comp_dec.fastq").unlink()
    rc, out = _minicom(["-d", "X_comp.minicom"], d)
    assert rc == 0, out[-3000:]
    assert (d / "X_comp_dec.fastq").read_bytes() == gpu                                    # host and GPU routes: the same bytes
    want = sorted((reads[i].tobytes(), quals[i].tobytes()) for i in range(reads.shape[0]))
    assert sorted(_records(gpu)) == want                                                   # every read with its own quality line, duplicates counted


def test_minicom_q_single_file_check(single_q, tmp_path):
    d, reads, quals, where = single_q
    (tmp_path / "X_comp.minicom").write_bytes((d / "X_comp.minicom").read_bytes())
    rc, out = _minicom(["-d", "X_comp.minicom", "-c", str(d / "X.fastq")], tmp_path)
    assert rc == 0 and "identical" in out, out[-3000:]
    # the quality lines of two reads of different sequence swapped
    q2 = quals.copy(); q2[[10, 2000]] = q2[[2000, 10]]
    assert not np.array_equal(reads[10], reads[2000])
    (tmp_path / "swapped.fastq").write_bytes(qc.fastq_bytes(reads, q2))
    rc, out = _minicom(["-d", "X_comp.minicom", "-c", "swapped.fastq"], tmp_path)
    assert rc == 2 and "DIFFERENT" in out, out[-3000:]
    # one byte of the quality lines of two exact duplicates: the reads alone would still be the same multiset
    a, b = where["dup"][0], where["dup_of"][0]
    assert np.array_equal(reads[a], reads[b])
    q3 = quals.copy()
    for i in (a, b):
        q3[i, 50] = 33 if q3[i, 50] != 33 else 34
    (tmp_path / "dup.fastq").write_bytes(qc.fastq_bytes(reads, q3))
    rc, out = _minicom(["-d", "X_comp.minicom", "-c", "dup.fastq"], tmp_path)
    assert rc == 2 and "2 records of the FASTQ are missing" in out, out[-3000:]
    assert sorted(os.listdir(tmp_path)) == ["X_comp.minicom", "dup.fastq", "swapped.fastq"]        # -c leaves nothing behind


PAIR_DUPS = ((100, 900), (200, 1200), (100, 1300))           # (pair i, pair j) among the pairs that hold no read of a list: pair j becomes a copy of pair i


@pytest.fixture(scope="module")
def paired_q(special, tmp_path_factory):
    d = tmp_path_factory.mktemp("q_paired")
    reads, where = special
    reads = reads.copy()
    half = reads.shape[0] // 2
    special_rows = {i % half for k in ("allA", "allT", "nearA", "N") for i in where[k]}
    plain = [i for i in range(half) if i not in special_rows]
    for i, j in PAIR_DUPS:                                                                 # exact duplicate PAIRS: both mates of pair j are those of pair i
        i, j = plain[i], plain[j]
        reads[j] = reads[i]; reads[half + j] = reads[half + i]
    quals = _numbered_quals(43, reads.shape[0], L100)
    (d / "A_1.fastq").write_bytes(qc.fastq_bytes(reads[:half], quals[:half]))
    (d / "A_2.fastq").write_bytes(qc.fastq_bytes(reads[half:], quals[half:]))
    rc, out = _minicom(["-1", "A_1.fastq", "-2", "A_2.fastq", "-q", "-G", "-t", "2"], d)
    assert rc == 0, out[-3000:]
    return d, reads, quals, half, [(plain[i], plain[j]) for i, j in PAIR_DUPS]


def test_minicom_q_paired_files(paired_q):
    d, reads, quals, half, _ = paired_q
    names = _members(d / "A_comp_pe.minicom")
    assert "rqual_1.mcq" in names and "rqual_2.mcq" in names and "read_order.bin" not in names
    assert not list(d.glob("*.order")) and not (d / "A_comp_pe").exists()
    rc, out = _minicom(["-d", "A_comp_pe.minicom", "-G"], d)
    assert rc == 0, out[-3000:]
    gpu = [(d / ("A_comp_pe_dec_%d.fastq" % k)).read_bytes() for k in (1, 2)]
    for k in (1, 2):
        (d / ("A_comp_pe_dec_%d.fastq" % k)).unlink()
    rc, out = _minicom(["-d", "A_comp_pe.minicom"], d)
    assert rc == 0, out[-3000:]
    assert [(d / ("A_comp_pe_dec_%d.fastq" % k)).read_bytes() for k in (1, 2)] == gpu
    r1, r2 = _records(gpu[0]), _records(gpu[1])
    assert len(r1) == len(r2) == half
    got = sorted(x + y for x, y in zip(r1, r2))                                             # record j of one file is the mate of record j of the other
    want = sorted((reads[i].tobytes(), quals[i].tobytes(), reads[half + i].tobytes(), quals[half + i].tobytes()) for i in range(half))
    assert got == want


def test_minicom_q_paired_files_check(paired_q, tmp_path):
    d, reads, quals, half, dups = paired_q
    (tmp_path / "A_comp_pe.minicom").write_bytes((d / "A_comp_pe.minicom").read_bytes())
    rc, out = _minicom(["-d", "A_comp_pe.minicom", "-c", str(d / "A_1.fastq"), "-C", str(d / "A_2.fastq")], tmp_path)
    assert rc == 0 and "identical" in out, out[-3000:]
    # only the second file's quality differs, in one byte
    q2 = quals[half:].copy(); q2[321, 99] = 33 if q2[321, 99] != 33 else 34
    (tmp_path / "B_2.fastq").write_bytes(qc.fastq_bytes(reads[half:], q2))
    rc, out = _minicom(["-d", "A_comp_pe.minicom", "-c", str(d / "A_1.fastq"), "-C", "B_2.fastq"], tmp_path)
    assert rc == 2 and "1 records of the FASTQ are missing" in out and " 321" in out, out[-3000:]
    # the quality lines of two pairs swapped in the first file only
    q1 = quals[:half].copy(); q1[[7, 700]] = q1[[700, 7]]
    (tmp_path / "B_1.fastq").write_bytes(qc.fastq_bytes(reads[:half], q1))
    rc, out = _minicom(["-d", "A_comp_pe.minicom", "-c", "B_1.fastq", "-C", str(d / "A_2.fastq")], tmp_path)
    assert rc == 2, out[-3000:]
    # one byte of the first file's quality lines of two exact-duplicate pairs: reads and mates alone would still be the same multiset of pairs
    a, b = dups[0]
    assert np.array_equal(reads[a], reads[b]) and np.array_equal(reads[half + a], reads[half + b]) and not np.array_equal(quals[a], quals[b])
    q3 = quals[:half].copy()
    for i in (a, b):
        q3[i, 50] = 33 if q3[i, 50] != 33 else 34
    (tmp_path / "D_1.fastq").write_bytes(qc.fastq_bytes(reads[:half], q3))
    rc, out = _minicom(["-d", "A_comp_pe.minicom", "-c", "D_1.fastq", "-C", str(d / "A_2.fastq")], tmp_path)
    assert rc == 2 and "2 records of the FASTQ are missing" in out and "2 records of the archive are not in the FASTQ" in out, out[-3000:]
    # ... and of the second file's, of another duplicate pair
    a, b = dups[1]
    q4 = quals[half:].copy()
    for i in (a, b):
        q4[i, 60] = 33 if q4[i, 60] != 33 else 34
    (tmp_path / "D_2.fastq").write_bytes(qc.fastq_bytes(reads[half:], q4))
    rc, out = _minicom(["-d", "A_comp_pe.minicom", "-c", str(d / "A_1.fastq"), "-C", "D_2.fastq"], tmp_path)
    assert rc == 2 and "2 records of the FASTQ are missing" in out, out[-3000:]
    assert sorted(os.listdir(tmp_path)) == ["A_comp_pe.minicom", "B_1.fastq", "B_2.fastq", "D_1.fastq", "D_2.fastq"]


def test_python_route_and_the_gpu_decoders_refuse_what_the_host_refuses(single_q, tmp_path):
    """container.compress_fastq(quality_reordered=True) -> decompress_file on both routes -> verify_file; a -p archive and a missing member
    are refused by the GPU decoders as by the host ones, with no output file"""
    from minicom_amd import McomError, container, pipeline
    d, reads, quals, _ = single_q
    sizes = container.compress_fastq(str(d / "X.fastq"), str(tmp_path / "py.minicom"), codec="rans", device=0, threads=2, quality_reordered=True)
    assert sizes["n_reads"] == reads.shape[0] and sizes["rqual.mcq"] > 0 and "read_order.bin" not in sizes
    assert container.decompress_file(str(tmp_path / "py.minicom"), str(tmp_path / "gpu.fastq"), device=0) == reads.shape[0]
    assert container.decompress_file(str(tmp_path / "py.minicom"), str(tmp_path / "host.fastq")) == reads.shape[0]
    assert (tmp_path / "gpu.fastq").read_bytes() == (tmp_path / "host.fastq").read_bytes()
    assert sorted(_records((tmp_path / "gpu.fastq").read_bytes())) == sorted((reads[i].tobytes(), quals[i].tobytes()) for i in range(reads.shape[0]))
    rep = container.verify_file(str(tmp_path / "py.minicom"), str(d / "X.fastq"))
    assert rep["identical"] and rep["n_input"] == rep["n_archive"] == reads.shape[0]
    kinds = container.unpack(str(tmp_path / "py.minicom"), str(tmp_path / "un"))
    assert kinds == {"order": False, "paired": False, "quality_reordered": True}
    (tmp_path / "un" / "rqual.mcq").rename(tmp_path / "un" / "gone.mcq")
    with pytest.raises(McomError):
        pipeline.decompress_fastq_reordered(str(tmp_path / "un"), str(tmp_path / "no.fastq"), device=0)
    with pytest.raises(McomError):
        pipeline.verify_records(str(tmp_path / "un"), str(d / "X.fastq"))
    (tmp_path / "un" / "gone.mcq").rename(tmp_path / "un" / "rqual.mcq")
    (tmp_path / "un" / "allA.ids.bin").write_bytes(b"")                                     # the mark of a -p archive
    with pytest.raises(McomError):
        pipeline.decompress_fastq_reordered(str(tmp_path / "un"), str(tmp_path / "no.fastq"), device=0)
    assert not (tmp_path / "no.fastq").exists()


# ---- the GPU decoders refuse what the host decoders refuse -------------------------------------------------------------------------------
from test_reordered_qual import _copy, _extract, _refused, default_archive, paired_archive   # noqa: E402,F401  (the golden archives and the refusal check of the CPU tests)


def test_gpu_decoders_refuse_what_the_host_decoders_refuse(golden_dir, default_archive, paired_archive, tmp_path):  # noqa: F811
    """the cases of tests/test_reordered_qual.py on GPU 0: a -p archive, an archive of the other kind, a missing member, a member of another n
    or L, a damaged member, a pair with one member -- an error and no output file, of two outputs neither; the archives as they are decode to
    the host routes' bytes"""
    from minicom_amd import pipeline
    d0, rows, quals = default_archive
    dp, (r1, r2), (q1, q2) = paired_archive
    n, npair, L = rows.shape[0], r1.shape[0], rows.shape[1]
    assert pipeline.decompress_fastq_reordered(str(d0), str(tmp_path / "ok.fastq"), device=0) == n
    assert (tmp_path / "ok.fastq").read_bytes() == qc.fastq_bytes(rows, quals)
    assert pipeline.decompress_fastq_pe(str(dp), str(tmp_path / "ok1.fastq"), str(tmp_path / "ok2.fastq"), device=0) == npair
    assert ((tmp_path / "ok1.fastq").read_bytes(), (tmp_path / "ok2.fastq").read_bytes()) == (qc.fastq_bytes(r1, q1), qc.fastq_bytes(r2, q2))
    d = tmp_path / "order"
    _extract(golden_dir, "streams_order_stages_L100.tar.gz", d)
    for name in ("rqual.mcq", "rqual_1.mcq", "rqual_2.mcq"):
        (d / name).write_bytes(pipeline.qual_encode(qc.synth_quals(1, n, L)))
    assert _refused(tmp_path, d, False, device=0) and _refused(tmp_path, d, True, device=0)
    d = tmp_path / "pe_as_default"; _copy(dp, d); (d / "rqual.mcq").write_bytes(pipeline.qual_encode(qc.synth_quals(1, 2 * npair, L)))
    assert _refused(tmp_path, d, False, device=0)
    d = tmp_path / "default_as_pe"; _copy(d0, d)
    for name in ("rqual_1.mcq", "rqual_2.mcq"):
        (d / name).write_bytes(pipeline.qual_encode(qc.synth_quals(1, n // 2, L)))
    assert _refused(tmp_path, d, True, device=0)
    for name, q in {"none": None, "n": qc.synth_quals(1, n - 1, L), "L": qc.synth_quals(1, n, L - 1)}.items():
        d = tmp_path / ("d_" + name); _copy(d0, d); (d / "rqual.mcq").unlink()
        if q is not None:
            (d / "rqual.mcq").write_bytes(pipeline.qual_encode(q))
        assert _refused(tmp_path, d, False, device=0), name
    d = tmp_path / "d_damaged"; _copy(d0, d)
    b = bytearray((d / "rqual.mcq").read_bytes()); b[len(b) // 2] ^= 4; (d / "rqual.mcq").write_bytes(bytes(b))
    assert _refused(tmp_path, d, False, device=0)
    for which in ("rqual_1.mcq", "rqual_2.mcq"):
        for name, q in {"none": None, "n": qc.synth_quals(1, npair + 1, L), "L": qc.synth_quals(1, npair, L + 1)}.items():
            d = tmp_path / ("p_%s_%s" % (which[6], name)); _copy(dp, d); (d / which).unlink()
            if q is not None:
                (d / which).write_bytes(pipeline.qual_encode(q))
            assert _refused(tmp_path, d, True, device=0), (which, name)
        d = tmp_path / ("p_%s_damaged" % which[6]); _copy(dp, d)
        b = bytearray((d / which).read_bytes()); b[len(b) // 2] ^= 4; (d / which).write_bytes(bytes(b))
        assert _refused(tmp_path, d, True, device=0), which
