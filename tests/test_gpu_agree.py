"""`minicom -a Q[:C]` on the device: mcom_agree_coverage, mcom_agree_mask and mcom_qual_agree against the
independent statement of tests/agree_cases.py with canaries around everything they write; mcomh_agree_mask on the GPU against its host
twin, byte for byte; `bin/minicom -a` end to end per archive kind; the Python container."""
import functools
import gzip
import io
import os
import re
import shutil
import subprocess
import tarfile

import numpy as np
import pytest

import agree_cases as AC
import name_cases as nc
import qual_cases as qc
import qual_lossy_reference as LR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5


@pytest.fixture(scope="module")
def ctx():
    import minicom_amd
    return minicom_amd.Context(0)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def _bytes(path):
    return np.frombuffer(path.read_bytes(), np.uint8)


def _vacuity(bits, member_rows):
    m = bits[member_rows]
    assert m.any() and not m.all(), "vacuous: the members' mask rows are all %s" % ("set" if m.any() else "clear")


# ---- the device calls on hand-made stream sets ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,n_members", [(37, 15), (40, 16), (41, 17), (150, 33), (256, 33), (256, 16)])
def test_coverage_and_agree_kernels_on_hand_made_sets(ctx, tmp_path, L, n_members):
    import torch
    import minicom_amd.hip as H
    d = tmp_path / "a"
    reads, truth, member_rows, n_lists = AC.write_hand_made(d, L, n_members, False)
    (s,) = AC.hand_made_sets(L, n_members)
    img = _bytes(d / "beg_pos.bin.0")
    moff = ctx.decode_walk_headers(img)
    cid, pos, coff, ref_bases, flag = ctx.decode_member_table(_dev(img), _dev(moff), L)
    assert flag == 0 and ref_bases == sum(len(c) for c in s.contigs)
    # coverage: numpy over the builder's placements, canaries around the array
    want_cov = np.zeros(ref_bases + 1, np.int64)
    starts = np.concatenate([[0], np.cumsum([len(c) for c in s.contigs])])
    for c, p, _, _ in s.members:
        want_cov[starts[c] + p] += 1; want_cov[starts[c] + p + L] -= 1
    want_cov = np.cumsum(want_cov)[:-1]
    buf = torch.full((64 + ref_bases + 64,), CANARY, dtype=torch.uint8, device="cuda")
    cov, flag = ctx.decode_coverage(cid, pos, coff, L, ref_bases, out=buf[64:64 + ref_bases])
    g = buf.cpu().numpy()
    assert flag == 0 and np.array_equal(g[64:64 + ref_bases], np.minimum(want_cov, 255).astype(np.uint8))
    assert (g[:64] == CANARY).all() and (g[64 + ref_bases:] == CANARY).all()
    assert want_cov.max() >= 3 and len(set(want_cov[:L])) >= 2                                          # coverage steps inside the first read
    # the mask: scattered rows of a larger table, a pitch above ceil(L / 8), canaries in every byte the kernel must not write
    n = len(s.members)
    mb, pitch, n_rows = (L + 7) // 8, (L + 7) // 8 + 3, n + 5
    dest = np.random.default_rng(L).permutation(n_rows)[:n].astype(np.int64)
    text = _bytes(d / "dif_char.txt.0")
    start, _ = ctx.decode_line_index(_dev(text))
    src = dict(text=_dev(text), line_start=start, ref=_dev(_bytes(d / "ref.bin.0")), cid=cid, pos=pos, coff=coff, dirbits=_dev(_bytes(d / "dir.bin.0")))
    placements = [(m[0], m[1], m[2], r) for m, r in zip(s.members, reads[n_lists:])]
    for Cm in AC.HAND_C:
        mbuf = torch.full((64 + n_rows * pitch + 64,), CANARY, dtype=torch.uint8, device="cuda")
        _, flag = ctx.decode_agree(n, L, n_rows, cov=cov, min_cov=Cm, dest=_dev(dest), mask=mbuf[64:64 + n_rows * pitch], mask_pitch=pitch, **src)
        assert flag == 0
        g = mbuf.cpu().numpy()
        body = g[64:64 + n_rows * pitch].reshape(n_rows, pitch)
        want = AC.mask_of(s.contigs, placements, L, Cm)
        assert np.array_equal(want, truth(Cm)[member_rows])
        assert np.array_equal(body[dest, :mb], AC.pack_mask(want)), (L, Cm)
        assert (body[dest, mb:] == CANARY).all() and (np.delete(body, dest, axis=0) == CANARY).all()
        assert (g[:64] == CANARY).all() and (g[64 + n_rows * pitch:] == CANARY).all()
        if Cm <= 3:
            _vacuity(want, np.arange(n))
    # the decoder's rows of the same source are what the builder says: the mask rows lie beside the right reads
    out, flag = ctx.decode_reads(n, L, n_rows, dest=_dev(dest), **src)
    assert flag == 0
    rows = out.cpu().numpy().reshape(n_rows, L + 1)[dest, :L]
    assert [r.tobytes().decode() for r in rows] == reads[n_lists:]
    # sources without a member table: zero rows, whatever the coverage array says
    for kw in (dict(ref=_dev(_bytes(d / "single.seq"))), dict(ref_const="A"), dict(text=_dev(_bytes(d / "single_N.seq")), line_start=ctx.decode_line_index(_dev(_bytes(d / "single_N.seq")))[0], verbatim=True, ref_const="N")):
        k = 1 if "text" in kw else 2
        mbuf = torch.full((4 * mb,), CANARY, dtype=torch.uint8, device="cuda")
        _, flag = ctx.decode_agree(k, L, 4, cov=cov, min_cov=1, dest0=1, mask=mbuf, **kw)
        g = mbuf.cpu().numpy().reshape(4, mb)
        assert flag == 0 and (g[1:1 + k] == 0).all() and (g[0] == CANARY).all() and (g[1 + k:] == CANARY).all()
    # a member whose contig or place leaves the tables is flagged, not counted, and gets no set bit
    bad_cid = cid.clone(); bad_cid[0] = 1000
    cov2, flag = ctx.decode_coverage(bad_cid, pos, coff, L, ref_bases)
    assert flag == H.DECODE_F_BOUNDS
    w2 = np.zeros(ref_bases + 1, np.int64)
    for c, p, _, _ in s.members[1:]:
        w2[starts[c] + p] += 1; w2[starts[c] + p + L] -= 1
    assert np.array_equal(cov2.cpu().numpy(), np.cumsum(w2)[:-1].astype(np.uint8))
    bad_pos = pos.clone(); bad_pos[n - 1] = ref_bases
    _, flag = ctx.decode_coverage(cid, bad_pos, coff, L, ref_bases)
    assert flag == H.DECODE_F_BOUNDS
    mbuf = torch.full((n_rows * mb,), CANARY, dtype=torch.uint8, device="cuda")
    _, flag = ctx.decode_agree(n, L, n_rows, cov=cov, min_cov=1, dest=_dev(dest), mask=mbuf, **dict(src, pos=bad_pos))
    assert flag & H.DECODE_F_BOUNDS and (mbuf.cpu().numpy().reshape(n_rows, mb)[dest[n - 1]] == 0).all()
    with pytest.raises(H.McomError):
        ctx.decode_agree(n, L, n_rows, cov=cov, min_cov=0, dest=_dev(dest), **src)
    with pytest.raises(H.McomError):
        ctx.decode_agree(n, L, n_rows, cov=cov, min_cov=1, dest=_dev(dest), mask=mbuf, mask_pitch=mb - 1, **src)


def test_coverage_saturates_at_255(ctx):
    """300 members on one place: 255; 254 on another: exact"""
    L = 40
    pos = np.concatenate([np.zeros(300), np.full(254, 100)]).astype(np.uint32)
    cid = np.zeros(554, np.uint32)
    coff = np.array([0, 140], np.uint64)
    cov, flag = ctx.decode_coverage(_dev(cid), _dev(pos), _dev(coff), L, 140)
    want = np.zeros(140, np.uint8); want[:40] = 255; want[100:] = 254
    assert flag == 0 and np.array_equal(cov.cpu().numpy(), want)


@pytest.mark.parametrize("n", [0, 1, 17, 700])
@pytest.mark.parametrize("L,pitch_extra,offset,mask_extra,first", [(37, 0, 0, 0, 0), (40, 5, 3, 0, 3), (41, 1, 13, 2, 1), (150, 16, 8, 1, 0), (256, 0, 16, 0, 2), (1, 3, 1, 0, 0), (16, 0, 0, 0, 0),
                                                                     (17, 0, 15, 0, 0)])
def test_transform_kernel_with_canaries(ctx, L, pitch_extra, offset, mask_extra, first, n):
    import torch
    rng = np.random.default_rng(L * 1000 + n)
    pitch, mb = L + pitch_extra, (L + 7) // 8
    q = qc.synth_quals(L + n, max(n, 1), L)[:n].copy()
    q[1::2] = rng.integers(0, 256, q[1::2].shape, dtype=np.uint8)
    bits = rng.random((first + n, L)) < 0.6
    mask = np.full((first + n, mb + mask_extra), 0xFF, np.uint8)
    mask[:, :mb] = AC.pack_mask(bits)
    d_mask = torch.from_numpy(mask).cuda()
    for Q in (0, 40, 93):
        buf = torch.full((64 + offset + n * pitch + 64,), CANARY, dtype=torch.uint8, device="cuda")
        view = torch.as_strided(buf, (n, L), (pitch, 1), 64 + offset)
        if n:
            view.copy_(torch.from_numpy(q).cuda())
        want, rep = AC.transform(q, bits[first:], Q)
        _, got = ctx.qual_agree(view, d_mask, Q, first_mask_row=first, in_place=True)
        img = buf.cpu().numpy()
        body = img[64 + offset:64 + offset + n * pitch].reshape(n, pitch) if n else np.zeros((0, pitch), np.uint8)
        assert np.array_equal(body[:, :L], want), (L, n, Q)
        assert got == rep, (got, rep)
        assert (body[:, L:] == CANARY).all() and (img[:64 + offset] == CANARY).all() and (img[64 + offset + n * pitch:] == CANARY).all()
        assert np.array_equal(d_mask.cpu().numpy(), mask)
    if n == 17:                                                                                          # the host twin: the same bytes and report
        from minicom_amd.pipeline import qual_agree
        assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(qual_agree(q, mask, 40, first, device=0), qual_agree(q, mask, 40, first)))


def test_transform_kernel_refuses_bad_arguments(ctx):
    import torch
    from minicom_amd.hip import McomError, QualAgreeReport
    rows = torch.full((3, 40), 70, dtype=torch.uint8, device="cuda"); mask = torch.full((3, 5), 0xFF, dtype=torch.uint8, device="cuda")
    call = lambda n, L, pitch, mp, Q: ctx.lib.mcom_qual_agree(ctx._h, rows.data_ptr(), n, L, pitch, mask.data_ptr(), mp, 0, Q, None)
    for bad in ((3, 40, 40, 5, 94), (3, 0, 40, 5, 40), (3, 257, 257, 33, 40), (3, 40, 39, 5, 40), (3, 40, 40, 4, 40)):
        assert call(*bad) != 0, bad
        assert (rows == 70).all()
    assert call(3, 40, 40, 5, 40) == 0 and (rows == 73).all()


# ---- mcomh_agree_mask on the GPU against its host twin --------------------------------------------------------------------------------------------
def _both(folder, Cm):
    from minicom_amd.pipeline import agree_mask
    h = agree_mask(str(folder), Cm)
    g = agree_mask(str(folder), Cm, device=0)
    assert g[1:] == h[1:] and np.array_equal(g[0], h[0]), (str(folder), Cm)
    return g


@pytest.mark.parametrize("order", [False, True], ids=["default", "order"])
@pytest.mark.parametrize("L", AC.HAND_L)
def test_mask_on_the_gpu_equals_the_host_twin_on_hand_made_archives(tmp_path, L, order):
    for n_members in AC.HAND_MEMBERS:
        d = tmp_path / ("a%d" % n_members)
        reads, truth, member_rows, _ = AC.write_hand_made(d, L, n_members, order, second_set=n_members == 17)
        for Cm in (1, 3, 255):
            mask, gotL, bits = _both(d, Cm)
            assert gotL == L and np.array_equal(mask, AC.pack_mask(truth(Cm))), (L, n_members, order, Cm)


def _untar(golden_dir, name, d):
    d.mkdir()
    with gzip.open(os.path.join(golden_dir, name), "rb") as g:
        tf = tarfile.open(fileobj=io.BytesIO(g.read()))
        for m in tf.getmembers():
            (d / m.name).write_bytes(tf.extractfile(m).read())


@pytest.mark.parametrize("name", ["streams_order_stages_L100", "streams_order_stages_L150", "streams_stages_L40", "streams_stages_L100", "streams_stages_L150"])
def test_mask_on_the_gpu_equals_the_host_twin_on_the_golden_streams(golden_dir, tmp_path, name):
    d = tmp_path / "s"
    _untar(golden_dir, name + ".tar.gz", d)
    for Cm in (1, 3):
        _both(d, Cm)


def test_a_paired_end_default_mode_archive_has_no_mask(golden_dir, tmp_path):
    from minicom_amd.hip import McomError
    from minicom_amd.pipeline import agree_mask
    pe = tmp_path / "pe"
    _untar(golden_dir, "streams_pe_stages_L100.tar.gz", pe)
    for dev in (None, 0):
        with pytest.raises(McomError):
            agree_mask(str(pe), 3, device=dev, out_path=str(tmp_path / "m"))
        assert not (tmp_path / "m").exists()


@pytest.mark.parametrize("stream_sets", [1, 3])
def test_mask_of_a_pipeline_archive(tmp_path, stream_sets):
    """2 000 synthetic reads of 100 bases at coverage 30 with substitutions: GPU == host twin == the Python parser, default mode and -p"""
    from minicom_amd import synth
    from minicom_amd.pipeline import Pipeline
    reads = synth.synth_reads(77, 2000, 100, coverage=30, sub_rate=0.01)
    p = Pipeline(np.ascontiguousarray(reads), host_threads=4, stream_sets=stream_sets); p.pre_process()
    try:
        for order in (False, True):
            d = tmp_path / ("o%d" % order)
            d.mkdir()
            p.cluster_dump(str(d), order=order, paired=False)
            for Cm in (2, 3):
                mask, L, bits = _both(d, Cm)
                p_reads, p_bits, p_rows = AC.parse_folder(d, Cm)
                assert np.array_equal(mask, AC.pack_mask(p_bits)) and bits == int(p_bits.sum())
                _vacuity(p_bits, p_rows)
            if order:
                assert [r.encode() for r in p_reads] == [r.tobytes() for r in reads]
    finally:
        p.close()


def test_a_damaged_folder_has_no_mask_on_either_route(tmp_path):
    from minicom_amd.hip import McomError
    from minicom_amd.pipeline import agree_mask
    good = tmp_path / "good"
    AC.write_hand_made(good, 40, 17, True)

    def cut(name):
        def f(c):
            b = (c / name).read_bytes(); (c / name).write_bytes(b[:len(b) // 2])
        return f
    damages = {"dif_char cut": cut("dif_char.txt.0"), "ref cut": cut("ref.bin.0"), "ids cut": cut("ids.bin.0"), "dir cut": cut("dir.bin.0"),
               "bad line": lambda c: (c / "dif_char.txt.0").write_bytes(b"41\n" + (c / "dif_char.txt.0").read_bytes()),
               "id >= n_seq": lambda c: (c / "ids.bin.0").write_bytes(np.uint32(10 ** 6).tobytes() + (c / "ids.bin.0").read_bytes()[4:])}
    for name, damage in damages.items():
        c = tmp_path / "bad"
        shutil.copytree(good, c)
        damage(c)
        verdict = []
        for dev in (None, 0):
            try:
                agree_mask(str(c), 2, device=dev, out_path=str(tmp_path / "m")); verdict.append(False); os.remove(tmp_path / "m")
            except McomError:
                verdict.append(True); assert not (tmp_path / "m").exists(), name
        assert verdict[0] == verdict[1], name
        if name != "dir cut":                                                                            # (missing direction bits read as zero, on both routes)
            assert verdict[0], name
        shutil.rmtree(c)


# ---- records under the mask (`-q -a`): equal reads at places with different masks ---------------------------------------------------------------
def test_records_under_the_mask_need_an_exact_matching(tmp_path):
    """Four equal reads: three members of one contig (covered three times: every column masked at C = 2) and the lone member of a second
    contig with the same bases (covered once: no column masked).  The archive's rows hold Q, Q, Q and the fourth record's own values;
    the file lists that record FIRST, so an assignment that hands the first record the first row that takes it runs out of rows: only
    an exact matching finds that the two sides are the same records."""
    from minicom_amd.pipeline import agree_mask, qual_encode, verify_records
    L, Q = 40, 40
    rng = np.random.default_rng(9)
    contig = "".join("ACGT"[c] for c in rng.integers(0, 4, L))
    d = tmp_path / "s"
    d.mkdir()
    (d / "info.txt").write_text("%d 1 0 0 0\n" % L)
    for name in ("single.seq", "single_N.seq", "AA.txt", "TT.txt", "NN.txt"):
        (d / name).write_bytes(b"")
    (d / "beg_pos.bin.0").write_bytes(np.uint32(3).tobytes() + np.zeros(3, "<u2").tobytes() + np.uint32(1).tobytes() + np.zeros(1, "<u2").tobytes())
    (d / "ref.bin.0").write_bytes(AC._pack2(contig + contig))
    (d / "dir.bin.0").write_bytes(b"\0")
    (d / "dif_char.txt.0").write_bytes(b"\n\n\n\n")
    mask, _, bits_set = _both(d, 2)
    bits = AC.unpack_mask(mask, L)
    assert bits[:3].all() and not bits[3].any() and bits_set == 3 * L
    quals = qc.synth_quals(4, 4, L).copy()
    quals[:, 0] = [35, 36, 37, 38]                                                                       # four different rows, none of them Q throughout
    reads = np.frombuffer((contig * 4).encode(), np.uint8).reshape(4, L)
    (d / "rqual.mcq").write_bytes(qual_encode(AC.transform(quals, bits, Q)[0]))
    (d / "qual_agree.txt").write_bytes(b"%d 2\n" % Q)
    for name, file_order, identical in (("last_first", [3, 0, 1, 2], True), ("as_rows", [0, 1, 2, 3], True)):
        (tmp_path / (name + ".fastq")).write_bytes(qc.fastq_bytes(reads, quals[file_order]))
        rep = verify_records(str(d), str(tmp_path / (name + ".fastq")))
        assert rep["identical"] == identical and rep["missing"] == 0 and rep["extra"] == 0, (name, rep)
    changed = quals[[3, 0, 1, 2]].copy()
    changed[0, 5] ^= 1                                                                                   # the unmasked record, changed: no row takes it
    (tmp_path / "changed.fastq").write_bytes(qc.fastq_bytes(reads, changed))
    rep = verify_records(str(d), str(tmp_path / "changed.fastq"))
    assert not rep["identical"] and rep["missing"] == 1 and rep["extra"] == 1, rep
    masked = quals[[3, 0, 1, 2]].copy()
    masked[1:, :] = 70                                                                                   # the three masked records, any values: not kept, by definition
    (tmp_path / "masked.fastq").write_bytes(qc.fastq_bytes(reads, masked))
    assert verify_records(str(d), str(tmp_path / "masked.fastq"))["identical"]
    (d / "qual_agree.txt").write_bytes(b"x")
    from minicom_amd.hip import McomError
    with pytest.raises(McomError):
        verify_records(str(d), str(tmp_path / "as_rows.fastq"))


# ---- bin/minicom -a end to end ---------------------------------------------------------------------------------------------------------------
N_READS, L100 = 2000, 100


def _minicom(args, cwd):
    p = subprocess.run(["bash", os.path.join(ROOT, "bin", "minicom")] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    return p.returncode, p.stdout.decode(errors="replace")


def _named_fastq(reads, quals, names, plus) -> bytes:
    return b"".join(b"@" + names[i] + b"\n" + reads[i].tobytes() + b"\n+" + plus[i] + b"\n" + quals[i].tobytes() + b"\n" for i in range(reads.shape[0]))


def _members(archive):
    with tarfile.open(archive) as t:
        return {os.path.basename(m.name): t.extractfile(m).read() for m in t.getmembers() if m.isfile()}


def _retar(src, dst, marker):
    """the archive with qual_agree.txt dropped (marker None) or holding `marker`"""
    with tarfile.open(src) as t:
        items = [(m.name, t.extractfile(m).read()) for m in t.getmembers() if m.isfile()]
    assert any(os.path.basename(n) == "qual_agree.txt" for n, _ in items)
    with tarfile.open(dst, "w", format=tarfile.GNU_FORMAT) as t:
        for name, data in items:
            if os.path.basename(name) == "qual_agree.txt":
                if marker is None:
                    continue
                data = marker
            ti = tarfile.TarInfo(name); ti.size = len(data); ti.mode = 0o644
            t.addfile(ti, io.BytesIO(data))


@functools.lru_cache(maxsize=None)
def _inputs():
    from minicom_amd import synth
    reads = synth.synth_reads(1003, N_READS, L100, coverage=30, sub_rate=0.01)
    quals = qc.synth_quals(52, N_READS, L100)
    names = nc.illumina(6, N_READS)
    plus = nc.mixed_plus(names)
    return reads, quals, names, plus


ROUTES = {
    # name: (compress flags without -a / -b / -G, -a argument, -b spec or None, archive)
    "order": (["-r", "X.fastq", "-p", "-Q", "-N"], "40", None, "X_comp_order.minicom"),
    "pair": (["-1", "A_1.fastq", "-2", "A_2.fastq", "-p", "-Q", "-N"], "40", None, "A_comp_pe_order.minicom"),
    "both": (["-r", "X.fastq", "-p", "-Q"], "30:2", "ill8", "X_comp_order.minicom"),
    "reordered": (["-r", "X.fastq", "-q"], "40:2", None, "X_comp.minicom"),
}
PLAIN_NAMES = ("both", "reordered")         # routes whose records are named @1 ... @n


def _assign(row_reads, row_quals, reads, quals, bits, Q, bspec):
    """A `-q` archive keeps its own order: which record of the input is row j?  order[j] such that row j holds that record's read and its
    quality values sent through mask row j (then through the -b transform) -- found read group by read group, by trying the few ways a
    group of equal reads can be laid out.  Fails when there is no such order: that is the check of the archive's records."""
    import itertools
    by_read, rows_of = {}, {}
    for i in range(reads.shape[0]):
        by_read.setdefault(reads[i].tobytes(), []).append(i)
    for j, r in enumerate(row_reads):
        rows_of.setdefault(r.encode(), []).append(j)
    assert sorted(by_read) == sorted(rows_of)

    def fits(i, j):
        w = AC.transform(quals[i:i + 1], bits[j:j + 1], Q)[0]
        if bspec:
            w = LR.transform(w, bspec)[0]
        return np.array_equal(w[0], row_quals[j])
    order = np.full(len(row_reads), -1, np.int64)
    for r, js in rows_of.items():
        cand = by_read[r]
        assert len(cand) == len(js) <= 6
        ways = [p for p in itertools.permutations(cand) if all(fits(i, j) for i, j in zip(p, js))]
        assert ways, "no record of the input gives row %d under its mask row" % js[0]
        order[js] = ways[0]
    assert sorted(order) == list(range(reads.shape[0]))
    return order


@pytest.fixture(scope="module", params=sorted(ROUTES))
def route(request, tmp_path_factory):
    """the inputs of a route; its archive made with -a ... -G, in host/ the one made without -G, in plain/ the one made without -a; the
    mask the Python parser derives from the unpacked archive, and the quality values the archive must hold"""
    from minicom_amd import container
    name = request.param
    flags, aspec, bspec, archive = ROUTES[name]
    d = tmp_path_factory.mktemp("agree_" + name)
    reads, quals, names, plus = _inputs()
    half = N_READS // 2
    files = {}
    if name == "order":
        files["X.fastq"] = _named_fastq(reads, quals, names, plus)
    elif name in PLAIN_NAMES:
        files["X.fastq"] = qc.fastq_bytes(reads, quals)
    else:
        files["A_1.fastq"] = _named_fastq(reads[:half], quals[:half], names[:half], plus[:half])
        files["A_2.fastq"] = _named_fastq(reads[half:], quals[half:], names[half:], plus[half:])
    outs = {}
    for sub, extra in (("", ["-a", aspec, "-G"]), ("host", ["-a", aspec]), ("plain", ["-G"])):
        w = d / sub if sub else d
        w.mkdir(exist_ok=True)
        for f, data in files.items():
            (w / f).write_bytes(data)
        rc, out = _minicom(flags + extra + (["-b", bspec] if bspec else []) + ["-t", "2"], w)
        assert rc == 0, out[-3000:]
        assert sorted(f for f in os.listdir(w) if f not in ("host", "plain")) == sorted(list(files) + [archive]), "the temporary mask must not stay"
        outs[sub] = out
    Q, Cm = (int(x) for x in (aspec + ":3").split(":")[:2])
    container.unpack(str(d / archive), str(d / "unpacked"), device=0)
    p_reads, bits, member_rows = AC.parse_folder(d / "unpacked", Cm)
    order = np.arange(N_READS)
    if name == "reordered":                                                                              # rows in the archive's own order, as records
        from minicom_amd.pipeline import qual_decode
        order = _assign(p_reads, qual_decode((d / "unpacked" / "rqual.mcq").read_bytes()), reads, quals, bits, Q, bspec)
    shutil.rmtree(d / "unpacked")
    assert [r.encode() for r in p_reads] == [r.tobytes() for r in reads[order]]
    _vacuity(bits, member_rows)
    want_q, rep = AC.transform(quals[order], bits, Q)                                                    # row j of the archive
    if bspec:
        want_q = LR.transform(want_q, bspec)[0]
    rows = bits
    bits = np.zeros_like(rows); bits[order] = rows                                                       # mask row of input record i
    check = ["-c", "X.fastq"] if name != "pair" else ["-c", "A_1.fastq", "-C", "A_2.fastq"]
    return dict(name=name, d=d, flags=flags, aspec=aspec, bspec=bspec, archive=archive, check=check, files=files, outs=outs, Q=Q, C=Cm, bits=bits, want_q=want_q, rep=rep, order=order)


def test_minicom_a_members_and_report(route):
    r = route
    d, archive = r["d"], r["archive"]
    gm, hm, pm = _members(d / archive), _members(d / "host" / archive), _members(d / "plain" / archive)
    assert gm["qual_agree.txt"] == b"%d %d\n" % (r["Q"], r["C"]) and "qual_agree.txt" not in pm
    mcq = [k for k in gm if k.endswith(".mcq")]
    assert mcq and all(gm[k] == hm[k] for k in mcq)                                                      # with and without -G: the same members
    assert all(gm[k] != pm[k] for k in mcq)
    # an archive made without -a: the same members but the marker, every stream file the same bytes (the members are packed tar files,
    # which carry the time of their making: the files inside are what is compared), and nothing of -a in it
    assert sorted(set(gm) - {"qual_agree.txt"}) == sorted(pm)
    from minicom_amd import container
    folders = []
    for sub in ("", "plain"):
        u = d / ("unpacked_" + (sub or "agree"))
        container.unpack(str(d / sub / archive), str(u), device=0)
        folders.append({f: (u / f).read_bytes() for f in sorted(os.listdir(u))})
        shutil.rmtree(u)
    assert sorted(set(folders[0]) - {"qual_agree.txt"}) == sorted(folders[1])
    assert all(folders[0][f] == folders[1][f] for f in folders[1] if not f.endswith(".mcq"))
    # the report of the quality pass: mask bits and changed bytes are the Python statement's
    for out in (r["outs"][""], r["outs"]["host"]):
        got = [(int(a), int(b)) for a, b in re.findall(r"agree %d: mask_bits (\d+) changed (\d+)" % r["Q"], out)]
        assert len(got) == (2 if r["name"] == "pair" else 1)
        assert sum(g[0] for g in got) == r["rep"]["mask_bits"] and sum(g[1] for g in got) == r["rep"]["changed"] and r["rep"]["changed"] > 0


@pytest.mark.parametrize("gpu", [["-G"], []], ids=["G", "host"])
def test_minicom_a_decodes_to_the_transformed_file(route, gpu):
    r = route
    d, archive, name = r["d"], r["archive"], r["name"]
    reads, quals, names, plus = _inputs()
    half = N_READS // 2
    rc, out = _minicom(["-d", archive] + gpu, d)
    assert rc == 0 and ("the quality values of this archive are lossy: agreeing bases stored as Phred %d (coverage >= %d)\n" % (r["Q"], r["C"])) in out, out[-3000:]
    assert (r["bspec"] is None) == ("stored under" not in out)
    stem = archive[:-len(".minicom")]
    w = r["want_q"]
    if name == "order":
        assert (d / (stem + "_dec.fastq")).read_bytes() == _named_fastq(reads, w, names, plus)
    elif name in PLAIN_NAMES:
        assert (d / (stem + "_dec.fastq")).read_bytes() == qc.fastq_bytes(reads[r["order"]], w)
    else:
        assert (d / (stem + "_dec_1.fastq")).read_bytes() == _named_fastq(reads[:half], w[:half], names[:half], plus[:half])
        assert (d / (stem + "_dec_2.fastq")).read_bytes() == _named_fastq(reads[half:], w[half:], names[half:], plus[half:])


def _edited(r, what):
    """the route's input files with one byte changed: a quality value at a masked / an unmasked column, or a base"""
    reads, quals, names, plus = _inputs()
    reads, quals = reads.copy(), quals.copy()
    bits = r["bits"]
    if what == "longer":                                                                                 # one record more than the archive has rows, per file
        half = N_READS // 2
        names, plus = list(names), list(plus)
        at = [half - 1, N_READS - 1] if r["name"] == "pair" else [N_READS - 1]
        reads, quals = (np.insert(a, [k + 1 for k in at], a[at], axis=0) for a in (reads, quals))
        for k in reversed(at):
            names = names[:k + 1] + [names[k]] + names[k + 1:]; plus = plus[:k + 1] + [plus[k]] + plus[k + 1:]
        n_all = reads.shape[0]
        if r["name"] == "order":
            return {"X.fastq": _named_fastq(reads, quals, names, plus)}
        if r["name"] in PLAIN_NAMES:
            return {"X.fastq": qc.fastq_bytes(reads, quals)}
        h = n_all // 2
        return {"A_1.fastq": _named_fastq(reads[:h], quals[:h], names[:h], plus[:h]), "A_2.fastq": _named_fastq(reads[h:], quals[h:], names[h:], plus[h:])}
    if what == "base":
        j, i = np.argwhere(bits)[len(np.argwhere(bits)) // 2]
        reads[j, i] = ord("A") if reads[j, i] != ord("A") else ord("C")
    else:
        # a value of Phred 30 or more becomes Phred 2: the -b transform (where there is one) does not fold the two onto one bin
        cand = np.argwhere((bits if what == "masked" else ~bits) & (quals >= 33 + 30))
        j, i = cand[len(cand) // 2]
        quals[j, i] = 33 + 2
    half = N_READS // 2
    if r["name"] == "order":
        return {"X.fastq": _named_fastq(reads, quals, names, plus)}
    if r["name"] in PLAIN_NAMES:
        return {"X.fastq": qc.fastq_bytes(reads, quals)}
    return {"A_1.fastq": _named_fastq(reads[:half], quals[:half], names[:half], plus[:half]), "A_2.fastq": _named_fastq(reads[half:], quals[half:], names[half:], plus[half:])}


@pytest.mark.parametrize("what,want_rc", [("input", 0), ("masked", 0), ("unmasked", 2), ("base", 2), ("longer", 2)])
def test_minicom_a_check(route, what, want_rc):
    """-d -c on the input; with one quality byte changed at a masked column (that byte is not kept, by definition: identical), at an
    unmasked column, with one base changed, and with one record more than the archive holds (different, not refused)"""
    r = route
    d, archive, check = r["d"], r["archive"], r["check"]
    before = set(os.listdir(d))
    e = d / ("edit_" + what)
    e.mkdir()
    for f, data in (r["files"] if what == "input" else _edited(r, what)).items():
        (e / f).write_bytes(data)
    shutil.copy(d / archive, e / archive)
    rc, out = _minicom(["-d", archive] + check, e)
    assert rc == want_rc, (what, out[-3000:])
    assert ("DIFFERENT" in out) == (want_rc == 2), (what, out[-3000:])
    if what == "input":
        want = "identical under agree %d:%d" % (r["Q"], r["C"]) + (" and under %s" % r["bspec"] if r["bspec"] else "")
        assert want in out, out[-3000:]
    assert sorted(os.listdir(e)) == sorted(list(r["files"]) + [archive])                                 # -c leaves nothing behind
    shutil.rmtree(e)
    assert set(os.listdir(d)) == before


@pytest.mark.parametrize("marker,want_rc", [(b"x", 1), (None, 2)], ids=["garbage", "removed"])
def test_minicom_a_check_and_the_marker(route, marker, want_rc):
    """a marker that does not parse is refused; a marker removed leaves the file's own values to be expected, and they differ"""
    r = route
    d, archive, check = r["d"], r["archive"], r["check"]
    t = d / ("marker_%d" % want_rc)
    t.mkdir()
    _retar(d / archive, t / archive, marker)
    for f in r["files"]:
        shutil.copy(d / f, t / f)
    rc, out = _minicom(["-d", archive] + check, t)
    assert rc == want_rc, out[-3000:]
    assert ("qual_agree.txt" in out) if want_rc == 1 else ("DIFFERENT" in out), out[-3000:]
    shutil.rmtree(t)


def test_an_archive_without_a_verifies_as_before(route):
    r = route
    rc, out = _minicom(["-d", r["archive"]] + r["check"], r["d"] / "plain")
    assert rc == 0 and "identical" in out and "agree" not in out, out[-3000:]


REFUSALS = [
    (["-r", "X.fastq", "-p", "-a", "40", "-G"], "there are no quality values to change"),
    (["-r", "X.fastq", "-a", "40", "-G"], "there are no quality values to change"),
    (["-1", "X.fastq", "-2", "Y.fastq", "-q", "-a", "40", "-G"], "-a with -1/-2 needs -p"),
    (["-1", "X.fastq", "-2", "Y.fastq", "-a", "40", "-G"], "-a with -1/-2 needs -p"),
    (["-1", "X.fastq", "-2", "Y.fastq", "-Q", "-a", "40", "-G"], "-a with -1/-2 needs -p"),
    (["-1", "X.fastq", "-2", "Y.fastq", "-p", "-a", "40", "-G"], "there are no quality values to change"),
    (["-r", "X.fastq", "-q", "-V", "-a", "40", "-G"], "-V cannot be combined with -q"),
    (["-r", "X.fastq", "-p", "-V", "-Q", "-a", "40", "-G"], "-a cannot be combined with -V"),
    (["-r", "X.fastq", "-p", "-Q", "-a", "94", "-G"], "-a takes Q or Q:C"),
    (["-r", "X.fastq", "-p", "-Q", "-a", "40:0", "-G"], "-a takes Q or Q:C"),
    (["-r", "X.fastq", "-p", "-Q", "-a", "40:256", "-G"], "-a takes Q or Q:C"),
    (["-r", "X.fastq", "-p", "-Q", "-a", "040", "-G"], "-a takes Q or Q:C"),
    (["-r", "X.fastq", "-p", "-Q", "-a", "40:", "-G"], "-a takes Q or Q:C"),
    (["-r", "X.fastq", "-p", "-Q", "-a", "x", "-G"], "-a takes Q or Q:C"),
    (["-r", "X.fastq", "-p", "-Q", "-a", "4 0", "-G"], "-a takes Q or Q:C"),
]


def test_minicom_a_refusals_leave_nothing(tmp_path):
    reads, quals, names, plus = _inputs()
    (tmp_path / "X.fastq").write_bytes(qc.fastq_bytes(reads[:200], quals[:200]))
    (tmp_path / "Y.fastq").write_bytes(qc.fastq_bytes(reads[200:400], quals[200:400]))
    for args, words in REFUSALS:
        rc, out = _minicom(args, tmp_path)
        assert rc == 1 and words in out, (args, out[-2000:])
        assert sorted(os.listdir(tmp_path)) == ["X.fastq", "Y.fastq"], args


# ---- the Python container ----------------------------------------------------------------------------------------------------------------------
def test_container_round_trip_and_verify(route, tmp_path):
    from minicom_amd import container
    from minicom_amd.hip import McomError
    r = route
    d = r["d"]
    files = [str(d / f) for f in sorted(r["files"])]
    out = str(tmp_path / "py.minicom")
    qa = (r["Q"], r["C"])
    if r["name"] == "order":
        container.compress_fastq(files[0], out, order=True, quality=True, names=True, quality_agree=qa, codec="rans")
    elif r["name"] == "both":
        container.compress_fastq(files[0], out, order=True, quality=True, quality_agree=qa, quality_lossy=r["bspec"], codec="rans")
    elif r["name"] == "reordered":
        container.compress_fastq(files[0], out, quality_reordered=True, quality_agree=qa, codec="rans")
    else:
        container.compress_fastq_pair(files[0], files[1], out, quality=True, names=True, quality_agree=qa, codec="rans")
    gm, sm = _members(out), _members(d / r["archive"])
    assert gm["qual_agree.txt"] == b"%d %d\n" % qa and all(gm[k] == sm[k] for k in sm if k.endswith(".mcq"))   # the script's members
    rep = container.verify_file(out, *files)
    assert rep["identical"] and rep["quality_agree"] == qa
    outs = [str(tmp_path / ("o%d.fastq" % k)) for k in range(len(files))]
    container.decompress_file(out, *outs, device=0)
    reads, quals, names, plus = _inputs()
    half = N_READS // 2
    w = r["want_q"]
    if r["name"] == "order":
        assert open(outs[0], "rb").read() == _named_fastq(reads, w, names, plus)
    elif r["name"] in PLAIN_NAMES:
        assert open(outs[0], "rb").read() == qc.fastq_bytes(reads[r["order"]], w)
    else:
        assert open(outs[1], "rb").read() == _named_fastq(reads[half:], w[half:], names[half:], plus[half:])
    _retar(out, str(tmp_path / "bad.minicom"), b"garbage\n")
    with pytest.raises(McomError):
        container.verify_file(str(tmp_path / "bad.minicom"), *files)
    _retar(out, str(tmp_path / "no.minicom"), None)
    assert not container.verify_file(str(tmp_path / "no.minicom"), *files)["identical"]
    for kw in (dict(quality_agree=(40, 3)), dict(order=True, quality=True, quality_agree=(94, 3)), dict(order=True, quality=True, quality_agree=(40, 0)),
               dict(quality_reordered=True, path2=files[0], quality_agree=(40, 3)), dict(quality_reordered=True, quality_agree=(40, 256)), dict(order=True, quality=True, ragged=True, quality_agree=(40, 3))):
        with pytest.raises(ValueError):
            container.compress_fastq(files[0], str(tmp_path / "x.minicom"), **kw)
    assert not (tmp_path / "x.minicom").exists()
