"""The device decoder (csrc/decode.hip under host/mcom_decompress_gpu.cpp) against the host decoder, which is the specification: the same
output files byte for byte, the same archives refused.  Pieces of it against numpy restatements written here."""
import gzip
import hashlib
import io
import os
import tarfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
MODES = ["default", "order", "paired"]


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------
def _host(d, mode, stem):
    from minicom_amd.pipeline import decompress, decompress_pe
    outs = [stem + ".h1"] + ([stem + ".h2"] if mode == "paired" else [])
    n = decompress_pe(str(d), *outs) if mode == "paired" else decompress(str(d), outs[0], order=mode == "order")
    return n, [open(o, "rb").read() for o in outs]


def _gpu(d, mode, stem):
    from minicom_amd.pipeline import decompress, decompress_pe
    outs = [stem + ".g1"] + ([stem + ".g2"] if mode == "paired" else [])
    n = decompress_pe(str(d), *outs, device=0) if mode == "paired" else decompress(str(d), outs[0], order=mode == "order", device=0)
    return n, [open(o, "rb").read() for o in outs]


def _same(d, mode, tmp_path, name="x"):
    """both routes on one archive: byte-identical files; returns them"""
    stem = str(tmp_path / name)
    hn, h = _host(d, mode, stem)
    gn, g = _gpu(d, mode, stem)
    assert gn == hn
    for a, b in zip(g, h):
        assert len(a) == len(b) and a == b, (name, mode)
    return g


def _try(fn, d, mode, stem):
    """(refused?, files) of one route; whatever a refusing route left behind is removed"""
    from minicom_amd.hip import McomError
    try:
        return False, fn(d, mode, stem)[1]
    except McomError:
        return True, None


def _dump(reads, d, mode, stream_sets=1, pipeline=None):
    from minicom_amd.pipeline import Pipeline
    p = pipeline
    if p is None:
        p = Pipeline(np.ascontiguousarray(reads), host_threads=4, stream_sets=stream_sets); p.pre_process()
    d.mkdir()
    p.cluster_dump(str(d), order=mode == "order", paired=mode == "paired")
    if pipeline is None:
        p.close()


def _untar(golden_dir, name, d):
    d.mkdir()
    with gzip.open(os.path.join(golden_dir, name), "rb") as g:
        tf = tarfile.open(fileobj=io.BytesIO(g.read()))
        for m in tf.getmembers():
            (d / m.name).write_bytes(tf.extractfile(m).read())


def _golden_reads(golden_dir, tag):
    with gzip.open(os.path.join(golden_dir, tag + ".reads.gz"), "rb") as f:
        return f.read().split(b"\n")[:-1]


def _pack2(codes):
    """bases 0..3 -> 4 per byte, low bits first (single.seq / ref.bin)"""
    c = np.concatenate([np.asarray(codes, dtype=np.uint8), np.zeros((-len(codes)) % 4, dtype=np.uint8)]).reshape(-1, 4)
    return (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).astype(np.uint8).tobytes()


def _hand_made(d, L, single=b"", beg_pos=b"", ref=b"", dirb=b"", dif=b"", counts=(0, 0, 0), texts=(b"", b"", b""), nfile=b""):
    d.mkdir()
    (d / "info.txt").write_text("%d 1 %d %d %d\n" % ((L,) + tuple(counts)))
    for name, data in (("single.seq", single), ("single_N.seq", nfile), ("AA.txt", texts[0]), ("TT.txt", texts[1]), ("NN.txt", texts[2]),
                       ("beg_pos.bin.0", beg_pos), ("ref.bin.0", ref), ("dir.bin.0", dirb), ("dif_char.txt.0", dif)):
        (d / name).write_bytes(data)


# ---- 1. the reference's own streams -----------------------------------------------------------------------------------------------------
def _fixture_name(mode, L):
    return "streams_%sstages_L%d.tar.gz" % ({"default": "", "order": "order_", "paired": "pe_"}[mode], L)


_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = [(mode, L) for mode in MODES for L in (40, 100, 150) if os.path.exists(os.path.join(_GOLDEN, _fixture_name(mode, L)))]


@pytest.mark.parametrize("mode,L", FIXTURES)
def test_reference_streams_decode_to_the_host_routes_bytes(golden_dir, tmp_path, mode, L):
    name = _fixture_name(mode, L)
    d = tmp_path / "s"
    _untar(golden_dir, name, d)
    files = _same(d, mode, tmp_path)
    want = _golden_reads(golden_dir, "stages_L%d" % L)
    rows = [f.split(b"\n")[:-1] for f in files]
    if mode == "default":
        assert sorted(rows[0]) == sorted(want)
    elif mode == "order":
        assert rows[0] == want
    else:
        half = len(want) // 2
        assert sorted(zip(rows[0], rows[1])) == sorted(zip(want[:half], want[half:2 * half]))


# ---- 2. round trips no fixture covers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [40, 100, 150, 256, 176])
@pytest.mark.parametrize("stream_sets", [1, 5])
def test_round_trips_equal_the_host_route(tmp_path, L, stream_sets):
    from minicom_amd import synth
    from minicom_amd.pipeline import Pipeline
    reads = np.concatenate([synth.synth_reads(909, 120000, L), synth.synth_reads(910, 6000, L, plumbing=True)])
    n = reads.shape[0]
    p = Pipeline(reads, host_threads=8, stream_sets=stream_sets); p.pre_process()
    try:
        for mode in MODES:
            d = tmp_path / mode
            _dump(reads, d, mode, pipeline=p)
            files = _same(d, mode, tmp_path, mode)
            if mode == "order":
                assert np.array_equal(np.frombuffer(files[0], dtype=np.uint8).reshape(n, L + 1)[:, :L], reads)
            else:
                assert sum(len(f) for f in files) == n * (L + 1)
    finally:
        p.close()


def test_round_trip_of_four_million_reads_by_md5(tmp_path):
    from minicom_amd import synth
    from minicom_amd.pipeline import Pipeline
    L = 150
    reads = synth.synth_reads(4242, 4_000_000, L)
    p = Pipeline(reads, host_threads=8); p.pre_process()
    try:
        for mode in MODES:
            d = tmp_path / mode
            _dump(reads, d, mode, pipeline=p)
            stem = str(tmp_path / mode)
            hn, h = _host(d, mode, stem)
            gn, g = _gpu(d, mode, stem)
            assert gn == hn
            assert [hashlib.md5(x).hexdigest() for x in g] == [hashlib.md5(x).hexdigest() for x in h], mode
            for f in os.listdir(tmp_path):
                if f.startswith(mode + "."):
                    os.remove(tmp_path / f)
    finally:
        p.close()


# ---- 3. edges of the domain -------------------------------------------------------------------------------------------------------------
def test_edges_built_by_the_pipeline(tmp_path):
    from minicom_amd import synth
    L = 100
    base = synth.synth_reads(1000, 300, L)
    rng = np.random.default_rng(5)
    sets = {"two": base[:2].copy(), "copies_of_one": np.repeat(base[:1], 64, axis=0),
            "all_n": np.full((8, L), ord("N"), dtype=np.uint8),
            "specials": np.concatenate([np.full((6, L), ord("A"), dtype=np.uint8), np.full((4, L), ord("N"), dtype=np.uint8), base[:90], np.full((6, L), ord("T"), dtype=np.uint8), base[90:184]]),
            "only_singletons": np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(50, L))],
            "identical_mates": np.concatenate([base[:100], base[:100]])}
    for name, reads in sets.items():
        for mode in MODES:
            d = tmp_path / ("%s_%s" % (name, mode))
            _dump(reads, d, mode)
            if name == "only_singletons":
                assert (d / "beg_pos.bin.0").stat().st_size == 0
            _same(d, mode, tmp_path, "%s_%s" % (name, mode))


@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_hand_made_archives_of_unclustered_reads_only(tmp_path, n):
    """no reads at all; 1 - 3 reads of 75 bases leave the last byte of single.seq 3, 2 and 1 bases full"""
    L = 75
    rng = np.random.default_rng(n)
    codes = rng.integers(0, 4, size=n * L)
    d = tmp_path / "s"
    _hand_made(d, L, single=_pack2(codes))
    (g,) = _same(d, "default", tmp_path)
    assert g == b"".join(bytes(b"ACGT"[c] for c in codes[i * L:(i + 1) * L]) + b"\n" for i in range(n))


def test_hand_made_contigs_with_long_runs_empty_contigs_and_both_directions(tmp_path):
    """one contig holding several members, a contig of no member, a contig of one; a line with a multi-digit run, "0", literals at both ends;
    counted and near-constant reads and a read kept as text in front of them"""
    L = 150
    rng = np.random.default_rng(77)
    c0, c1 = rng.integers(0, 4, size=L + 130), rng.integers(0, 4, size=L)
    beg = b"".join([np.uint32(4).tobytes(), np.array([0, 0, 7, 123], "<u2").tobytes(), np.uint32(0).tobytes(), np.uint32(1).tobytes(), np.array([0], "<u2").tobytes()])
    dif = b"0\n120C\nT148G\n17AC3N\n5\n"
    d = tmp_path / "s"
    _hand_made(d, L, beg_pos=beg, ref=_pack2(np.concatenate([c0, c1])), dirb=bytes([0b10110]), dif=dif, counts=(2, 1, 3),
               texts=(b"10C\n", b"0\nGG\n", b""), nfile=b"N" * 149 + b"A\n", single=_pack2(rng.integers(0, 4, size=2 * L + 1)))
    (g,) = _same(d, "default", tmp_path)
    assert len(g) == (2 + 1 + 3 + 1 + 2 + 0 + 1 + 2 + 5) * (L + 1)


# ---- 4. pieces against numpy ------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("text", [b"", b"\n", b"abc", b"a\n\nbc\n", b"\n\n\n", b"12\nX\n\nlast line has no newline",
                                  bytes(np.random.default_rng(3).choice(np.frombuffer(b"A0\n", dtype=np.uint8), size=70001, p=[.45, .45, .1]))])
def test_line_index(ctx, text):
    start, flag = ctx.decode_line_index(_dev(np.frombuffer(text, dtype=np.uint8)))
    want = np.concatenate([[0], np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10) + 1])
    assert flag == 0 and np.array_equal(start.cpu().numpy(), want)


def _beg_pos(contigs):
    return b"".join(np.uint32(len(c)).tobytes() + np.asarray(c, dtype="<u2").tobytes() for c in contigs)


def test_member_table_and_member_ids(ctx):
    rng = np.random.default_rng(11)
    contigs = [[0], [5], [], [0, 0, 0, 65535, 0, 65535], [65535], [], []] + [list(rng.choice([0, 0, 1, 9, 300], size=int(k))) for k in rng.integers(1, 700, size=60)] + [[]]
    L = 100
    img = np.frombuffer(_beg_pos(contigs) + b"\x07", dtype=np.uint8)                       # a trailing byte short of a header is ignored
    moff = ctx.decode_walk_headers(img)
    assert np.array_equal(moff, np.concatenate([[0], np.cumsum([len(c) for c in contigs])]).astype(np.uint64))
    cid, pos, coff, ref_bases, flag = ctx.decode_member_table(_dev(img), _dev(moff), L)
    want_cid = np.concatenate([np.full(len(c), i) for i, c in enumerate(contigs)]).astype(np.int64)
    want_pos = np.concatenate([np.cumsum(c) for c in contigs if len(c)]).astype(np.int64)
    clen = np.array([int(np.sum(c)) + L if len(c) else 0 for c in contigs], dtype=np.int64)
    assert flag == 0
    assert np.array_equal(cid.cpu().numpy(), want_cid) and np.array_equal(pos.cpu().numpy(), want_pos)
    assert np.array_equal(coff.cpu().numpy(), np.concatenate([[0], np.cumsum(clen)])) and ref_bases == int(clen.sum())
    # -p ids: absolute for the first member of a contig and where the delta is non-zero, else a difference (32 bit)
    nm = len(want_cid)
    words = rng.integers(0, 1 << 32, size=nm, dtype=np.uint64).astype(np.uint32)
    want, q = np.zeros(nm, dtype=np.int64), 0
    for c in contigs:
        pre = 0
        for j, dlt in enumerate(c):
            idv = int(words[q]) + (pre if dlt == 0 else 0)
            pre = idv
            want[q] = idv & 0xFFFFFFFF
            q += 1
    got = ctx.decode_member_ids(_dev(words), _dev(moff), cid, pos)
    assert np.array_equal(got.cpu().numpy(), want)


def test_list_ids(ctx):
    rng = np.random.default_rng(12)
    for n in (1, 255, 256, 100003):
        delta = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        assert np.array_equal(ctx.decode_list_ids(_dev(delta)).cpu().numpy(), np.cumsum(delta.astype(np.int64)))


def test_paired_end_destinations(ctx):
    rng = np.random.default_rng(13)
    for n in (1, 9, 4097, 200001):
        bits = rng.integers(0, 2, size=n).astype(np.uint8)
        ones = int(bits.sum())
        half = max(n - ones + 3, ones)
        peids = rng.permutation(half)[:ones].astype(np.uint32)
        dest, got_ones, flag = ctx.decode_pe_dest(_dev(np.packbits(bits, bitorder="little")), n, _dev(peids), 3, half)
        want = np.where(bits == 1, half + peids[np.minimum(np.cumsum(bits) - bits, ones - 1)].astype(np.int64) if ones else 0, 3 + np.cumsum(1 - bits) - (1 - bits))
        assert flag == 0 and got_ones == ones and np.array_equal(dest.cpu().numpy(), want)
    # a mate row outside its half, a zero row outside its half, a missing mate word: flagged, row -1
    import minicom_amd.hip as H
    dest, _, flag = ctx.decode_pe_dest(_dev(np.array([0b101], dtype=np.uint8)), 3, _dev(np.array([1, 2], dtype=np.uint32)), 0, 2)
    assert flag == H.DECODE_F_DEST and dest.cpu().numpy().tolist() == [3, 0, -1]
    dest, _, flag = ctx.decode_pe_dest(_dev(np.array([0b11], dtype=np.uint8)), 2, _dev(np.array([0], dtype=np.uint32)), 0, 2)
    assert flag == H.DECODE_F_BOUNDS and dest.cpu().numpy().tolist() == [2, -1]


def test_decode_kernel_against_a_restatement(ctx):
    """random members on a random reference: literals, runs, both directions, scattered rows; L at the ends of the domain"""
    import minicom_amd.hip as H
    comp = {65: 84, 84: 65, 67: 71, 71: 67}
    for L in (1, 7, 40, 150, 255, 256):
        rng = np.random.default_rng(L)
        n, ref_len = 3000, 5000 + L
        ref = rng.integers(0, 4, size=ref_len)
        off = rng.integers(0, ref_len - L + 1, size=n)
        rev = rng.integers(0, 2, size=n).astype(np.uint8)
        lines, want = [], np.zeros((n, L + 1), dtype=np.uint8)
        for m in range(n):
            seq = np.frombuffer(b"ACGT", dtype=np.uint8)[ref[off[m]:off[m] + L]].copy()
            txt, at = b"", 0
            for p in sorted(rng.choice(L, size=min(L, int(rng.integers(0, 5))), replace=False)):
                run = p - at
                txt += (b"" if run == 0 else bytes([seq[at]]) if run == 1 and rng.integers(0, 2) else str(run).encode()) + b"N"
                seq[p] = ord("N"); at = p + 1
            lines.append(txt if txt or rng.integers(0, 2) else b"0")
            if rev[m]:
                seq = np.array([comp.get(int(c), 78) for c in seq[::-1]], dtype=np.uint8)
            want[m, :L], want[m, L] = seq, 10
        text = np.frombuffer(b"".join(t + b"\n" for t in lines), dtype=np.uint8)
        start, _ = ctx.decode_line_index(_dev(text))
        dest = rng.permutation(n + 5)[:n].astype(np.int64)
        import torch
        seen = torch.zeros((n + 5) // 32 + 1, dtype=torch.int32, device="cuda")
        # one contig per member would need its own table: instead every member is its own "contig" of the table (cid = m, coff = off, pos = 0)
        out, flag = ctx.decode_reads(n, L, n + 5, text=_dev(text), line_start=start, ref=_dev(np.frombuffer(_pack2(ref), dtype=np.uint8)),
                                     cid=_dev(np.arange(n, dtype=np.uint32)), pos=_dev(np.zeros(n, dtype=np.uint32)), coff=_dev(np.concatenate([off, [0]]).astype(np.uint64)),
                                     dirbits=_dev(np.packbits(rev, bitorder="little")), dest=_dev(dest), seen=seen)
        assert flag == 0, L
        assert np.array_equal(out.cpu().numpy().reshape(n + 5, L + 1)[dest], want), L
        # the same rows twice: flagged as duplicates, nothing else
        _, flag = ctx.decode_reads(n, L, n + 5, ref_const="T", dest=_dev(dest), seen=seen, out=out)
        assert flag == H.DECODE_F_DUP


# ---- 5. refused archives ----------------------------------------------------------------------------------------------------------------
def _corruptions(d, mode, L):
    """name -> function that damages a copy of the good archive `d`"""
    def trunc(name, how):
        def f(c):
            b = (c / name).read_bytes()
            (c / name).write_bytes(b[:len(b) - 1] if how == "one" else b[:len(b) // 2])
        return f

    def info_plus(i):
        def f(c):
            w = (c / "info.txt").read_text().split()
            w[i] = str(int(w[i]) + 1)
            (c / "info.txt").write_text(" ".join(w) + "\n")
        return f

    def patch(name, at, data):
        def f(c):
            b = bytearray((c / name).read_bytes())
            assert len(b) >= at + len(data), name
            b[at:at + len(data)] = data
            (c / name).write_bytes(bytes(b))
        return f

    def first_line(name, line):
        def f(c):
            b = (c / name).read_bytes()
            (c / name).write_bytes(line + b[b.index(b"\n"):])
        return f

    info = (d / "info.txt").read_text().split()
    files = ["dif_char.txt.0", "beg_pos.bin.0", "ref.bin.0", "dir.bin.0", "single.seq", "single_N.seq", "AA.txt"] + {"default": [], "order": ["ids.bin.0", "singleFile.ids.bin"], "paired": ["peids.bin.0", "file.bin.0", "file.bin.sp"]}[mode]
    out = {}
    for name in files:
        for how in ("one", "half"):
            out["%s cut by %s" % (name, how)] = trunc(name, how)
    for i in range(2, len(info)):
        out["info.txt word %d raised" % i] = info_plus(i)
    out["num = 2^31"] = patch("beg_pos.bin.0", 0, np.uint32(1 << 31).tobytes())
    out["digit run longer than L"] = first_line("dif_char.txt.0", str(L + 1).encode())
    out["run that passes L behind a literal"] = first_line("dif_char.txt.0", b"A" + str(L).encode() + b"C")
    out["byte 0x01 in dif_char"] = patch("dif_char.txt.0", 0, b"\x01")
    if mode == "order":
        out["id >= n_seq"] = patch("ids.bin.0", 0, np.uint32(int(info[5])).tobytes())
        out["duplicated id"] = patch("singleFile.ids.bin", 4, np.uint32(0).tobytes())
    if mode == "paired":
        out["mate row >= half"] = patch("peids.bin.0", 0, np.uint32(int(info[2])).tobytes())
        out["duplicated mate row"] = lambda c: (c / "peids.bin.0").write_bytes((lambda b: b[4:8] + b[4:])((c / "peids.bin.0").read_bytes()))
    return out


@pytest.mark.parametrize("mode", MODES)
def test_refused_archives(tmp_path, mode):
    import shutil
    from minicom_amd import synth
    L = 100
    reads = np.concatenate([synth.synth_reads(31, 30000, L), synth.synth_reads(32, 3000, L, plumbing=True)])
    good = tmp_path / "good"
    _dump(reads, good, mode)
    want = _same(good, mode, tmp_path, "good")
    verdicts = {}
    for name, damage in _corruptions(good, mode, L).items():
        c = tmp_path / "bad"
        shutil.copytree(good, c)
        damage(c)
        stem = str(tmp_path / "bad_out")
        h_refused, h = _try(_host, c, mode, stem)
        g_refused, g = _try(_gpu, c, mode, stem)
        assert g_refused == h_refused, name
        if g_refused:
            assert not os.path.exists(stem + ".g1") and not os.path.exists(stem + ".g2"), name
        else:
            assert g == h, name
        verdicts[name] = g_refused
        shutil.rmtree(c)
        for f in os.listdir(tmp_path):
            if f.startswith("bad_out"):
                os.remove(tmp_path / f)
    print(verdicts)
    for name in ("num = 2^31", "digit run longer than L", "byte 0x01 in dif_char", "dif_char.txt.0 cut by half", "beg_pos.bin.0 cut by half") + \
            {"default": (), "order": ("id >= n_seq", "duplicated id", "info.txt word 5 raised"), "paired": ("mate row >= half", "duplicated mate row", "info.txt word 2 raised")}[mode]:
        assert verdicts[name], name
    assert _same(good, mode, tmp_path, "again") == want                                      # and a good archive decodes afterwards
