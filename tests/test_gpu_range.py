"""A record range of a -p archive on the GPU (`minicom -d -R`): mcom_range_decode_reads against the rows of
mcom_decode_reads, mcom_range_check_dest, mcom_qual_decode_rows against the host twin's bytes -- each with canaries around what it may
write -- and `bin/minicom -d -G -R` end to end against slices of the input files, on both routes, through -z, for a pair, with the refusals."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import qual_reference as QR
import ragged_cases as rgc
import range_cases as rc

pytestmark = pytest.mark.gpu
ROOT = rc.ROOT
N = 53                                  # three groups of sixteen lanes' reads and a rest
WINDOWS = [(0, 0), (0, 1), (52, 1), (0, 53), (15, 2), (16, 16), (17, 36)]


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


def _pack2(codes):
    """bases 0..3 -> 4 per byte, low bits first (single.seq / ref.bin)"""
    c = np.concatenate([np.asarray(codes, dtype=np.uint8), np.zeros((-len(codes)) % 4, dtype=np.uint8)]).reshape(-1, 4)
    return (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).astype(np.uint8).tobytes()


def _sources(ctx, L):
    """name -> keyword arguments of decode_reads / decode_reads_window for N reads: members of a random reference with literals, runs and
    both directions (every member its own "contig": cid = m, coff = its offset, pos = 0), lines that are the reads (verbatim), lines over a
    constant base, a constant base alone, and 2-bit reads back to back (single.seq)"""
    rng = np.random.default_rng(1000 + L)
    ref_len = 400 + L
    ref = rng.integers(0, 4, size=ref_len)
    off = rng.integers(0, ref_len - L + 1, size=N)
    rev = rng.integers(0, 2, size=N).astype(np.uint8)
    lines, const_lines = [], []
    for m in range(N):
        txt, at = b"", 0
        for p in sorted(rng.choice(L, size=min(L, int(rng.integers(0, 5))), replace=False)):
            run = p - at
            txt += (b"" if run == 0 else str(run).encode()) + b"N"
            at = p + 1
        lines.append(txt if txt or rng.integers(0, 2) else b"0")
        const_lines.append(b"%dC" % (m % L) if m % 3 else b"")
    text = np.frombuffer(b"".join(t + b"\n" for t in lines), dtype=np.uint8)
    ctext = np.frombuffer(b"".join(t + b"\n" for t in const_lines), dtype=np.uint8)
    vtext = np.frombuffer(b"".join(bytes(rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=L)) + b"\n" for _ in range(N)), dtype=np.uint8)
    t, c, v = _dev(text), _dev(ctext), _dev(vtext)
    return {
        "members": dict(text=t, line_start=ctx.decode_line_index(t)[0], ref=_dev(np.frombuffer(_pack2(ref), dtype=np.uint8)), cid=_dev(np.arange(N, dtype=np.uint32)),
                        pos=_dev(np.zeros(N, dtype=np.uint32)), coff=_dev(np.concatenate([off, [0]]).astype(np.uint64)), dirbits=_dev(np.packbits(rev, bitorder="little"))),
        "verbatim": dict(text=v, line_start=ctx.decode_line_index(v)[0], verbatim=True, ref_const="N"),
        "constant lines": dict(text=c, line_start=ctx.decode_line_index(c)[0], ref_const="T"),
        "constant": dict(ref_const="A"),
        "single.seq": dict(ref=_dev(np.frombuffer(_pack2(rng.integers(0, 4, size=N * L)), dtype=np.uint8))),
    }


@pytest.mark.parametrize("L", [1, 15, 16, 31, 100, 255, 256])
def test_window_rows_are_the_rows_of_the_full_decode(ctx, L):
    """every source kind, a seeded permutation and the dest0 form, every window, d_out at an aligned and at an odd address: the window's
    rows byte for byte, no flag, and nothing written on either side of them"""
    import torch
    row = L + 1
    dest = np.random.default_rng(L).permutation(N).astype(np.int64)
    for name, src in _sources(ctx, L).items():
        for d in (_dev(dest), None):
            full, flag = ctx.decode_reads(N, L, N, dest=d, **src)
            assert flag == 0, (name, L)
            full = full.cpu().numpy().reshape(N, row)
            for first, count in WINDOWS:
                for odd in (0, 1):
                    buf = torch.full((64 + count * row + 64 + odd,), 0xC3, dtype=torch.uint8, device="cuda")
                    out = buf[48 + odd:48 + odd + count * row]
                    assert (buf.data_ptr() + 48 + odd) % 16 == odd          # (an empty window's tensor has no address of its own)
                    _, flag = ctx.decode_reads_window(N, L, first, count, dest=d, out=out, **src)
                    got = buf.cpu().numpy()
                    assert flag == 0, (name, L, first, count)
                    assert np.array_equal(got[48 + odd:48 + odd + count * row].reshape(count, row), full[first:first + count]), (name, L, first, count, odd)
                    assert (got[:48 + odd] == 0xC3).all() and (got[48 + odd + count * row:] == 0xC3).all(), (name, L, first, count, odd)
    # a read inside the window whose reference window leaves the reference raises F_BOUNDS; the same read outside the window is not looked at
    import minicom_amd.hip as H
    src = _sources(ctx, L)["members"]
    coff = src["coff"].clone(); coff[7] = 1 << 40
    bad = dict(src, coff=coff)
    _, flag = ctx.decode_reads_window(N, L, 7, 1, **bad)
    assert flag == H.DECODE_F_BOUNDS
    out, flag = ctx.decode_reads_window(N, L, 8, 45, **bad)
    full, _ = ctx.decode_reads(N, L, N, **src)
    assert flag == 0 and np.array_equal(out.cpu().numpy(), full.cpu().numpy()[8 * row:])


def test_check_dest(ctx):
    """the placement check on its own: a destination == n_rows, one duplicated row, a clean permutation -- over one source and over two that
    share the bits; more reads inside a window than it has rows are flagged by the window decode itself"""
    import minicom_amd.hip as H
    rng = np.random.default_rng(7)
    for n in (1, 53, 64, 65, 5000):
        perm = rng.permutation(n).astype(np.int64)
        flag, seen = ctx.decode_check_dest(n, n, dest=_dev(perm))
        assert flag == 0 and int(np.unpackbits(seen.cpu().numpy().view(np.uint8)).sum()) == n
        flag, _ = ctx.decode_check_dest(n, n, dest0=0)
        assert flag == 0
        bad = perm.copy(); bad[n // 2] = n
        assert ctx.decode_check_dest(n, n, dest=_dev(bad))[0] == H.DECODE_F_DEST
        assert ctx.decode_check_dest(n, n, dest0=1)[0] == H.DECODE_F_DEST
        if n > 1:
            dup = perm.copy(); dup[0] = dup[n - 1]
            assert ctx.decode_check_dest(n, n, dest=_dev(dup))[0] == H.DECODE_F_DUP
            a, b = perm[:n // 2], perm[n // 2:]                              # two sources of one archive
            f1, seen = ctx.decode_check_dest(len(a), n, dest=_dev(a))
            f2, seen = ctx.decode_check_dest(len(b), n, dest=_dev(b), seen=seen)
            f3, _ = ctx.decode_check_dest(1, n, dest=_dev(a[:1]), seen=seen)
            assert (f1, f2, f3) == (0, 0, H.DECODE_F_DUP)
    import torch
    buf = torch.full((16 + 2 * 11 + 16,), 0xC3, dtype=torch.uint8, device="cuda")
    _, flag = ctx.decode_reads_window(5, 10, 3, 2, ref_const="A", dest=_dev(np.array([3, 4, 3, 9, 4], dtype=np.int64)), out=buf[16:16 + 22])
    got = buf.cpu().numpy()
    assert flag == H.DECODE_F_DUP and (got[:16] == 0xC3).all() and (got[38:] == 0xC3).all()


@pytest.mark.parametrize("L,A", [(L, A) for L in rc.QUAL_L for A in rc.QUAL_A], ids=lambda v: str(v))
def test_qual_rows_equal_the_host_twins(ctx, L, A):
    """the grid of the host test, every forced model and kind 1 (A = 94 under model 4: the cumulative table in global memory; A = 4: in LDS):
    the host twin's bytes at pitch L and L + 1, nothing written outside the rows, the same refusal of first > n"""
    import torch
    from minicom_amd import McomError, pipeline
    n = rc.qual_matrix(L, A).shape[0]
    for model in rc.QUAL_MODELS:
        member = rc.qual_member(L, A, model)
        d_member = _dev(np.frombuffer(member, dtype=np.uint8))
        for first, count in rc.qual_ranges(L, n):
            want = pipeline.qual_decode_rows(member, first, count)
            c = want.shape[0]
            for pitch in (L, L + 1):
                buf = torch.full((c + 2, pitch), 0xC3, dtype=torch.uint8, device="cuda")
                got = ctx.qual_decode_rows(d_member, first, count, out=buf[1:1 + max(c, 1)] if c else buf[1:2])
                assert got.shape == (c, L) and np.array_equal(got.cpu().numpy(), want), (model, first, count, pitch)
                h = buf.cpu().numpy()
                assert (h[0] == 0xC3).all() and (h[1 + c:] == 0xC3).all() and (h[:, L:] == 0xC3).all(), (model, first, count, pitch)
        with pytest.raises(McomError):
            ctx.qual_decode_rows(d_member, n + 1, 1)
    if (L, A) == (100, 41):                                                 # the documented reach of a range's checks, as on the host
        q, rps = rc.qual_matrix(L, A), QR.default_rps(L)
        bad = _dev(np.frombuffer(rc.flip_in_segment(rc.qual_member(L, A, 3), 1), dtype=np.uint8))
        for first, count in ((rps, 1), (rps - 1, 2), (0, n)):
            with pytest.raises(McomError):
                ctx.qual_decode_rows(bad, first, count)
        for first, count in ((0, rps), (2 * rps, 3)):
            assert np.array_equal(ctx.qual_decode_rows(bad, first, count).cpu().numpy(), q[first:first + count])


# ---- through bin/minicom -----------------------------------------------------------------------------------------------------------------
MINICOM = os.path.join(ROOT, "bin", "minicom")
N_READS = 2000
RANGES = [(1, 1), (1, 256), (256, 2), (257, 1744), (2000, 1), (1, 5000)]     # FIRST (from 1) : COUNT
TILING = [(1, 255), (256, 1001), (1257, 5000)]


def _run(args, cwd):
    return subprocess.run([MINICOM] + [str(a) for a in args], cwd=str(cwd), capture_output=True, text=True, timeout=300)


def _synthetic(seed, n=N_READS, L=100):
    """two files of n records: reads of the synthetic genome (a few with N), names, '+' texts and quality lines"""
    from minicom_amd import synth
    reads = synth.synth_reads(seed, 2 * n, L)
    out = []
    for f in range(2):
        recs = rgc.make_records(seed + f, [L] * n, n_rate=0.0)
        rows = reads[f * n:(f + 1) * n].copy()
        rows[::97, 11] = ord("N")
        out.append([(nm if f == 0 else nm + b"/2", rows[i].tobytes(), p, q) for i, (nm, _, p, q) in enumerate(recs)])
    return out


# kind -> (what follows the input on the compression line, the archive)
KINDS = {"QN": (["-p", "-Q", "-N", "-K"], "X_comp_order.minicom"), "p": (["-p"], "X_comp_order.minicom"), "pair_QN": (["-p", "-Q", "-N"], "X_comp_pe_order.minicom"),
         "V": (["-p", "-V", "-Q"], "X_comp_order.minicom"), "q": (["-q"], "X_comp.minicom"), "default": ([], "X_comp.minicom")}


@pytest.fixture(scope="module")
def archives(tmp_path_factory):
    """made on demand, once: kind -> (folder with the input files and the archive made with -G, archive name, the records of both files)"""
    made = {}

    def get(kind):
        if kind not in made:
            flags, arc = KINDS[kind]
            d = tmp_path_factory.mktemp("range_" + kind)
            a, b = _synthetic(71)
            if kind == "V":
                a = [(nm, s[:60], p, q[:60]) if i % 11 == 3 else (nm, s, p, q) for i, (nm, s, p, q) in enumerate(a)]
            (d / "X_1.fastq").write_bytes(rgc.text_of(a)); (d / "X_2.fastq").write_bytes(rgc.text_of(b))
            shutil.copy(d / "X_1.fastq", d / "X.fastq")
            p = _run((["-1", "X_1.fastq", "-2", "X_2.fastq"] if kind == "pair_QN" else ["-r", "X.fastq"]) + flags + ["-G"], d)
            assert p.returncode == 0 and (d / arc).exists(), p.stdout + p.stderr
            made[kind] = (d, arc, (a, b))
        return made[kind]
    return get


def _slice(recs, first1, count, reads_only=False):
    part = recs[first1 - 1:first1 - 1 + count]
    return rgc.reads_only(part) if reads_only else rgc.text_of(part)


def _decode_range(arc, work, first1, count, flags, stems, ext):
    """-d -R in an empty folder: the files it left, by name, which must be exactly the expected ones"""
    work.mkdir()
    p = _run(["-d", arc, "-R", "%d:%d" % (first1, count)] + flags, work)
    assert p.returncode == 0, p.stdout + p.stderr
    names = ["%s.%d-%d.%s%s" % (s, first1, first1 + count - 1, ext, ".gz" if "-z" in flags else "") for s in stems]
    assert sorted(f.name for f in work.iterdir()) == sorted(names), (p.stdout, names)
    out = [(work / f).read_bytes() for f in names]
    return p, [gzip.decompress(b) if "-z" in flags else b for b in out]


E2E = ["QN", "p", "pair_QN"]


def _shape(kind, recs):
    """(the '_dec' stems, the extension, the input files' records, reads only?) of an archive kind"""
    a, b = recs
    pair, reads_only = kind == "pair_QN", kind == "p"
    stems = ["X_comp_pe_order_dec_1", "X_comp_pe_order_dec_2"] if pair else ["X_comp_order_dec"]
    return stems, "reads" if reads_only else "fastq", (a, b) if pair else (a,), reads_only


@pytest.mark.parametrize("first1,count", RANGES, ids=["%d:%d" % r for r in RANGES])
@pytest.mark.parametrize("kind", E2E)
def test_a_range_is_the_slice_of_the_input_on_both_routes(archives, tmp_path, kind, first1, count):
    """-d -G -R: the slice of the input file (of both files of a pair), under the name that carries the range; the -K archive says what a
    range does not check and exits 0.  At a sixteen-lane boundary and on the long tail the host route writes the same files"""
    d, arc, recs = archives(kind)
    stems, ext, files, reads_only = _shape(kind, recs)
    p, got = _decode_range(d / arc, tmp_path / "g", first1, count, ["-G"], stems, ext)
    assert got == [_slice(r, first1, count, reads_only) for r in files]
    assert ("a range is not checked against the digest" in p.stdout) == (kind == "QN")
    if (first1, count) in ((256, 2), (257, 1744)):
        assert _decode_range(d / arc, tmp_path / "h", first1, count, [], stems, ext)[1] == got


@pytest.mark.parametrize("kind", E2E)
def test_a_tiling_concatenates_to_the_input(archives, tmp_path, kind):
    d, arc, recs = archives(kind)
    stems, ext, files, reads_only = _shape(kind, recs)
    parts = [_decode_range(d / arc, tmp_path / ("t%d" % k), f, c, ["-G"], stems, ext)[1] for k, (f, c) in enumerate(TILING)]
    for j, r in enumerate(files):
        assert b"".join(part[j] for part in parts) == (rgc.reads_only(r) if reads_only else rgc.text_of(r))


@pytest.mark.parametrize("kind", E2E)
def test_gz_ranges_and_the_full_decode(archives, tmp_path, kind):
    """-R with -z: files whose gunzipped text is the slice (compressed on the card with -G, by the host twin without); and the full -d of
    the archive is what it was: the input"""
    d, arc, recs = archives(kind)
    stems, ext, files, reads_only = _shape(kind, recs)
    _, got = _decode_range(d / arc, tmp_path / "z", 256, 1001, ["-G", "-z"], stems, ext)
    assert got == [_slice(r, 256, 1001, reads_only) for r in files]
    if kind == "QN":
        _, got = _decode_range(d / arc, tmp_path / "hz", 256, 2, ["-z"], stems, ext)
        assert got == [_slice(r, 256, 2, reads_only) for r in files]
    full = tmp_path / "full"; full.mkdir()
    p = _run(["-d", d / arc, "-G"], full)
    assert p.returncode == 0 and sorted(f.name for f in full.iterdir()) == sorted("%s.%s" % (s, ext) for s in stems), p.stdout + p.stderr
    for s_, r in zip(stems, files):
        assert (full / ("%s.%s" % (s_, ext))).read_bytes() == (rgc.reads_only(r) if reads_only else rgc.text_of(r))


def test_library_routes_agree_on_an_unpacked_archive(archives, tmp_path):
    """pipeline.decompress_range and container.decompress_file(records=) on the GPU and on the host: the same files, the same refusal"""
    from minicom_amd import McomError, container, pipeline
    d, arc, (a, _) = archives("QN")
    n = len(a)
    for first, count in ((0, 1), (255, 2), (1999, 1), (n, 4), (16, n)):
        g, h = tmp_path / "g.fastq", tmp_path / "h.fastq"
        assert container.decompress_file(str(d / arc), str(g), device=0, records=(first, count)) == container.decompress_file(str(d / arc), str(h), records=(first, count)) == max(0, min(count, n - first))
        assert g.read_bytes() == h.read_bytes() == rgc.text_of(a[first:first + count])
        g.unlink(); h.unlink()
    for device in (0, None):
        with pytest.raises(McomError):
            container.decompress_file(str(d / arc), str(tmp_path / "no.fastq"), device=device, records=(n + 1, 1))
        assert not (tmp_path / "no.fastq").exists()


def test_refused_options_and_ranges(archives, tmp_path):
    """-c and -T beside -R, -R 0:5 and -R x: status 1 and a line that says why before the archive is opened; a range behind the last
    record is refused by the decoder; FIRST == n + 1 is an empty file and success"""
    d, arc, _ = archives("QN")
    for k, (extra, word) in enumerate(((["-R", "1:5", "-c", d / "X.fastq"], "-R decompresses a range"), (["-R", "1:5", "-T"], "-R decompresses a range"),
                                       (["-R", "0:5"], "-R takes FIRST:COUNT"), (["-R", "x"], "-R takes FIRST:COUNT"))):
        w = tmp_path / ("a%d" % k); w.mkdir()
        p = _run(["-d", d / arc, "-G"] + extra, w)
        assert p.returncode == 1 and word in p.stdout and not list(w.iterdir()), p.stdout + p.stderr
    w = tmp_path / "behind"; w.mkdir()
    p = _run(["-d", d / arc, "-G", "-R", "2002:1"], w)
    assert p.returncode == 1 and not list(w.iterdir()), p.stdout + p.stderr
    w = tmp_path / "empty"; w.mkdir()
    p = _run(["-d", d / arc, "-G", "-R", "2001:3"], w)
    assert p.returncode == 0 and [f.stat().st_size for f in w.iterdir()] == [0], p.stdout + p.stderr


@pytest.mark.parametrize("kind,word", [("V", "made with -V"), ("q", "made with -q"), ("default", "made without -p")])
def test_refused_archives(archives, tmp_path, kind, word):
    """an archive made with -V, with -q, without -p: status 1, a line that says why, nothing left -- with and without -G"""
    d, arc, _ = archives(kind)
    for flags in (["-G"], []):
        w = tmp_path / ("g" if flags else "h"); w.mkdir()
        p = _run(["-d", d / arc, "-R", "1:5"] + flags, w)
        assert p.returncode == 1 and word in p.stdout and not list(w.iterdir()), p.stdout + p.stderr
