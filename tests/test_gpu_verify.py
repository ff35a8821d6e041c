"""The verifier (csrc/verify.hip under mcomh_verify_gpu): are two tables of reads in HBM the same reads?  The kernels against
collections.Counter and numpy over the same rows; the whole call on the reference's own stream sets against a FASTQ written from the reads
they were made from."""
import collections
import gzip
import io
import os
import shutil
import subprocess
import tarfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACGTN = np.frombuffer(b"ACGTN", dtype=np.uint8)
LS = [1, 15, 16, 17, 100, 150, 255, 256]
NS = [0, 1, 2, 63, 64, 65, 1000, 70001]


@pytest.fixture(scope="module")
def ctx():
    import minicom_amd
    return minicom_amd.Context(0)


# ---- tables -----------------------------------------------------------------------------------------------------------------------------
def _side_a(rows, L):
    """pitch L, as the ingested reads lie"""
    import torch
    n = rows.shape[0]
    return (torch.from_numpy(np.ascontiguousarray(rows).reshape(-1).copy()).cuda() if n else None, L, n)


def _side_b(rows, L, rng, lead=1):
    """pitch L + 1 from an odd byte of a buffer of other bytes, as the decoder's image lies; the byte behind a row is a newline"""
    import torch
    n = rows.shape[0]
    if n == 0:
        return (None, L + 1, 0)
    buf = rng.integers(0, 256, size=lead + n * (L + 1) + 7, dtype=np.uint8)
    img = buf[lead:lead + n * (L + 1)].reshape(n, L + 1)
    img[:, :L] = rows
    img[:, L] = 10
    return (torch.from_numpy(buf).cuda()[lead:], L + 1, n)


def _counts(a, b, ca=None):
    ca, cb = ca if ca is not None else collections.Counter(map(bytes, a)), collections.Counter(map(bytes, b))
    return sum((ca - cb).values()), sum((cb - ca).values()), ca, cb


def _check_multiset(ctx, a, b, L, rng, want=None, mates=None, ca=None):
    """a, b: uint8 [n, L] (paired: mates = (a2, b2), a record is the row and its mate); the report against Counter, and its examples.
    ca: Counter of a's rows, where the caller has it (computed once for all cases of one side a)"""
    ta, tb = _side_a(a, L), _side_b(b, L, rng)
    ka, kb = a, b
    if mates is not None:
        ta, tb = ta + (_side_a(mates[0], L)[0],), tb + (_side_b(mates[1], L, rng, lead=3)[0],)
        ka, kb = np.concatenate([a, mates[0]], axis=1), np.concatenate([b, mates[1]], axis=1)
    r = ctx.verify_multiset(ta, tb, L)
    missing, extra, ca, cb = _counts(ka, kb, ca)
    assert (r["n_a"], r["n_b"]) == (a.shape[0], b.shape[0])
    assert (r["missing"], r["extra"]) == (missing, extra), (r, missing, extra)
    assert r["identical"] == (missing == 0 and extra == 0)
    if want is not None:
        assert (missing, extra) == want
    for key, rows, more, n_want in (("missing_examples", ka, ca - cb, missing), ("extra_examples", kb, cb - ca, extra)):
        ex = r[key]
        assert len(ex) == min(8, n_want) and ex == sorted(set(ex)), r
        for i in ex:
            assert more[bytes(rows[i])] > 0, (key, i)
    return r


def _pool_rows(rng, n, L):
    """about 50 distinct strings, so that duplicates dominate, and a few unique rows"""
    pool = ACGTN[rng.integers(0, 5, size=(50, L))]
    rows = pool[rng.integers(0, 50, size=n)]
    for i in rng.choice(n, size=min(n, 3), replace=False) if n else []:
        rows[i] = ACGTN[rng.integers(0, 5, size=L)]
    return rows


def _other(c):
    return ACGTN[(int(np.flatnonzero(ACGTN == c)[0]) + 1) % 5]


def _cases(rng, a, L):
    """(name, side b, (missing, extra) the case is built to give -- None where the rows decide) for side a"""
    n = a.shape[0]
    out = [("permuted", a[rng.permutation(n)], (0, 0)), ("empty b", a[:0], (n, 0)), ("empty a", None, (0, n))]
    if n == 0:
        return out + [("added to nothing", ACGTN[rng.integers(0, 5, size=(5, L))], (0, 5))]
    for row, col in ((0, 0), (0, L - 1), (n - 1, 0), (n - 1, L - 1)):
        b = a.copy()
        b[row, col] = _other(b[row, col])
        out.append(("character %d of row %d changed" % (col, row), b[rng.permutation(n)], (1, 1)))
    keys = [bytes(r) for r in a]
    cnt = collections.Counter(keys)
    dup = next((i for i, k in enumerate(keys) if cnt[k] >= 2), None)
    if dup is not None and len(cnt) >= 2:
        src = next(i for i, k in enumerate(keys) if k != keys[dup])
        b = a.copy()
        b[dup] = a[src]
        out.append(("a copy replaced by a copy of another row", b[rng.permutation(n)], (1, 1)))           # the sets of rows are equal
    drop = int(rng.integers(0, n))
    out.append(("row dropped", np.delete(a, drop, axis=0)[rng.permutation(n - 1)], (1, 0)))
    out.append(("row added", np.concatenate([a, a[drop:drop + 1]])[rng.permutation(n + 1)], (0, 1)))
    return out


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("L", LS)
def test_multiset_against_counter(ctx, L, n):
    rng = np.random.default_rng(1000 * L + n)
    a = _pool_rows(rng, n, L)
    ca = collections.Counter(map(bytes, a))
    for name, b, want in _cases(rng, a, L):
        if b is None:                                        # side a empty: everything of b is extra
            r = _check_multiset(ctx, a[:0], a, L, rng, want)
        else:
            r = _check_multiset(ctx, a, b, L, rng, want, ca=ca)
        assert r["exact_runs"] == 0, name                    # 64 bits of hash: no run of unequal records


@pytest.mark.parametrize("bits", [2, 0])
def test_truncated_hashes_walk_the_collision_path(ctx, bits):
    """a thousand distinct rows under hashes of 2 and of 0 bits: every run holds unequal records; the same verdicts and counts"""
    L, n = 100, 1000
    rng = np.random.default_rng(bits)
    a = ACGTN[rng.integers(0, 5, size=(n, L))]
    assert len(set(map(bytes, a))) == n
    ctx.set_verify_hash_bits(bits)
    try:
        for name, b, want in _cases(rng, a, L):
            if b is None:
                _check_multiset(ctx, a[:0], a, L, rng, want)
                continue
            r = _check_multiset(ctx, a, b, L, rng, want)
            if b.shape[0]:
                assert r["exact_runs"] > 0, name
                assert r["exact_runs"] <= (1 << bits), name
        b = np.concatenate([a[:500], a[:500]])               # duplicates among the collisions
        r = _check_multiset(ctx, a, b[rng.permutation(n)], L, rng, (500, 500))
        assert r["exact_runs"] > 0
    finally:
        ctx.set_verify_hash_bits(64)
    assert _check_multiset(ctx, a, a[rng.permutation(n)], L, rng, (0, 0))["exact_runs"] == 0


@pytest.mark.parametrize("L", [17, 150])
def test_pairs(ctx, L):
    rng = np.random.default_rng(L)
    n = 1000
    a1, a2 = _pool_rows(rng, n, L), _pool_rows(rng, n, L)
    p = rng.permutation(n)
    _check_multiset(ctx, a1, a1[p], L, rng, (0, 0), mates=(a2, a2[p]))
    # the mates of two pairs exchanged: the single rows are the same multisets, the pairs are not
    i, j = next((i, j) for i in range(n) for j in range(i + 1, n) if len({bytes(a1[i]), bytes(a1[j]), bytes(a2[i]), bytes(a2[j])}) == 4)
    b2 = a2.copy()
    b2[[i, j]] = a2[[j, i]]
    assert _counts(np.concatenate([a1, a2]), np.concatenate([a1, b2]))[:2] == (0, 0)
    _check_multiset(ctx, a1, a1[p], L, rng, (2, 2), mates=(a2, b2[p]))
    # one pair with its rows swapped between the files
    b1, b2 = a1.copy(), a2.copy()
    b1[i], b2[i] = a2[i], a1[i]
    _check_multiset(ctx, a1, b1[p], L, rng, (1, 1), mates=(a2, b2[p]))
    _check_multiset(ctx, a1[:0], a1, L, rng, (0, n), mates=(a2[:0], a2))
    # the ordered form takes pairs too
    r = ctx.verify_ordered(_side_a(a1, L) + (_side_a(a2, L)[0],), _side_b(a1, L, rng) + (_side_b(b2, L, rng, lead=5)[0],), L)
    assert (r["identical"], r["differing"], r["first_diff"]) == (False, 1, i)


@pytest.mark.parametrize("n", [1, 65, 1000, 70001])
@pytest.mark.parametrize("L", LS)
def test_ordered_against_numpy(ctx, L, n):
    rng = np.random.default_rng(77 * L + n)
    a = _pool_rows(rng, n, L)
    r = ctx.verify_ordered(_side_a(a, L), _side_b(a, L, rng), L)
    assert (r["identical"], r["differing"], r["first_diff"], r["n_a"], r["n_b"]) == (True, 0, None, n, n)
    b = a[rng.permutation(n)]
    diff = np.flatnonzero((a != b).any(axis=1))
    r = ctx.verify_ordered(_side_a(a, L), _side_b(b, L, rng), L)
    assert r["identical"] == (diff.size == 0) and r["differing"] == diff.size and r["first_diff"] == (int(diff[0]) if diff.size else None)
    for row, col in ((0, 0), (n - 1, L - 1)):
        b = a.copy()
        b[row, col] = _other(b[row, col])
        r = ctx.verify_ordered(_side_a(a, L), _side_b(b, L, rng), L)
        assert (r["identical"], r["differing"], r["first_diff"]) == (False, 1, row)
    # unequal counts: different, whatever the common rows say
    r = ctx.verify_ordered(_side_a(a, L), _side_b(a[:n - 1], L, rng), L)
    assert (r["identical"], r["differing"], r["n_a"], r["n_b"]) == (False, 0, n, n - 1)
    r = ctx.verify_ordered(_side_a(a[:0], L), _side_b(a, L, rng), L)
    assert (r["identical"], r["differing"]) == (False, 0)


def test_empty_tables_and_bad_arguments(ctx):
    from minicom_amd.hip import McomError
    rng = np.random.default_rng(1)
    a = _pool_rows(rng, 10, 20)
    for f in (ctx.verify_multiset, ctx.verify_ordered):
        r = f((None, 20, 0), (None, 21, 0), 20)
        assert r["identical"] and (r["n_a"], r["n_b"], r["missing"], r["extra"], r["differing"]) == (0, 0, 0, 0, 0)
        for L in (0, 257):
            with pytest.raises(McomError):
                f(_side_a(a, 20), _side_b(a, 20, rng), L)
        with pytest.raises(McomError):
            f((_side_a(a, 20)[0], 19, 10), _side_b(a, 20, rng), 20)                            # a pitch below L
        with pytest.raises(McomError):
            f(_side_a(a, 20) + (_side_a(a, 20)[0],), _side_b(a, 20, rng), 20)                  # one side paired, the other not


def test_two_calls_give_the_same_report(ctx):
    L, n = 150, 70001
    rng = np.random.default_rng(5)
    a = _pool_rows(rng, n, L)
    b = a[rng.permutation(n)].copy()
    b[rng.choice(n, size=300, replace=False)] = ACGTN[rng.integers(0, 5, size=(300, L))]
    ta, tb = _side_a(a, L), _side_b(b, L, rng)
    first = ctx.verify_multiset(ta, tb, L)
    assert first["missing"] == 300 and len(first["missing_examples"]) == 8 and len(first["extra_examples"]) == 8
    for _ in range(2):
        assert ctx.verify_multiset(ta, tb, L) == first
    ctx.set_verify_hash_bits(3)
    try:
        narrow = ctx.verify_multiset(ta, tb, L)
        assert narrow == ctx.verify_multiset(ta, tb, L)
        assert narrow["exact_runs"] > 0 and {k: v for k, v in narrow.items() if k != "exact_runs"} == {k: v for k, v in first.items() if k != "exact_runs"}
    finally:
        ctx.set_verify_hash_bits(64)
    assert ctx.verify_ordered(ta, tb, L) == ctx.verify_ordered(ta, tb, L)


# ---- the whole call on the reference's own stream sets ----------------------------------------------------------------------------------
MODES = ["default", "order", "paired"]
_GOLDEN = os.path.join(ROOT, "tests", "golden")


def _fixture_name(mode, L):
    return "streams_%sstages_L%d.tar.gz" % ({"default": "", "order": "order_", "paired": "pe_"}[mode], L)


FIXTURES = [(mode, L) for mode in MODES for L in (40, 100, 150) if os.path.exists(os.path.join(_GOLDEN, _fixture_name(mode, L)))]


def _untar(name, d):
    d.mkdir()
    with gzip.open(os.path.join(_GOLDEN, name), "rb") as g:
        tf = tarfile.open(fileobj=io.BytesIO(g.read()))
        for m in tf.getmembers():
            (d / m.name).write_bytes(tf.extractfile(m).read())


def _golden_reads(L):
    with gzip.open(os.path.join(_GOLDEN, "stages_L%d.reads.gz" % L), "rb") as f:
        return f.read().split(b"\n")[:-1]


def _write_fastq(path, rows):
    with open(path, "wb") as f:
        for i, r in enumerate(rows):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))
    return str(path)


def _fastqs(tmp_path, mode, rows, tag):
    """the FASTQ file(s) of one mode from a list of reads: paired end cuts the list in two halves, as the fixture was made"""
    if mode != "paired":
        return [_write_fastq(tmp_path / (tag + ".fastq"), rows)]
    half = len(rows) // 2
    return [_write_fastq(tmp_path / (tag + "_1.fastq"), rows[:half]), _write_fastq(tmp_path / (tag + "_2.fastq"), rows[half:2 * half])]


def _verify(d, mode, files):
    from minicom_amd.pipeline import verify
    return verify(str(d), files[0], files[1] if mode == "paired" else None, order=mode == "order", device=0)


def _changed(rows, at):
    r = bytearray(rows[at])
    r[len(r) // 2] = ord("C") if r[len(r) // 2] != ord("C") else ord("G")
    return rows[:at] + [bytes(r)] + rows[at + 1:]


@pytest.mark.parametrize("mode,L", FIXTURES)
def test_reference_streams_against_their_fastq(tmp_path, mode, L):
    d = tmp_path / "s"
    _untar(_fixture_name(mode, L), d)
    rows = _golden_reads(L)
    units = len(rows) // 2 if mode == "paired" else len(rows)
    r = _verify(d, mode, _fastqs(tmp_path, mode, rows, "same"))
    assert r["identical"] and (r["n_input"], r["n_archive"], r["missing"], r["extra"], r["differing"], r["exact_runs"]) == (units, units, 0, 0, 0, 0), r
    assert r["mode"] == mode and r["times_ms"]["total"] >= r["times_ms"]["compare"] > 0
    # the reads in another order: the same multiset, other lines
    back = rows[::-1] if mode != "paired" else rows[:units][::-1] + rows[units:2 * units][::-1]
    r = _verify(d, mode, _fastqs(tmp_path, mode, back, "reversed"))
    if mode == "order":
        want = sum(1 for x, y in zip(rows, back) if x != y)
        assert want > 0 and not r["identical"] and r["differing"] == want and r["first_diff"] == next(i for i, (x, y) in enumerate(zip(rows, back)) if x != y)
    else:
        assert r["identical"], r
    # one base changed
    at = units // 3
    r = _verify(d, mode, _fastqs(tmp_path, mode, _changed(rows, at), "changed"))
    assert not r["identical"] and (r["n_input"], r["n_archive"]) == (units, units)
    if mode == "order":
        assert (r["differing"], r["first_diff"]) == (1, at)
    else:
        assert (r["missing"], r["extra"], len(r["extra_examples"])) == (1, 1, 1) and r["missing_examples"] == [at], r
    # one read (pair) removed: a verdict, not an error
    less = rows[:at] + rows[at + 1:] if mode != "paired" else rows[:at] + rows[at + 1:units] + rows[units:units + at] + rows[units + at + 1:2 * units]
    r = _verify(d, mode, _fastqs(tmp_path, mode, less, "less"))
    assert not r["identical"] and (r["n_input"], r["n_archive"]) == (units - 1, units), r
    if mode != "order":
        assert (r["missing"], r["extra"]) == (0, 1)


def test_altered_archive_is_a_verdict_and_a_refused_one_an_error(tmp_path):
    from minicom_amd.hip import McomError
    from minicom_amd.pipeline import Pipeline
    L, n = 100, 300
    rng = np.random.default_rng(9)
    reads = ACGTN[rng.integers(0, 4, size=(n, L))]           # random reads: every one unclustered
    d = tmp_path / "s"; d.mkdir()
    p = Pipeline(np.ascontiguousarray(reads), host_threads=2); p.pre_process()
    try:
        p.cluster_dump(str(d))
    finally:
        p.close()
    assert (d / "beg_pos.bin.0").stat().st_size == 0 and (d / "single.seq").stat().st_size == n * L // 4
    fq = [_write_fastq(tmp_path / "r.fastq", [bytes(r) for r in reads])]
    assert _verify(d, "default", fq)["identical"]
    b = bytearray((d / "single.seq").read_bytes())
    b[len(b) // 2] ^= 0b00010001                             # two bits of one byte: two bases of one read (L / 4 bytes per read)
    (d / "single.seq").write_bytes(bytes(b))
    r = _verify(d, "default", fq)
    assert not r["identical"] and (r["missing"], r["extra"], r["n_input"], r["n_archive"]) == (1, 1, n, n), r
    # another read length: an error
    with pytest.raises(McomError):
        _verify(d, "default", [_write_fastq(tmp_path / "short.fastq", [bytes(r[:L - 1]) for r in reads])])
    # an archive the decoders refuse: an error, not a verdict
    g = tmp_path / "g"
    _untar(_fixture_name("default", 100), g)
    rows = _golden_reads(100)
    fq = [_write_fastq(tmp_path / "g.fastq", rows)]
    assert _verify(g, "default", fq)["identical"]
    ref = (g / "ref.bin.0").read_bytes()
    (g / "ref.bin.0").write_bytes(ref[:len(ref) // 2])
    with pytest.raises(McomError):
        _verify(g, "default", fq)
    from minicom_amd.pipeline import decompress
    with pytest.raises(McomError):
        decompress(str(g), str(tmp_path / "g.out"), device=0)


@pytest.mark.parametrize("mode", ["default", "paired"])
def test_container_and_command_line(tmp_path, mode):
    from minicom_amd import container
    L = 100
    d = tmp_path / "s"
    _untar(_fixture_name(mode, L), d)
    rows = _golden_reads(L)
    units = len(rows) // 2 if mode == "paired" else len(rows)
    work = tmp_path / "work"; work.mkdir()
    arch = str(work / "x.minicom")
    container.pack(str(d), arch, codec="rans", device=0)
    good, bad = _fastqs(tmp_path, mode, rows, "good"), _fastqs(tmp_path, mode, _changed(rows, 7), "bad")
    r = container.verify_file(arch, *good, device=0)
    assert r["identical"] and r["mode"] == mode and r["n_input"] == units
    assert not container.verify_file(arch, *bad, device=0)["identical"]
    script = os.path.join(ROOT, "bin", "minicom")
    for files, status, word in ((good, 0, "verified: %d %s identical" % (units, "pairs" if mode == "paired" else "reads")), (bad, 2, "DIFFERENT")):
        argv = [script, "-d", arch, "-c", files[0]] + (["-C", files[1]] if mode == "paired" else [])
        q = subprocess.run(argv, capture_output=True, text=True, cwd=str(work))
        assert q.returncode == status and word in q.stdout, (q.returncode, q.stdout, q.stderr)
        assert sorted(os.listdir(work)) == ["x.minicom"], os.listdir(work)                       # no _dec.reads, no working directory
    shutil.rmtree(work)
