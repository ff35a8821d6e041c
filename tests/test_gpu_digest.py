"""Self-checking archives on the GPU (csrc/digest.hip, host/mcom_digest.cpp): each device call against the
definition in plain Python (tests/digest_reference.py) element for element with canaries around the arrays, the file call against the
host twin's bytes at the minimum piece size and on every file form, and `bin/minicom -K` / `-d` / `-d -T` end to end in every mode."""
import gzip
import os
import shutil
import subprocess
import tarfile

import numpy as np
import pytest

import digest_reference as dr
import ragged_cases as rc

pytestmark = pytest.mark.gpu
CANARY = 0x5A5A5A5A5A5A5A5A
CASES = dr.cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_PIECE = 1          # raised to the documented minimum of 2304 bytes: records straddle pieces


@pytest.fixture(scope="module")
def ctx():
    import minicom_amd
    return minicom_amd.Context(0)


def _dev(b, offset=0):
    """the bytes on the device, `offset` bytes into a fresh buffer (an odd address for offset 1 or 3)"""
    import torch
    buf = torch.full((offset + len(b) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    if len(b):
        buf[offset:offset + len(b)] = torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()
    return buf[offset:offset + len(b)]


def _arrays(n, k=3):
    """k hash arrays of n rows, each the middle of a buffer of canaries"""
    import torch
    bufs = [torch.full((n + 4, 2), CANARY, dtype=torch.int64, device="cuda") for _ in range(k)]
    return bufs, [b[2:2 + n] for b in bufs]


def _u64(t):
    return [tuple(int(v) for v in row) for row in t.cpu().numpy().view(np.uint64)]


def _canaries_intact(bufs, n):
    return all(_u64(b[:2]) + _u64(b[2 + n:]) == [(CANARY, CANARY)] * 4 for b in bufs)


@pytest.mark.parametrize("name,recs", CASES, ids=dr.case_ids())
def test_record_hashes_against_the_reference(ctx, name, recs):
    """pieces of seven records from odd addresses into arrays that cover all records: every word, and nothing outside the arrays"""
    n = len(recs)
    want = [dr.record_hashes(r) for r in recs]
    bufs, (hS, hQ, hN) = _arrays(n)
    step = 7 if n < 100 else 1499
    for k, first in enumerate(range(0, n, step)):
        _, _, _, bits, bad = ctx.fastq_record_hashes(_dev(rc.text_of(recs[first:first + step]), offset=(1, 3, 2, 0)[k % 4]), first_record=first, hS=hS, hQ=hQ, hN=hN)
        assert (bits, bad) == (0, None)
    assert _u64(hS) == [w[0] for w in want] and _u64(hQ) == [w[1] for w in want] and _u64(hN) == [w[2] for w in want]
    assert _canaries_intact(bufs, n)
    assert ctx.digest_reduce(hS, hQ, hN) == dr.sums16(dr.sums(recs))
    # one read per line: the sequence hashes alone; the other arrays are not touched
    bufs, (rS, rQ, rN) = _arrays(n)
    _, _, _, bits, _ = ctx.fastq_record_hashes(_dev(rc.reads_only(recs), offset=1), lines_per_record=1, hS=rS, hQ=rQ, hN=rN)
    assert bits == 0 and _u64(rS) == [w[0] for w in want] and _u64(rQ) == _u64(rN) == [(CANARY, CANARY)] * n and _canaries_intact(bufs, n)
    # without the quality and name arrays
    sS, sQ, sN, bits, _ = ctx.fastq_record_hashes(_dev(rc.text_of(recs)), with_qual=False, with_names=False)
    assert bits == 0 and sQ is None and sN is None and _u64(sS) == [w[0] for w in want]


@pytest.mark.parametrize("name,text,first_bad,bits", dr.bad_records(), ids=[c[0] for c in dr.bad_records()])
def test_bad_records_are_flagged_and_get_no_hash(ctx, name, text, first_bad, bits):
    from minicom_amd import pipeline
    bufs, (hS, hQ, hN) = _arrays(6)
    _, _, _, got_bits, first = ctx.fastq_record_hashes(_dev(text, offset=3), hS=hS, hQ=hQ, hN=hN)
    assert (got_bits, first) == (bits, first_bad - 1)
    tS, tQ, tN, _, _ = pipeline.fastq_record_hashes_host(text)
    for got, twin in ((hS, tS), (hQ, tQ), (hN, tN)):
        rows = _u64(got)
        assert rows[first_bad - 1] == (CANARY, CANARY)
        assert [r for k, r in enumerate(rows) if k != first_bad - 1] == [tuple(int(v) for v in r) for k, r in enumerate(twin) if k != first_bad - 1]
    assert _canaries_intact(bufs, 6)


def test_text_of_lines_that_are_no_records(ctx):
    """empty lines, a text without a newline at its end (the tail belongs to no line): flagged or ignored, nothing written"""
    bufs, (hS, hQ, hN) = _arrays(3)
    _, _, _, bits, first = ctx.fastq_record_hashes(_dev(b"\n\n\n\n@a\nAC\n+\nII\n@b\nACG\n+\nII", offset=1), hS=hS, hQ=hQ, hN=hN)     # the third record has no end: two records
    assert (bits, first) == (dr.F_NAME | dr.F_PLUS | dr.F_LENGTH, 0)
    assert _u64(hS)[0] == (CANARY, CANARY) and _u64(hS)[1] == dr.H(b"AC") and _u64(hS)[2] == (CANARY, CANARY) and _canaries_intact(bufs, 3)
    _, _, _, bits, first = ctx.fastq_record_hashes(_dev(b"ACGT\n\n" + b"A" * 257 + b"\nA\n", offset=3), lines_per_record=1, first_record=0, hS=_arrays(4)[1][0])
    assert (bits, first) == (dr.F_LENGTH, 1)


def _reduce_reference(arrs, n):
    """the sixteen sums from raw hash arrays (None: absent), by the definition"""
    S1, Q1, N1, S2, Q2, N2 = [None if a is None else [tuple(int(v) for v in r) for r in a[:n]] for a in arrs]
    out = {"seq.ordered.1": dr.ordered(S1)}
    if Q1 is not None:
        out["qual.ordered.1"] = dr.ordered(Q1)
    if N1 is not None:
        out["name.ordered.1"] = dr.ordered(N1)
    if S2 is None:
        out["seq.multiset"] = dr.multiset(S1)
        if Q1 is not None:
            out["rec.multiset"] = dr.multiset([dr.C(s, q) for s, q in zip(S1, Q1)])
    else:
        out["seq.ordered.2"] = dr.ordered(S2)
        out["seq.multiset"] = dr.multiset([dr.C(a, b) for a, b in zip(S1, S2)])
        if Q1 is not None:
            out["qual.ordered.2"] = dr.ordered(Q2)
            out["rec.multiset"] = dr.multiset([dr.C(dr.C(a, p), dr.C(b, q)) for a, p, b, q in zip(S1, Q1, S2, Q2)])
        if N1 is not None:
            out["name.ordered.2"] = dr.ordered(N2)
    return dr.sums16(out)


@pytest.mark.parametrize("n", [1, 255, 256, 257, dr.REDUCE_BLOCK, dr.REDUCE_BLOCK + 1])
def test_reduce_against_the_reference(ctx, n):
    """one record, the counts around a wave and a workgroup's threads, a whole workgroup and one record more; one file and a pair, with and
    without the quality and name arrays; rows behind n do not count"""
    import torch
    from minicom_amd import pipeline
    rng = np.random.default_rng(n)
    host = [rng.integers(0, 1 << 64, size=(n + 3, 2), dtype=np.uint64) for _ in range(6)]
    dev = [torch.from_numpy(a.view(np.int64).copy()).cuda() for a in host]
    for use in ((0,), (0, 1), (0, 2), (0, 1, 2), (0, 3), (0, 1, 3, 4), (0, 2, 3, 5), (0, 1, 2, 3, 4, 5)):
        pick = lambda arrs: [a if k in use else None for k, a in enumerate(arrs)]  # noqa: E731
        want = _reduce_reference(pick(host), n)
        assert ctx.digest_reduce(*pick(dev), n=n) == want, use
        assert pipeline.digest_reduce_host(*[None if a is None else a[:n] for a in pick(host)]) == want, use
    from minicom_amd import McomError
    with pytest.raises(McomError):
        ctx.digest_reduce(dev[0], dev[1], None, dev[3], None, None, n=n)               # the second file without the first one's arrays


# ---- the file call ----
@pytest.mark.parametrize("name,recs", CASES, ids=dr.case_ids())
def test_file_call_gives_the_twins_bytes_at_the_minimum_piece(tmp_path, name, recs):
    from minicom_amd import pipeline
    mate = dr.mate_of(recs)
    fq, fq2, rd = tmp_path / "in_1.fastq", tmp_path / "in_2.fastq", tmp_path / "in.reads"
    fq.write_bytes(rc.text_of(recs))
    fq2.write_bytes(rc.text_of(mate))
    rd.write_bytes(rc.reads_only(recs))
    for args, kw, want in (((str(fq),), {}, dr.digest_text(recs)), ((str(fq), str(fq2)), {}, dr.digest_text(recs, mate)), ((str(fq),), {"with_qual": False}, dr.digest_text(recs, with_qual=False)),
                           ((str(rd),), {"lines_per_record": 1}, dr.digest_text(recs, with_qual=False, with_names=False))):
        got = pipeline.fastq_digest(*args, device=0, piece_bytes=MIN_PIECE, **kw)
        assert got == pipeline.fastq_digest(*args, **kw) == want


@pytest.mark.parametrize("form", ["no_final_newline", "gz_one_member", "gz_five_members", "bgzf"])
@pytest.mark.parametrize("name", ["line_lengths", "n_17", "n_5000"])
def test_file_forms_on_the_gpu(tmp_path, name, form):
    """a missing last newline, gzip files of one and of several members (zlib's reader), and a BGZF file, which is inflated on the card"""
    from minicom_amd import pipeline
    recs = dict(CASES)[name]
    text = rc.text_of(recs, final_newline=form != "no_final_newline")
    fq = tmp_path / ("in.fastq" if form == "no_final_newline" else "in.fastq.gz")
    if form == "bgzf":
        (tmp_path / "plain").write_bytes(text)
        assert subprocess.run([os.path.join(ROOT, "bin", "mcomz"), "z", str(tmp_path / "plain"), str(fq)]).returncode == 0
    else:
        fq.write_bytes(text if form == "no_final_newline" else rc.gz_members(text, 1 if form == "gz_one_member" else 5))
    assert pipeline.fastq_digest(str(fq), device=0, piece_bytes=MIN_PIECE if form != "bgzf" else 70000) == dr.digest_text(recs)


@pytest.mark.parametrize("name,text,first_bad,bits", dr.bad_records(), ids=[c[0] for c in dr.bad_records()])
def test_file_call_refuses_with_the_host_twins_message(tmp_path, name, text, first_bad, bits):
    from minicom_amd import McomError, pipeline
    fq = tmp_path / "bad.fastq"
    fq.write_bytes(rc.text_of(rc.make_records(3, [100] * 40)) + text)          # a few pieces in front of the bad record
    msgs = []
    for device in (None, 0):
        with pytest.raises(McomError, match=r"record %d is not" % (40 + first_bad)) as e:
            pipeline.fastq_digest(str(fq), device=device, piece_bytes=MIN_PIECE, out_path=str(tmp_path / "digest.txt"))
        assert not (tmp_path / "digest.txt").exists()
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]


def test_file_call_refuses_a_cut_file_and_a_pair_of_different_counts(tmp_path):
    from minicom_amd import McomError, pipeline
    recs = dict(CASES)["n_17"]
    t = rc.text_of(recs)
    (tmp_path / "a.fastq").write_bytes(t)
    (tmp_path / "b.fastq").write_bytes(rc.text_of(recs[:-1]))
    (tmp_path / "cut.fastq").write_bytes(t[:t.rindex(b"\n+")])
    out = tmp_path / "digest.txt"
    with pytest.raises(McomError, match="different numbers of records: 17 and 16"):
        pipeline.fastq_digest(str(tmp_path / "a.fastq"), str(tmp_path / "b.fastq"), device=0, piece_bytes=MIN_PIECE, out_path=str(out))
    with pytest.raises(McomError, match="ends inside record 17"):
        pipeline.fastq_digest(str(tmp_path / "cut.fastq"), device=0, piece_bytes=MIN_PIECE, out_path=str(out))
    assert not out.exists()


# ---- through bin/minicom ----
MINICOM = os.path.join(ROOT, "bin", "minicom")
N_READS = 2000


def _run(args, cwd):
    return subprocess.run([MINICOM] + [str(a) for a in args], cwd=str(cwd), capture_output=True, text=True, timeout=300)


def _synthetic(seed, n=N_READS, L=100):
    """two files of n reads of L bases from the synthetic genome with names, '+' texts and quality lines; a few reads with N"""
    from minicom_amd import synth
    reads = synth.synth_reads(seed, 2 * n, L)
    out = []
    for f in range(2):
        recs = rc.make_records(seed + f, [L] * n, n_rate=0.0)
        rows = reads[f * n:(f + 1) * n].copy()
        rows[::97, 11] = ord("N")
        out.append([(nm if f == 0 else nm + b"/2", rows[i].tobytes(), p, q) for i, (nm, _, p, q) in enumerate(recs)])
    return out


def _ragged(recs, seed):
    """about one record in ten trimmed to 30 .. 99 bases"""
    import random
    rng = random.Random(seed)
    out = []
    for nm, s, p, q in recs:
        l = len(s) if rng.random() >= 0.1 else rng.randrange(30, len(s))
        out.append((nm, s[:l], p, q[:l]))
    return out


# mode -> (compression flags behind the input, archive, what -d says was compared, the unit, pair?, ragged?)
MODES = {
    "default": ([], "X_comp.minicom", "reads, in any order,", "records", False, False),
    "order_QN": (["-p", "-Q", "-N"], "X_comp_order.minicom", "reads, quality lines and names", "records", False, False),
    "ragged_QN": (["-p", "-V", "-Q", "-N"], "X_comp_order.minicom", "reads, quality lines and names", "records", False, True),
    "own_order_q": (["-q"], "X_comp.minicom", "reads with their quality lines, in any order,", "records", False, False),
    "pair": ([], "X_comp_pe.minicom", "reads, in any order,", "pairs", True, False),
    "pair_order_QN": (["-p", "-Q", "-N"], "X_comp_pe_order.minicom", "reads, quality lines and names", "pairs", True, False),
    "lossy_ill8": (["-p", "-Q", "-b", "ill8"], "X_comp_order.minicom", "reads", "records", False, False),
}


@pytest.fixture(scope="module")
def archives(tmp_path_factory):
    """made on demand, once: mode -> (folder with the input and the archive made with -K -G, archive name)"""
    made = {}

    def get(mode, digest=True):
        key = (mode, digest)
        if key not in made:
            flags, arc, _, _, pair, ragged = MODES[mode]
            d = tmp_path_factory.mktemp("digest_" + mode)
            a, b = _synthetic(61)
            if ragged:
                a = _ragged(a, 62)
            (d / "X_1.fastq").write_bytes(rc.text_of(a))
            (d / "X_2.fastq").write_bytes(rc.text_of(b))
            shutil.copy(d / "X_1.fastq", d / "X.fastq")
            p = _run((["-1", "X_1.fastq", "-2", "X_2.fastq"] if pair else ["-r", "X.fastq"]) + flags + ["-G"] + (["-K"] if digest else []), d)
            assert p.returncode == 0 and (d / arc).exists(), p.stdout + p.stderr
            made[key] = (d, arc)
        return made[key]
    return get


def _said(p, what, unit):
    return "verified: %s identical to the compressed input of %d %s\n" % (what, N_READS, unit) in p.stdout


@pytest.mark.parametrize("flags", [["-G"], [], ["-G", "-z"]], ids=["gpu", "host", "gpu_gz"])
@pytest.mark.parametrize("mode", list(MODES))
def test_decode_checks_itself(archives, tmp_path, mode, flags):
    """-d of an archive made with -K: status 0, one line that names what was compared, the files written as ever"""
    d, arc = archives(mode)
    _, _, what, unit, pair, _ = MODES[mode]
    p = _run(["-d", d / arc] + flags, tmp_path)
    assert p.returncode == 0 and _said(p, what, unit), p.stdout + p.stderr
    assert ("the quality values were not checked" in p.stdout) == (mode == "lossy_ill8")
    outs = sorted(f.name for f in tmp_path.iterdir())
    assert len(outs) == (2 if pair else 1) and all(("_dec" in f) and f.endswith(".gz") == ("-z" in flags) for f in outs), outs
    if mode in ("order_QN", "ragged_QN", "pair_order_QN"):
        for k, f in enumerate(outs):
            got = (tmp_path / f).read_bytes()
            assert (gzip.decompress(got) if "-z" in flags else got) == (d / ("X_%d.fastq" % (k + 1))).read_bytes()


def _repack(src, dst, work, change):
    """the archive with its digest.txt sent through `change`"""
    work.mkdir()
    with tarfile.open(src) as t:
        t.extractall(work)
    f = work / "digest.txt"
    f.write_text(change(f.read_text()))
    with tarfile.open(dst, "w") as t:
        for name in sorted(os.listdir(work)):
            t.add(work / name, arcname="./" + name)


def _one_digit(text, key="qual.ordered.1 "):
    at = text.index(key) + len(key) + 5
    return text[:at] + ("0" if text[at] != "0" else "1") + text[at + 1:]


def _other_digest(tmp_path):
    """the digest of another input of as many records"""
    from minicom_amd import pipeline
    other = _synthetic(71)[0]
    (tmp_path / "other.fastq").write_bytes(rc.text_of(other))
    return pipeline.fastq_digest(str(tmp_path / "other.fastq"), device=0)


@pytest.mark.parametrize("damage", ["one_digit", "another_input", "another_count", "no_last_newline"])
def test_damaged_digest_is_said(archives, tmp_path, damage):
    """one digit of digest.txt changed, the digest of another input put in, another record count: status 2, the part named, the file kept;
    a digest.txt that does not parse: status 1"""
    d, arc = archives("order_QN")
    change = {"one_digit": _one_digit, "another_input": lambda t: _other_digest(tmp_path), "another_count": lambda t: t.replace("n %d\n" % N_READS, "n %d\n" % (N_READS + 1)),
              "no_last_newline": lambda t: t[:-1]}[damage]
    _repack(d / arc, tmp_path / "bad.minicom", tmp_path / "w", change)
    p = _run(["-d", tmp_path / "bad.minicom", "-G"], tmp_path)
    if damage == "no_last_newline":
        assert p.returncode == 1 and "not a digest" in p.stderr, p.stdout + p.stderr
        return
    said = {"one_digit": "the quality lines differ (first: quality lines)", "another_input": "the reads, quality lines, names differ (first: reads)",
            "another_count": "held %d records, the decompressed output holds %d" % (N_READS + 1, N_READS)}[damage]
    assert p.returncode == 2 and "DIFFERENT" in p.stdout and said in p.stdout and "they were kept: bad_dec.fastq" in p.stdout, p.stdout + p.stderr
    assert (tmp_path / "bad_dec.fastq").read_bytes() == (d / "X.fastq").read_bytes()


@pytest.mark.parametrize("mode,case", [("order_QN", "good"), ("order_QN", "good_host"), ("order_QN", "damaged"), ("order_QN", "no_digest"), ("pair", "good"), ("pair", "damaged"), ("default", "good")])
def test_T_tests_the_archive_and_leaves_nothing_behind(archives, tmp_path, mode, case):
    """-d X.minicom -T: status 0 for the archive as made, 2 for a damaged digest, 1 without digest.txt; the folder holds what it held"""
    d, arc = archives(mode, digest=case != "no_digest")
    _, _, what, unit, _, _ = MODES[mode]
    (tmp_path / "cwd").mkdir()
    if case == "damaged":
        _repack(d / arc, tmp_path / "X.minicom", tmp_path / "cwd" / "w", lambda t: _one_digit(t, "seq.ordered.1 " if "order" in mode else "seq.multiset "))
        shutil.rmtree(tmp_path / "cwd" / "w")
    else:
        shutil.copy(d / arc, tmp_path / "X.minicom")
    p = _run(["-d", tmp_path / "X.minicom", "-T"] + ([] if case == "good_host" else ["-G"]), tmp_path / "cwd")
    if case.startswith("good"):
        assert p.returncode == 0 and _said(p, what, unit), p.stdout + p.stderr
    elif case == "damaged":
        assert p.returncode == 2 and "DIFFERENT" in p.stdout and "the reads" in p.stdout and "they were kept" not in p.stdout, p.stdout + p.stderr
    else:
        assert p.returncode == 1 and "holds none" in p.stdout, p.stdout + p.stderr
    assert [f.name for f in tmp_path.iterdir() if f.name != "cwd"] == ["X.minicom"] and not list((tmp_path / "cwd").iterdir())


def _members(archive_path, work):
    """every file of an archive, the packed groups opened: name -> bytes (tar headers carry times, the members do not)"""
    import io
    out = {}
    work.mkdir()
    with tarfile.open(archive_path) as t:
        for m in t.getmembers():
            if not m.isfile():
                continue
            data, name = t.extractfile(m).read(), os.path.basename(m.name)
            if name.endswith(".rans"):
                (work / name).write_bytes(data)
                assert subprocess.run([os.path.join(ROOT, "bin", "mcomz"), "d", str(work / name), str(work / name[:-5])]).returncode == 0
                data, name = (work / name[:-5]).read_bytes(), name[:-5]
            if name.endswith(".tar"):
                with tarfile.open(fileobj=io.BytesIO(data)) as inner:
                    for im in inner.getmembers():
                        if im.isfile():
                            out[name + "/" + os.path.basename(im.name)] = inner.extractfile(im).read()
            else:
                out[name] = data
    return out


@pytest.mark.parametrize("mode", ["order_QN", "pair"])
def test_without_K_the_archive_and_the_decode_are_what_they_were(archives, tmp_path, mode):
    """the archive made without -K holds the members of the one made with it but digest.txt, byte for byte; -d says nothing of a digest"""
    d, arc = archives(mode)
    plain, _ = archives(mode, digest=False)
    with_k, without = _members(d / arc, tmp_path / "a"), _members(plain / arc, tmp_path / "b")
    assert "digest.txt" in with_k and "digest.txt" not in without
    assert with_k.pop("digest.txt").decode() == dr.digest_text(*[[tuple(r) for r in recs] for recs in _synthetic(61)][:2 if mode == "pair" else 1])
    assert with_k == without
    (tmp_path / "out").mkdir()
    p = _run(["-d", plain / arc, "-G"], tmp_path / "out")
    assert p.returncode == 0 and "verified" not in p.stdout and "digest" not in p.stdout + p.stderr, p.stdout + p.stderr


def test_refusals(archives, tmp_path):
    """-K with an input that is no four-line record of the limits: said, status 1, no archive; -T with -c; the executable's own refusals"""
    recs = _synthetic(81, n=300)[0]
    recs[7] = (b"n" * 300, recs[7][1], recs[7][2], recs[7][3])                       # a name of 300 bytes: the reads are fine, the digest is not
    (tmp_path / "X.fastq").write_bytes(rc.text_of(recs))
    p = _run(["-r", "X.fastq", "-G", "-K"], tmp_path)
    assert p.returncode == 1 and "record 8 is not a four-line FASTQ record" in p.stderr and "minicom: -K: the input cannot be digested" in p.stdout, p.stdout + p.stderr
    assert sorted(f.name for f in tmp_path.iterdir()) == ["X.fastq"]
    d, arc = archives("order_QN")
    p = _run(["-d", d / arc, "-T", "-c", d / "X.fastq"], tmp_path)
    assert p.returncode == 1 and "use one of them" in p.stdout, p.stdout + p.stderr
    exe = os.path.join(ROOT, "bin", "mcomz")
    (tmp_path / "short.fastq").write_bytes(rc.text_of(recs[:6]))
    (tmp_path / "long.fastq").write_bytes(rc.text_of(recs[:7]))
    p = subprocess.run([exe, "e", "--fastq-digest", "--gpu", str(tmp_path / "short.fastq"), str(tmp_path / "long.fastq"), str(tmp_path / "d.txt")], capture_output=True, text=True)
    assert p.returncode == 1 and "different numbers of records: 6 and 7" in p.stderr and not (tmp_path / "d.txt").exists(), p.stdout + p.stderr
    p = subprocess.run([os.path.join(ROOT, "bin", "decompress"), "--check-digest", "--gpu", str(tmp_path), str(tmp_path / "short.fastq")], capture_output=True, text=True)
    assert p.returncode == 1 and "no digest.txt" in p.stderr, p.stdout + p.stderr


def test_python_container(tmp_path):
    """compress_fastq(digest=True) and compress_fastq_pair(digest=True): decompress_file checks, test_file tests, a damaged digest is said"""
    from minicom_amd import McomError, container
    a, b = _synthetic(91, n=500)
    (tmp_path / "A_1.fastq").write_bytes(rc.text_of(a))
    (tmp_path / "A_2.fastq").write_bytes(rc.text_of(b))
    one, two, bare = str(tmp_path / "one.minicom"), str(tmp_path / "two.minicom"), str(tmp_path / "bare.minicom")
    sizes = container.compress_fastq(str(tmp_path / "A_1.fastq"), one, order=True, quality=True, names=True, codec="rans", digest=True)
    assert sizes["digest.txt"] == len(dr.digest_text(a))
    assert "digest.txt" in container.compress_fastq_pair(str(tmp_path / "A_1.fastq"), str(tmp_path / "A_2.fastq"), two, quality=True, names=True, codec="rans", digest=True)
    assert "digest.txt" not in container.compress_fastq(str(tmp_path / "A_1.fastq"), bare, codec="rans")
    for device in (0, None):
        assert container.decompress_file(one, str(tmp_path / "o.fastq"), device=device) == 500
        assert (tmp_path / "o.fastq").read_bytes() == rc.text_of(a)
        rep = container.test_file(one, device=device)
        assert rep["identical"] and rep["compared"] == ["seq.ordered.1", "qual.ordered.1", "name.ordered.1"]
        rep = container.test_file(two, device=device)
        assert rep["identical"] and rep["compared"] == ["seq.ordered.1", "qual.ordered.1", "name.ordered.1", "seq.ordered.2", "qual.ordered.2", "name.ordered.2"]
    with pytest.raises(McomError, match="holds no digest.txt"):
        container.test_file(bare, device=0)
    _repack(one, tmp_path / "bad.minicom", tmp_path / "w", _one_digit)
    assert container.test_file(str(tmp_path / "bad.minicom"), device=0)["differing"] == ["qual.ordered.1"]
    with pytest.raises(McomError, match="qual.ordered.1 differs"):
        container.decompress_file(str(tmp_path / "bad.minicom"), str(tmp_path / "o2.fastq"), device=0)
    assert (tmp_path / "o2.fastq").read_bytes() == rc.text_of(a)
    assert sorted(f.name for f in tmp_path.iterdir() if f.name.startswith("tmp")) == []
