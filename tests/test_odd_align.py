"""CPU checks of `minicom -p -V -A`: the plain C++ twins (host/mcom_odd_align.cpp) against the Python restatement of
the rule (tests/odd_align_reference.py) -- hits and member bytes must be equal --, the folder call over the golden -p stream files, round
trips through the host decoders, one refusal per reason the decoder has, the fuzz program under the sanitizers, and the surface."""
import gzip
import io
import os
import random
import shutil
import struct
import subprocess
import tarfile

import numpy as np
import pytest

import odd_align_reference as ref
import ragged_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ref.cases()
F_HEADER, F_COUNT, F_SHORT, F_WINDOW, F_BUDGET, F_OFFSET, F_BASE, F_SAME, F_CRC = 1, 2, 4, 8, 16, 32, 64, 128, 256


def test_the_cases_state_what_they_claim():
    for name, refs, reads, want in CASES:
        if want is not None:
            assert ref.align_all(ref.text_of(refs), reads) == want, name


@pytest.mark.parametrize("name,refs,reads,want", CASES, ids=ref.case_ids())
def test_twins_give_the_reference(name, refs, reads, want):
    from minicom_amd import pipeline
    T = ref.text_of(refs)
    t, t_bases = pipeline.odd_text_host(refs)
    assert t_bases == len(T) and t[-1] == 0
    assert "".join("ACGT"[(int(t[i >> 5]) >> (2 * (i & 31))) & 3] for i in range(t_bases)) == T
    off = ref.offsets(reads)
    text = "".join(reads).encode()
    want_hits = ref.align_all(T, reads)
    hits = pipeline.odd_align_host(t, t_bases, text, off)
    assert [int(h) for h in hits] == want_hits
    want_member, want_res = ref.encode(T, reads, want_hits)
    member, res = pipeline.odd_align_encode_host(hits, t, t_bases, text, off)
    assert member == want_member and res == want_res
    if name == "all_aligned":
        assert res == b"" and member
    if not member:
        assert res == text and all(h == ref.NONE for h in want_hits)
        return
    assert ref.decode(member, T, res, [len(r) for r in reads]) == text
    back, flags, why = pipeline.odd_align_decode_host(member, t, t_bases, res, off)
    assert back == text and flags == 0 and why is None


def test_encoder_refuses_hit_words_the_text_does_not_bear_out():
    from minicom_amd import McomError, pipeline
    name, refs, reads, want = next(c for c in CASES if c[0] == "first_and_last_base")
    t, t_bases = pipeline.odd_text_host(refs)
    off, text = ref.offsets(reads), "".join(reads).encode()
    for bad in (ref.hit(0, 0, 300), ref.hit(1, 1, 300), ref.hit(1, 0, 4090), ref.hit(1, 0, 300) | 1 << 47):
        with pytest.raises(McomError):
            pipeline.odd_align_encode_host(np.array([bad] + want[1:], dtype=np.uint64), t, t_bases, text, off)


# ---- a member and what one damaged byte makes of it ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def good():
    from minicom_amd import pipeline
    name, refs, reads, _ = next(c for c in CASES if c[0] == "mixed_301")
    T = ref.text_of(refs)
    t, t_bases = pipeline.odd_text_host(refs)
    hits = ref.align_all(T, reads)
    member, res = ref.encode(T, reads, hits)
    return dict(T=T, t=t, t_bases=t_bases, reads=reads, hits=hits, member=member, res=res, layout=layout_of(member))


def layout_of(member):
    n_odd, n_al, _, n_mm, _ = struct.unpack_from("<QQQQQ", member, 24)
    Y = {"aligned": 64}
    Y["strand"] = Y["aligned"] + (n_odd + 7) // 8
    Y["p"] = Y["strand"] + (n_al + 7) // 8
    Y["d"] = Y["p"] + 5 * n_al
    Y["mm_off"] = Y["d"] + n_al
    Y["mm_base"] = Y["mm_off"] + n_mm
    Y["n_al"] = n_al
    return Y


def first_with_mismatch(good):
    """(index among the aligned records, index of its first mismatch, record, hit) of the first aligned record with d >= 1 and fewer than 255 bases"""
    a = m = 0
    for r, h in zip(good["reads"], good["hits"]):
        if h == ref.NONE:
            continue
        if h >> 48 and len(r) < 255:
            return a, m, r, h
        a += 1; m += h >> 48
    raise AssertionError("the case has no such record")


def damaged(good, what):
    """(member, residual, lengths) with one byte changed, and the flag that must come of it"""
    member, res, lengths, Y = bytearray(good["member"]), bytearray(good["res"]), [len(r) for r in good["reads"]], good["layout"]
    a, m, r, h = first_with_mismatch(good)
    j = good["reads"].index(r)
    if what == "window":
        member[Y["p"] + 4 * Y["n_al"] + a] = 0x7F
        return member, res, lengths, F_WINDOW
    if what == "offset":
        member[Y["mm_off"] + m] = 255
        return member, res, lengths, F_OFFSET
    if what == "base":
        member[Y["mm_base"] + m] = ord("X")
        return member, res, lengths, F_BASE
    if what == "same":
        p, s, l = h & ((1 << 40) - 1), (h >> 40) & 1, len(r)
        win = ref.revcomp(good["T"][p:p + l]) if s else good["T"][p:p + l]
        member[Y["mm_base"] + m] = ord(win[member[Y["mm_off"] + m]])
        return member, res, lengths, F_SAME
    if what == "budget":                                   # (d itself cannot change alone: the sum of d is a count.  The length of len.bin can)
        lengths[j] = 31
        return member, res, lengths, F_BUDGET
    if what == "short":
        lengths[j] = 30
        return member, res, lengths, F_SHORT
    if what == "count_header":
        member[32] ^= 1
        return member, res, lengths, F_COUNT
    if what == "count_d":
        member[Y["d"] + a] += 1
        return member, res, lengths, F_COUNT
    if what == "count_bits":
        member[Y["aligned"]] ^= 1
        return member, res, lengths, F_COUNT
    if what == "count_len_bin":
        k = good["hits"].index(ref.NONE)
        lengths[k] += 1
        return member, res, lengths, F_COUNT
    if what == "count_residual":
        return member, res[:-1], lengths, F_COUNT
    if what == "constants":
        member[12] = 16
        return member, res, lengths, F_HEADER
    if what == "magic":
        member[7] = ord("2")
        return member, res, lengths, F_HEADER
    if what == "crc_residual":
        res[0] = ord("C") if res[0] != ord("C") else ord("G")
        return member, res, lengths, F_CRC
    if what == "crc_field":
        member[20] ^= 0x10
        return member, res, lengths, F_CRC
    raise KeyError(what)


DAMAGE = ["window", "offset", "base", "same", "budget", "short", "count_header", "count_d", "count_bits", "count_len_bin", "count_residual", "constants", "magic", "crc_residual",
          "crc_field"]


@pytest.mark.parametrize("what", DAMAGE)
def test_decode_twin_refuses(good, what):
    from minicom_amd import pipeline
    member, res, lengths, flag = damaged(good, what)
    off = [0]
    for l in lengths:
        off.append(off[-1] + l)
    back, flags, why = pipeline.odd_align_decode_host(bytes(member), good["t"], good["t_bases"], bytes(res), off)
    assert back is None and flags & flag and why.startswith("odd.aln:"), (flags, why)
    assert why == pipeline.load_host_library().mcomh_odd_align_refusal(flags).decode()


# ---- the folder call and the host decoders over the golden -p stream files ---------------------------------------------------------------
def odd_folder(golden_dir, d, with_qual=True):
    """folder d: the golden -p stream files of stages_L150 as the even reads; in front of every third of them an odd record: a decoded read
    trimmed to 31 .. 149 bases (every fifth with a substitution), and now and then a random read or one shorter than 31.  Returns the records."""
    import qual_cases as qc
    from minicom_amd import pipeline
    d.mkdir()
    with gzip.open(os.path.join(golden_dir, "streams_order_stages_L150.tar.gz"), "rb") as g:
        tf = tarfile.open(fileobj=io.BytesIO(g.read()))
        for m in tf.getmembers():
            (d / m.name).write_bytes(tf.extractfile(m).read())
    with gzip.open(os.path.join(golden_dir, "stages_L150.reads.gz"), "rb") as f:
        rows = f.read().split(b"\n")[:-1]
    rng = random.Random(150)
    quals = np.resize(qc.synth_quals(22, 2000, 150), (len(rows), 150))
    recs = []
    for i, row in enumerate(rows):
        if i % 3 == 0:
            k = i // 3
            if k % 11 == 7:
                s = ref.rand_bases(rng, 60).encode()
            elif k % 13 == 5:
                s = row[:rng.randrange(1, 31)]
            else:
                src = rows[(7 * i + 3) % len(rows)]
                l = rng.randrange(31, 150)
                a = rng.randrange(0, 150 - l + 1)
                s = src[a:a + l]
                if k % 5 == 0 and b"N" not in s:
                    s = ref.mutate(s.decode(), [rng.randrange(l)]).encode()
            recs.append((b"odd%d" % i, s, b"", bytes(rng.randrange(33, 127) for _ in s)))
        recs.append((b"even%d" % i, row, b"", quals[i].tobytes()))
    want = rc.split(recs)
    assert want["L"] == 150 and want["n_even"] == len(rows)
    (d / "len.bin").write_bytes(want["len_bin"])
    (d / "odd.seq").write_bytes(want["odd_seq"])
    if with_qual:
        (d / "qual.mcq").write_bytes(pipeline.qual_encode(quals))
        (d / "odd.qual").write_bytes(want["odd_qual"])
        (d / "name.mcn").write_bytes(pipeline.name_encode(rc.name_text(recs)[0], len(recs)))
    return recs


def folder_text(d):
    """T of a folder with one stream set, by the reference: every contig is its last begin position + L bases long"""
    pos = (d / "beg_pos.bin.0").read_bytes()
    L = int((d / "info.txt").read_text().split()[0])
    at = bases = 0
    while at + 4 <= len(pos):
        num, = struct.unpack_from("<I", pos, at); at += 4
        if num:
            bases += sum(struct.unpack_from("<%dH" % num, pos, at)) + L
        at += 2 * num
    return ref.text_of([((d / "ref.bin.0").read_bytes(), bases)])


@pytest.fixture(scope="module")
def aligned_folder(golden_dir, tmp_path_factory):
    from minicom_amd import pipeline
    d = tmp_path_factory.mktemp("odd_align") / "arch"
    recs = odd_folder(golden_dir, d)
    before = {f: (d / f).read_bytes() for f in os.listdir(d)}
    counts = pipeline.odd_align_folder(str(d))
    return d, recs, before, counts


def test_folder_call_gives_the_reference_bytes(aligned_folder):
    d, recs, before, (n_odd, n_aligned, residual) = aligned_folder
    want = rc.split(recs)
    reads = [s.decode() for _, s, _, _ in recs if len(s) != 150]
    T = folder_text(d)
    hits = ref.align_all(T, reads)
    member, res = ref.encode(T, reads, hits)
    assert n_odd == want["n_odd"] == len(reads) and n_aligned == sum(h != ref.NONE for h in hits) and residual == len(res)
    assert 0 < n_aligned < n_odd                             # the trimmed reads of contig members are found, the random and the short ones are not
    assert (d / "odd.aln").read_bytes() == member and (d / "odd.seq").read_bytes() == res
    for f, data in before.items():                           # every other file is untouched
        if f != "odd.seq":
            assert (d / f).read_bytes() == data, f
    assert sorted(os.listdir(d)) == sorted(list(before) + ["odd.aln"])
    assert len(member) + len(res) < len(want["odd_seq"])


def test_folder_call_refuses_a_second_run_and_a_folder_without_odd_reads(aligned_folder, golden_dir, tmp_path):
    from minicom_amd import McomError, pipeline
    with pytest.raises(McomError):
        pipeline.odd_align_folder(str(aligned_folder[0]))
    d = tmp_path / "plain"
    d.mkdir()
    with gzip.open(os.path.join(golden_dir, "streams_order_stages_L150.tar.gz"), "rb") as g:
        tarfile.open(fileobj=io.BytesIO(g.read())).extractall(d)
    with pytest.raises(McomError):
        pipeline.odd_align_folder(str(d))
    assert not (d / "odd.aln").exists()


def test_no_read_aligned_leaves_the_folder_as_it_is(golden_dir, tmp_path):
    from minicom_amd import pipeline
    d = tmp_path / "arch"
    odd_folder(golden_dir, d, with_qual=False)
    lens = bytearray((d / "len.bin").read_bytes())
    rng = random.Random(3)
    (d / "odd.seq").write_bytes(ref.rand_bases(rng, len((d / "odd.seq").read_bytes())).encode())
    before = {f: (d / f).read_bytes() for f in os.listdir(d)}
    n_odd, n_aligned, residual = pipeline.odd_align_folder(str(d))
    assert n_aligned == 0 and residual == len(before["odd.seq"]) and n_odd == sum(b != 149 for b in lens)
    assert {f: (d / f).read_bytes() for f in os.listdir(d)} == before


def test_host_decoders_give_the_records_back(aligned_folder, tmp_path):
    from minicom_amd import pipeline
    d, recs, _, _ = aligned_folder
    out = tmp_path / "out.fastq"
    assert pipeline.decompress_fastq(str(d), str(out)) == len(recs)
    assert out.read_bytes() == rc.text_of(recs)
    exe = os.path.join(ROOT, "bin", "decompress")
    p = subprocess.run([exe, "--fastq", str(d), str(tmp_path / "out2.fastq")], capture_output=True, text=True)
    assert p.returncode == 0 and (tmp_path / "out2.fastq").read_bytes() == rc.text_of(recs), p.stdout + p.stderr
    e = tmp_path / "reads"
    shutil.copytree(d, e)
    for f in ("qual.mcq", "odd.qual", "name.mcn"):
        (e / f).unlink()
    assert pipeline.decompress(str(e), str(tmp_path / "out.reads"), order=True) == len(recs)
    assert (tmp_path / "out.reads").read_bytes() == rc.reads_only(recs)


def test_executable_step_gives_the_library_call(aligned_folder, golden_dir, tmp_path):
    d, recs, _, counts = aligned_folder
    e = tmp_path / "arch"
    odd_folder(golden_dir, e)
    p = subprocess.run([os.path.join(ROOT, "bin", "decompress"), "--odd-align", str(e)], capture_output=True, text=True)
    assert p.returncode == 0 and tuple(int(v) for v in p.stdout.split()) == counts, p.stdout + p.stderr
    assert (e / "odd.aln").read_bytes() == (d / "odd.aln").read_bytes() and (e / "odd.seq").read_bytes() == (d / "odd.seq").read_bytes()


def test_all_aligned_archive_has_no_odd_seq(aligned_folder, tmp_path):
    """every odd record aligned: the residual is empty and may be removed, as the script removes it"""
    from minicom_amd import pipeline
    d, recs, before, _ = aligned_folder
    member = (d / "odd.aln").read_bytes()
    n_odd = struct.unpack_from("<Q", member, 24)[0]
    bits = member[64:64 + (n_odd + 7) // 8]
    odd = [r for r in recs if len(r[1]) != 150]
    keep = [r for r in recs if len(r[1]) == 150 or (bits[odd.index(r) >> 3] >> (odd.index(r) & 7)) & 1]
    e = tmp_path / "arch"
    e.mkdir()
    for f, data in before.items():
        if f not in ("len.bin", "odd.seq", "odd.qual", "qual.mcq", "name.mcn"):
            (e / f).write_bytes(data)
    want = rc.split(keep)
    (e / "len.bin").write_bytes(want["len_bin"])
    (e / "odd.seq").write_bytes(want["odd_seq"])
    n_odd, n_aligned, residual = pipeline.odd_align_folder(str(e))
    assert n_odd == n_aligned > 0 and residual == 0 and (e / "odd.seq").read_bytes() == b""
    (e / "odd.seq").unlink()
    assert pipeline.decompress(str(e), str(tmp_path / "out.reads"), order=True) == len(keep)
    assert (tmp_path / "out.reads").read_bytes() == rc.reads_only(keep)


def _refused(d, tmp_path):
    from minicom_amd import McomError, pipeline
    for out, call in ((tmp_path / "never.fastq", pipeline.decompress_fastq), (tmp_path / "never.reads", lambda a, b: pipeline.decompress(a, b, order=True))):
        with pytest.raises(McomError):
            call(str(d), str(out))
        assert not out.exists()
    p = subprocess.run([os.path.join(ROOT, "bin", "decompress"), "--fastq", str(d), str(tmp_path / "never2.fastq")], capture_output=True, text=True)
    assert p.returncode != 0 and not (tmp_path / "never2.fastq").exists()
    return p.stderr


def folder_damage(d, recs, what):
    """one byte of one member of the folder changed; returns the words the decoder must say"""
    member = bytearray((d / "odd.aln").read_bytes())
    Y = layout_of(member)
    n_odd = struct.unpack_from("<Q", member, 24)[0]
    odd = [s.decode() for _, s, _, _ in recs if len(s) != 150]
    T = folder_text(d)
    hits = ref.align_all(T, odd)
    g = dict(reads=odd, hits=hits, T=T)
    a, m, r, h = first_with_mismatch(g)
    lens = bytearray((d / "len.bin").read_bytes())
    # where the record sits in len.bin: the k-th byte that is not L - 1
    odd_at = [i for i, b in enumerate(lens) if b != 149]
    j = odd.index(r)
    if what == "window":
        member[Y["p"] + 4 * Y["n_al"] + a] = 0x7F
    elif what == "offset":
        member[Y["mm_off"] + m] = 255
    elif what == "base":
        member[Y["mm_base"] + m] = ord("X")
    elif what == "same":
        p, s, l = h & ((1 << 40) - 1), (h >> 40) & 1, len(r)
        win = ref.revcomp(T[p:p + l]) if s else T[p:p + l]
        member[Y["mm_base"] + m] = ord(win[member[Y["mm_off"] + m]])
    elif what == "budget":
        lens[odd_at[j]] = 31 - 1
    elif what == "short":
        lens[odd_at[j]] = 30 - 1
    elif what == "count_header":
        member[32] ^= 1
    elif what == "count_len_bin":
        lens[odd_at[hits.index(ref.NONE)]] ^= 1
    elif what == "count_residual":
        (d / "odd.seq").write_bytes((d / "odd.seq").read_bytes()[:-1])
    elif what == "constants":
        member[8] = 25
    elif what == "crc":
        res = bytearray((d / "odd.seq").read_bytes())
        res[0] = ord("C") if res[0] != ord("C") else ord("G")
        (d / "odd.seq").write_bytes(bytes(res))
    else:
        raise KeyError(what)
    (d / "odd.aln").write_bytes(bytes(member))
    (d / "len.bin").write_bytes(bytes(lens))


WORDS = {"window": "leaves the contigs", "offset": "outside its read", "base": "outside ACGTN", "same": "repeats the contig's base", "budget": "more mismatches", "short": "shorter than 31",
         "count_header": "counts disagree", "count_len_bin": "counts disagree", "count_residual": "counts disagree", "constants": "no header of this version", "crc": "CRC-32"}


@pytest.mark.parametrize("what", list(WORDS))
def test_host_decoders_refuse(aligned_folder, tmp_path, what):
    d = tmp_path / "arch"
    shutil.copytree(aligned_folder[0], d)
    folder_damage(d, aligned_folder[1], what)
    assert WORDS[what] in _refused(d, tmp_path)


def test_odd_aln_beside_the_full_odd_seq_is_refused(aligned_folder, tmp_path):
    """what the decoder of an earlier version would have met: a member, and an odd.seq whose size the lengths do not add up to"""
    d = tmp_path / "arch"
    shutil.copytree(aligned_folder[0], d)
    (d / "odd.seq").write_bytes(aligned_folder[2]["odd.seq"])
    assert "counts disagree" in _refused(d, tmp_path)


def test_fuzz_program_under_the_sanitizers(aligned_folder, tmp_path):
    """tests/fuzz_odd_align.cpp built with -fsanitize=address,undefined and run on the CPU over the aligned folder"""
    exe = tmp_path / "fuzz_odd_align"
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "minicom_amd", "host"), "fuzz_odd_align", "FUZZ_ODD_ALIGN_OUT=" + str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    shutil.copytree(aligned_folder[0], tmp_path / "arch")
    p = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and "fuzz_odd_align ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
def test_minicom_refuses_A_without_V_before_anything_is_written(tmp_path):
    fq = tmp_path / "x.fastq"
    fq.write_bytes(b"@a\nACGT\n+\nIIII\n")
    exe = os.path.join(ROOT, "bin", "minicom")
    for args in (["-r", str(fq), "-p", "-A"], ["-r", str(fq), "-A"], ["-1", str(fq), "-2", str(fq), "-p", "-A"]):
        p = subprocess.run([exe] + args, capture_output=True, text=True, cwd=tmp_path)
        assert p.returncode == 1 and "-A" in p.stdout and "-V" in p.stdout, p.stdout + p.stderr
        assert sorted(os.listdir(tmp_path)) == ["x.fastq"]
    p = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert "\t-A \t" in p.stdout


def test_container_refuses_ragged_align_without_ragged(tmp_path):
    from minicom_amd import container
    with pytest.raises(ValueError):
        container.compress_fastq(str(tmp_path / "x.fastq"), str(tmp_path / "x.minicom"), order=True, ragged_align=True)
    assert "odd.aln" == container.ODD_ALIGN_MEMBER


def test_every_entry_point_is_declared():
    import minicom_amd
    from minicom_amd import pipeline
    assert {"mcom_odd_text_append", "mcom_odd_index_build", "mcom_odd_index_free", "mcom_odd_align", "mcom_odd_align_encode", "mcom_odd_align_decode"} <= set(minicom_amd.ABI_SYMBOLS)
    assert {"mcomh_odd_index_build", "mcomh_odd_align", "mcomh_odd_align_encode", "mcomh_odd_align_decode", "mcomh_odd_align_folder"} <= set(pipeline.HOST_ABI_SYMBOLS)
