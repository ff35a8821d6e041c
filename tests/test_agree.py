"""`minicom -a Q[:C]` on the host: the plain C++ twins -- mcomh_agree_mask with device -1, mcomh_qual_agree, the
quality-member call behind `mcomz e --fastq-qual ... --agree` -- against the independent statement of tests/agree_cases.py, the refusals,
and the fuzz program under the sanitizers.  No GPU."""
import ctypes as C
import gzip
import io
import os
import shutil
import subprocess
import tarfile

import numpy as np
import pytest

import agree_cases as AC
import qual_cases as QC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")


def _untar(golden_dir, name, d):
    d.mkdir()
    with gzip.open(os.path.join(golden_dir, name), "rb") as g:
        tf = tarfile.open(fileobj=io.BytesIO(g.read()))
        for m in tf.getmembers():
            (d / m.name).write_bytes(tf.extractfile(m).read())


def _vacuity(bits, member_rows):
    """the mask of the contig members must hold a set and a clear bit: a test over an empty or a full mask shows nothing"""
    m = bits[member_rows]
    assert m.any() and not m.all(), "vacuous: the members' mask rows are all %s" % ("set" if m.any() else "clear")


# ---- the mask twin ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [False, True], ids=["default", "order"])
@pytest.mark.parametrize("n_members", AC.HAND_MEMBERS)
@pytest.mark.parametrize("L", AC.HAND_L)
def test_mask_twin_on_hand_made_archives(tmp_path, L, n_members, order):
    from minicom_amd.pipeline import agree_mask, decompress
    d = tmp_path / "a"
    reads, truth, member_rows, n_lists = AC.write_hand_made(d, L, n_members, order)
    n = decompress(str(d), str(tmp_path / "reads"), order=order)
    assert (tmp_path / "reads").read_bytes().decode().split("\n")[:-1] == reads and n == len(reads)     # the archive is what the builder says it is
    for Cm in AC.HAND_C:
        want = truth(Cm)
        mask, gotL, bits = agree_mask(str(d), Cm)
        assert gotL == L and mask.shape == (len(reads), (L + 7) // 8)
        assert np.array_equal(mask, AC.pack_mask(want)), (L, n_members, order, Cm)
        assert bits == int(want.sum())
        lists = np.setdiff1d(np.arange(len(reads)), member_rows)
        assert len(lists) == n_lists and not want[lists].any()                                          # counted lists, single.seq, single_N.seq: zero rows
        if Cm <= 3:
            _vacuity(want, member_rows)
        if Cm == 255:
            assert not want.any()
    # the parser of agree_cases.py reads the same archive to the same truth (it is what the fixtures and the pipeline's archives are checked with)
    p_reads, p_bits, p_rows = AC.parse_folder(d, 2)
    assert p_reads == reads and np.array_equal(p_bits, truth(2)) and sorted(p_rows) == sorted(member_rows)


def test_a_contig_of_one_member(tmp_path):
    """the mask twin on the lone member of a contig: all zero for C >= 2, every agreeing column for C = 1"""
    from minicom_amd.pipeline import agree_mask
    d = tmp_path / "a"
    reads, truth, member_rows, _ = AC.write_hand_made(d, 41, 16, False)
    sets = AC.hand_made_sets(41, 16)
    lone = [k for k, m in enumerate(sets[0].members) if m[0] == 1]
    assert len(lone) == 1
    row = member_rows[lone[0]]
    m1 = AC.unpack_mask(agree_mask(str(d), 1)[0], 41)
    m2 = AC.unpack_mask(agree_mask(str(d), 2)[0], 41)
    assert not m2[row].any() and not truth(2)[row].any()
    assert m1[row].sum() == 41 - 3 and np.array_equal(m1[row], truth(1)[row])                            # pattern 6: three literals that differ


def test_coverage_does_not_cross_stream_sets(tmp_path):
    from minicom_amd.pipeline import agree_mask
    for order in (False, True):
        d = tmp_path / ("s%d" % order)
        reads, truth, member_rows, _ = AC.write_hand_made(d, 40, 16, order, second_set=True)
        lone = member_rows[-1]                                                                          # the second set's only member, at the offset of contig 0 of the first
        for Cm in (1, 2, 3):
            want = truth(Cm)
            mask, _, _ = agree_mask(str(d), Cm)
            assert np.array_equal(mask, AC.pack_mask(want)), (order, Cm)
            assert want[lone].any() == (Cm == 1)


@pytest.mark.parametrize("name,order", [("streams_order_stages_L100", True), ("streams_order_stages_L150", True), ("streams_stages_L40", False),
                                        ("streams_stages_L100", False), ("streams_stages_L150", False)])
def test_mask_twin_on_the_golden_streams(golden_dir, tmp_path, name, order):
    from minicom_amd.pipeline import agree_mask, decompress
    d = tmp_path / "s"
    _untar(golden_dir, name + ".tar.gz", d)
    decompress(str(d), str(tmp_path / "reads"), order=order)
    reads = (tmp_path / "reads").read_bytes().decode().split("\n")[:-1]
    for Cm in (1, 3):
        p_reads, p_bits, p_rows = AC.parse_folder(d, Cm)
        assert p_reads == reads
        mask, L, bits = agree_mask(str(d), Cm)
        assert np.array_equal(mask, AC.pack_mask(p_bits)), (name, Cm)
        assert bits == int(p_bits.sum())
    _vacuity(AC.parse_folder(d, 1)[1], p_rows)


# ---- the transform twin --------------------------------------------------------------------------------------------------------------------------
def _host():
    from minicom_amd.pipeline import load_host_library
    return load_host_library()


@pytest.mark.parametrize("n", [0, 1, 17])
@pytest.mark.parametrize("L,pitch_extra,mask_extra,first", [(37, 0, 0, 0), (40, 5, 0, 3), (41, 1, 2, 1), (150, 16, 1, 0), (256, 0, 0, 2), (1, 3, 0, 0)])
def test_transform_twin_with_canaries(L, pitch_extra, mask_extra, first, n):
    from minicom_amd.hip import QualAgreeReport
    rng = np.random.default_rng(L * 100 + n)
    pitch, mb = L + pitch_extra, (L + 7) // 8
    mp = mb + mask_extra
    rows = QC.synth_quals(L + n, max(n, 1), L)[:n]
    bits = rng.random((first + n, L)) < 0.6
    buf = np.full(64 + n * pitch + 64, 0xA5, np.uint8)                                                  # canaries around and between the rows
    view = buf[64:64 + n * pitch].reshape(n, pitch) if n else np.zeros((0, pitch), np.uint8)
    if n:
        view[:, :L] = rows
    mask = np.full((first + n, mp), 0xFF, np.uint8)                                                     # the bytes behind ceil(L / 8) are hostile: never read as columns
    mask[:, :mb] = AC.pack_mask(bits)
    mask_before = mask.copy()
    for Q in (0, 40, 93):
        b = buf.copy()
        r = QualAgreeReport()
        assert _host().mcomh_qual_agree(b[64:].ctypes.data if n else None, n, L, pitch, mask.ctypes.data if mask.size else None, mp, first, Q, C.byref(r)) == 0
        want, rep = AC.transform(rows, bits[first:], Q)
        got = b[64:64 + n * pitch].reshape(n, pitch) if n else np.zeros((0, pitch), np.uint8)
        assert np.array_equal(got[:, :L], want)
        assert (got[:, L:] == 0xA5).all() and (b[:64] == 0xA5).all() and (b[64 + n * pitch:] == 0xA5).all()
        assert r.as_dict() == rep
        assert np.array_equal(mask, mask_before)
    if n:                                                                                                # the Python mirror: the same bytes and report
        from minicom_amd.pipeline import qual_agree
        out, rep2 = qual_agree(rows, mask, 40, first_mask_row=first)
        want, rep = AC.transform(rows, bits[first:], 40)
        assert np.array_equal(out, want) and rep2 == rep


def test_transform_twin_refuses_bad_arguments():
    from minicom_amd.hip import QualAgreeReport
    rows = np.full((3, 40), 70, np.uint8); mask = np.full((3, 5), 0xFF, np.uint8)
    call = lambda n, L, pitch, mp, Q, rp=rows, mk=mask: _host().mcomh_qual_agree(rp.ctypes.data if rp is not None else None, n, L, pitch, mk.ctypes.data if mk is not None else None, mp, 0, Q, None)
    assert call(3, 40, 40, 5, 40) == 0 and (rows == 73).all()
    rows[:] = 70
    for bad in ((3, 40, 40, 5, 94), (3, 0, 40, 5, 40), (3, 257, 257, 33, 40), (3, 40, 39, 5, 40), (3, 40, 40, 4, 40)):
        assert call(*bad) == -1, bad
        assert (rows == 70).all()
    assert call(3, 40, 40, 5, 40, rp=None) == -1 and call(3, 40, 40, 5, 40, mk=None) == -1
    assert call(0, 40, 40, 5, 40, rp=None, mk=None) == 0


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def _damages(L):
    def cut(name, how):
        def f(c):
            b = (c / name).read_bytes()
            (c / name).write_bytes(b[:len(b) - 1] if how == "one" else b[:len(b) // 2])
        return f

    def patch(name, at, data):
        def f(c):
            b = bytearray((c / name).read_bytes()); b[at:at + len(data)] = data
            (c / name).write_bytes(bytes(b))
        return f

    def first_line(name, line):
        def f(c):
            b = (c / name).read_bytes()
            (c / name).write_bytes(line + b[b.index(b"\n"):])
        return f

    return {"dif_char cut by half": cut("dif_char.txt.0", "half"), "beg_pos cut by half": cut("beg_pos.bin.0", "half"), "ref cut by half": cut("ref.bin.0", "half"),
            "num = 2^31": patch("beg_pos.bin.0", 0, np.uint32(1 << 31).tobytes()), "digit run longer than L": first_line("dif_char.txt.0", str(L + 1).encode()),
            "run that passes L behind a literal": first_line("dif_char.txt.0", b"A" + str(L).encode() + b"C"), "byte 0x01 in dif_char": patch("dif_char.txt.0", 0, b"\x01"),
            "no info.txt": lambda c: os.remove(c / "info.txt")}


@pytest.mark.parametrize("order", [False, True], ids=["default", "order"])
def test_a_damaged_folder_has_no_mask_and_leaves_no_file(tmp_path, order):
    from minicom_amd.hip import McomError
    from minicom_amd.pipeline import agree_mask, decompress
    L = 40
    good = tmp_path / "good"
    AC.write_hand_made(good, L, 17, order)
    damages = dict(_damages(L))
    if order:
        damages["id >= n_seq"] = lambda c: (c / "ids.bin.0").write_bytes(np.uint32(10 ** 6).tobytes() + (c / "ids.bin.0").read_bytes()[4:])
        damages["duplicated id"] = lambda c: (c / "singleFile.ids.bin").write_bytes((c / "singleFile.ids.bin").read_bytes()[:4] + np.uint32(0).tobytes())
    out = tmp_path / "m.mask"
    for name, damage in damages.items():
        c = tmp_path / "bad"
        shutil.copytree(good, c)
        damage(c)
        verdict = []
        for call in (lambda: decompress(str(c), str(tmp_path / "x"), order=order), lambda: agree_mask(str(c), 2, out_path=str(out))):
            try:
                call(); verdict.append(False)
            except McomError:
                verdict.append(True)
        assert verdict[0] == verdict[1], name                                                           # what the decoder refuses has no mask, what it takes has one
        if verdict[1]:
            assert not out.exists(), name
        else:                                                                                           # (a cut that ends on a contig's header: fewer reads, no error)
            p_reads, p_bits, _ = AC.parse_folder(c, 2)
            assert np.array_equal(np.fromfile(out, np.uint8).reshape(len(p_reads), -1), AC.pack_mask(p_bits)), name
            os.remove(out)
        if name != "beg_pos cut by half":
            assert verdict[1], name
        shutil.rmtree(c)
    for Cm in (0, 256, -1):
        with pytest.raises(McomError):
            agree_mask(str(good), Cm, out_path=str(out))
        assert not out.exists()
    # archives whose decoder's row order is not covered: paired end in the default mode, ragged
    for extra in ("len.bin",) if order else ("file.bin.0", "len.bin"):                                   # (ids.bin.* says -p before file.bin.* is looked for)
        c = tmp_path / "bad"
        shutil.copytree(good, c)
        (c / extra).write_bytes(b"\0")
        with pytest.raises(McomError):
            agree_mask(str(c), 2, out_path=str(out))
        assert not out.exists(), extra
        shutil.rmtree(c)
    assert agree_mask(str(good), 2, out_path=str(out))[0].size and out.exists()                         # and the good folder has one afterwards


def test_marker(tmp_path):
    from minicom_amd.hip import McomError
    from minicom_amd.pipeline import qual_agree_marker
    assert qual_agree_marker(str(tmp_path)) is None
    for text, want in ((b"40 3\n", (40, 3)), (b"0 1\n", (0, 1)), (b"93 255\n", (93, 255))):
        (tmp_path / "qual_agree.txt").write_bytes(text)
        assert qual_agree_marker(str(tmp_path)) == want
    for text in (b"x", b"", b"40 3", b"40:3\n", b"94 3\n", b"40 0\n", b"40 256\n", b"040 3\n", b"40 3\n\n", b"40 3 \n"):
        (tmp_path / "qual_agree.txt").write_bytes(text)
        with pytest.raises(McomError):
            qual_agree_marker(str(tmp_path))


# ---- the quality member ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def order_fixture(golden_dir, tmp_path_factory):
    """the golden -p stream files of L = 100, their reads, synthetic qualities as a FASTQ file, the mask file for C = 2 and its bits"""
    from minicom_amd.pipeline import agree_mask, decompress
    t = tmp_path_factory.mktemp("agree_member")
    d = t / "s"
    _untar(golden_dir, "streams_order_stages_L100.tar.gz", d)
    decompress(str(d), str(t / "reads"), order=True)
    reads = np.frombuffer((t / "reads").read_bytes(), np.uint8).reshape(-1, 101)[:, :100]
    quals = QC.synth_quals(5, reads.shape[0], 100)
    (t / "in.fastq").write_bytes(QC.fastq_bytes(reads, quals))
    mask, L, _ = agree_mask(str(d), 2, out_path=str(t / "m.mask"))
    bits = AC.parse_folder(d, 2)[1]
    assert np.array_equal(mask, AC.pack_mask(bits))
    return t, quals, bits


def _decode_member(path):
    from minicom_amd.pipeline import qual_decode
    return qual_decode(open(path, "rb").read())


def test_mcomz_agree_member_is_the_transform_of_the_lines(order_fixture):
    from minicom_amd.pipeline import qual_transform
    t, quals, bits = order_fixture
    n = quals.shape[0]
    exe = os.path.join(BIN, "mcomz")
    p = subprocess.run([exe, "e", "--fastq-qual", "100", "--agree", "40", str(t / "m.mask"), str(t / "in.fastq"), str(t / "a.mcq")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.split() == [str(n)], p.stderr
    want, rep = AC.transform(quals, bits, 40)
    assert rep["changed"] > 0
    assert ("agree 40: mask_bits %d changed %d sum_abs %d sum_sq %d max_abs %d" % (rep["mask_bits"], rep["changed"], rep["sum_abs"], rep["sum_sq"], rep["max_abs"])) in p.stderr
    assert np.array_equal(_decode_member(t / "a.mcq"), want)
    # with --lossy as well: agreement first, then SPEC (Q = 30, which ill8 moves: the order of the two steps shows)
    p = subprocess.run([exe, "e", "--fastq-qual", "100", "--agree", "30", str(t / "m.mask"), "--lossy", "ill8", str(t / "in.fastq"), str(t / "b.mcq")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    both, _ = qual_transform(AC.transform(quals, bits, 30)[0], "ill8")
    other, _ = AC.transform(qual_transform(quals, "ill8")[0], bits, 30)
    assert not np.array_equal(both, other)
    assert np.array_equal(_decode_member(t / "b.mcq"), both)
    assert p.stderr.index("agree 30:") < p.stderr.index("lossy ill8:")
    # --mask-first: the second half of the rows under the mask rows of the second half
    half = n // 2
    (t / "half.fastq").write_bytes(b"".join((t / "in.fastq").read_bytes().split(b"\n")[4 * half:4 * n][k] + b"\n" for k in range(4 * (n - half))))
    p = subprocess.run([exe, "e", "--fastq-qual", "100", "--agree", "40", str(t / "m.mask"), "--mask-first", str(half), str(t / "half.fastq"), str(t / "c.mcq")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert np.array_equal(_decode_member(t / "c.mcq"), want[half:])
    # --order: the rows gathered first, the mask row r beside member row r
    order = np.random.default_rng(3).permutation(n).astype("<u4")
    (t / "order.bin").write_bytes(order.tobytes())
    p = subprocess.run([exe, "e", "--fastq-qual", "100", "--order", str(t / "order.bin"), "--agree", "40", str(t / "m.mask"), str(t / "in.fastq"), str(t / "d.mcq")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert np.array_equal(_decode_member(t / "d.mcq"), AC.transform(quals[order], bits, 40)[0])


def test_mcomz_agree_refusals(order_fixture, tmp_path):
    t, quals, bits = order_fixture
    exe = os.path.join(BIN, "mcomz")
    out = tmp_path / "x.mcq"
    (tmp_path / "short.mask").write_bytes((t / "m.mask").read_bytes()[:-13])
    (tmp_path / "odd.mask").write_bytes((t / "m.mask").read_bytes() + b"\0")
    for args in (["--agree", "94", str(t / "m.mask")], ["--agree", "040", str(t / "m.mask")], ["--agree", "x", str(t / "m.mask")], ["--agree", "40", str(tmp_path / "none.mask")],
                 ["--agree", "40", str(tmp_path / "short.mask")], ["--agree", "40", str(tmp_path / "odd.mask")], ["--agree", "40", str(t / "m.mask"), "--mask-first", "1"],
                 ["--agree", "40", str(t / "m.mask"), "--mask-first", "-1"]):
        p = subprocess.run([exe, "e", "--fastq-qual", "100"] + args + [str(t / "in.fastq"), str(out)], capture_output=True, text=True)
        assert p.returncode == 1 and p.stderr.strip() and not out.exists(), args
    p = subprocess.run([exe, "e", "--qual", "100", "--agree", "40", str(t / "m.mask"), str(t / "in.fastq"), str(out)], capture_output=True, text=True)
    assert p.returncode == 1 and not out.exists()


def test_decompress_agree_mask_tool(order_fixture, tmp_path):
    t, quals, bits = order_fixture
    exe = os.path.join(BIN, "decompress")
    p = subprocess.run([exe, "--agree-mask", str(t / "s"), "2", str(tmp_path / "m")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.split() == [str(bits.shape[0]), "100", str(int(bits.sum()))], p.stderr
    assert (tmp_path / "m").read_bytes() == (t / "m.mask").read_bytes()
    for Cm in ("0", "256", "03", "x", ""):
        p = subprocess.run([exe, "--agree-mask", str(t / "s"), Cm, str(tmp_path / "bad")], capture_output=True, text=True)
        assert p.returncode == 1 and p.stderr.strip() and not (tmp_path / "bad").exists(), Cm


# ---- the sanitizers ------------------------------------------------------------------------------------------------------------------------------
def test_fuzz_program_under_the_sanitizers(tmp_path):
    """tests/fuzz_agree.cpp built with -fsanitize=address,undefined and run on the CPU over hand-made folders of both modes"""
    exe = tmp_path / "fuzz_agree"
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "minicom_amd", "host"), "fuzz_agree", "FUZZ_AGREE_OUT=" + str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    AC.write_hand_made(tmp_path / "arch0", 37, 17, False)
    AC.write_hand_made(tmp_path / "arch1", 41, 16, True, second_set=True)
    p = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and "fuzz_agree ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
