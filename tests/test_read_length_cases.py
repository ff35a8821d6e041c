"""CPU: the inputs of tests/read_length_cases.py do what they are built for, on the sequential oracle alone.  Without this the GPU
tests of test_gpu_read_lengths.py could pass on rows that miss their target."""
import numpy as np
import pytest

import read_length_cases as rlc


def test_sweep_holds_three_lengths_of_every_word_count():
    assert len(rlc.SWEEP) == 24 and rlc.SWEEP[0] == 1 and rlc.SWEEP[-1] == 256
    for W in range(1, 9):
        ls = [L for L in rlc.SWEEP if (L + 31) // 32 == W]
        assert ls == [32 * W - 31, 32 * W - 13, 32 * W]
        assert ls[1] % 16 != 0
    assert rlc.ks(256) == [31, 30, 17, 16, 15, 8] and rlc.ks(19) == [19, 17, 16, 15, 8] and rlc.ks(1) == [1]
    assert rlc.ks(31) == [31, 30, 17, 16, 15, 8] and rlc.ks(8) == [8]
    # (W, k >= 17, k odd) picks the sketch kernel: the sweep reaches all 32
    assert len({((L + 31) // 32, k >= 17, k % 2) for L in rlc.SWEEP for k in rlc.ks(L)}) == 32


@pytest.mark.parametrize("e", [1, 4])
@pytest.mark.parametrize("L", rlc.SWEEP)
def test_every_directed_row_gets_the_class_it_is_built_for(L, e):
    import oracle
    rows = rlc.class_rows(L, e)
    names = [n for n, _, _, _ in rows]
    assert len(set(names)) == len(names)
    reads, want = rlc.class_matrix(L, e)
    assert set(np.unique(reads).tolist()) <= set(b"ACGTN")
    sub, cls, _, ncnt = oracle.process_reads_batch(reads, rlc.ks(L)[0], e=e)
    for (name, row, c, rep), got in zip(rows, cls):
        assert got == c, (L, e, name, int(got))
    assert np.array_equal(ncnt, (reads == ord("N")).sum(axis=1))
    if L >= 16:
        assert set(cls.tolist()) == set(range(8))                  # every class of include/mcom.h
        assert sum(n.startswith("tie_") for n in names) == 11
        assert {"N_at_%d" % p for p in rlc.N_POSITIONS + (L - 1,) if p < L} <= set(names)
        assert {"near_%s_%d_bases" % (b, m) for b in "ATN" for m in (e, e + 1)} <= set(names)
        assert {"N_%d_of_%d" % (int(0.4 * L) + d, L) for d in (0, 1)} <= set(names)
    # the substituted base: the intended winner of every tie, the background of a near row that is kept
    checked = 0
    for i, (name, row, c, rep) in enumerate(rows):
        isn = row == ord("N")
        if c == rlc.SKETCH:
            assert np.array_equal(sub[i][~isn], row[~isn])
            assert ord("N") not in sub[i]
        if rep is not None:
            assert c == rlc.SKETCH and isn.any() and np.all(sub[i][isn] == ord(rep)), (L, e, name)
            checked += 1
    assert checked >= (11 if L >= 16 else 0)


@pytest.mark.parametrize("L", [2, 7, 8])
def test_a_row_of_two_near_classes_is_poly_a(L):
    """L <= 2 e: as many T as A is no further than e from all-A and from all-T; the reference tests all-A first."""
    import oracle
    rows = {n: (r, c) for n, r, c, _ in rlc.class_rows(L, 4)}
    row, c = rows["near_A_and_T"]
    assert c == rlc.NEARA and (row != ord("A")).sum() <= 4 and (row != ord("T")).sum() <= 4
    assert oracle.process_reads_batch(row[None, :], min(L, 8), e=4)[1][0] == rlc.NEARA


@pytest.mark.parametrize("L", rlc.SWEEP)
def test_sketch_batch_reaches_both_ends_of_the_read_on_both_strands(L):
    """Over the 4000 reads of sketch_reads_for(L) the oracle's records hold the first (k-1) and the last (L-1) position of a k-mer's
    last base, each on both strands, for every k of ks(L); and an even k leaves (AT)n and (GC)n without a minimizer."""
    import oracle
    reads = rlc.sketch_reads_for(L)
    directed = rlc.directed_sketch_rows(L)
    assert directed.shape == (6, L)
    for k in rlc.ks(L):
        rec = oracle.sketch_two_batch(reads, k)
        y = rec["y"][rec["x"] != np.uint64(0xFFFFFFFFFFFFFFFF)]
        assert len(rlc.position_coverage(y, k, L)) == (4 if k < L else 2), (L, k)
        d = oracle.sketch_two_batch(directed, k)
        if k % 2 == 0:
            assert int((d["x"] == np.uint64(0xFFFFFFFFFFFFFFFF)).sum()) >= 2, (L, k)
        else:                                                       # an odd k-mer never equals its reverse complement
            assert len(y) == len(rec) and not (d["x"] == np.uint64(0xFFFFFFFFFFFFFFFF)).any(), (L, k)


@pytest.mark.parametrize("L", [L for L in rlc.SWEEP if L >= 32])
def test_encode_byte_cases_give_both_answers(L):
    import oracle
    reads, contigs, cid, pos, dirs = rlc.encode_byte_cases(L)
    assert len(reads) >= 200 and set(dirs.tolist()) == {0, 1}
    lens = np.array([len(c) for c in contigs])
    assert (pos == 0).sum() > 20 and (pos == lens[cid] - L).sum() > 20 and np.all(pos + L <= lens[cid])
    got = {oracle.encode_byte(reads[i].tobytes(), contigs[cid[i]] + b"\0", int(pos[i]), int(dirs[i]), L) for i in range(len(reads))}
    assert got == {0, 1}
