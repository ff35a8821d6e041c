"""The consensus references hold each other (no GPU): the whole-array construct_ref of tests/consensus_reference.py against the
per-member loop it restates, the column-count construct_ref2 against the oracle's C restatement, and what stack() promises."""
import numpy as np
import pytest

from consensus_reference import ACGT, _construct_ref, _oriented, construct_ref2_cols, construct_ref_vec, stack


def _random_groups(rng, n_groups, L, k, e):
    """Random stacks: offsets all over [0, L-k], both directions, substitutions from none to well above e."""
    out = []
    for g in range(n_groups):
        n = int(rng.choice([2, 2, 3, 5, 9, 30, 33, 70]))
        src = ACGT[rng.integers(0, 4, 2 * L)]
        spec = []
        for i in range(n):
            o = int(rng.integers(0, L - k + 1)) if i else 0
            cols = rng.integers(o, o + L, int(rng.choice([0, 0, 0, 1, e, e + 1, 3 * e + 2])))
            spec.append((o, int(rng.integers(0, 2)), [(int(c), int(rng.integers(0, 4))) for c in cols]))
        out.append(stack(L, k, spec, src=src))
    return out


@pytest.mark.parametrize("L,k,e", [(100, 31, 4), (33, 11, 1), (16, 11, 0), (256, 31, 4)])
def test_vectorised_construct_ref_equals_the_member_loop(L, k, e):
    rng = np.random.default_rng(L)
    kinds = set()
    for reads, members in _random_groups(rng, 60, L, k, e):
        keep, new, sv, ref = _construct_ref(reads, members, L, k, e)
        vkeep, vnew, vsv, vref = construct_ref_vec(reads, members, L, k, e)
        assert vkeep.tolist() == [bool(x) for x in keep] and vnew.tolist() == new and (vsv, vref) == (sv, ref)
        kinds.add((sum(keep) == 0, sum(keep) == len(keep), sv > 0))
    assert len(kinds) >= 3                                                      # all kept, some rejected, and more than that


def test_stack_lays_members_as_the_group_sort_hands_them_over():
    L, k = 40, 17
    src = ACGT[np.random.default_rng(3).integers(0, 4, 2 * L)]
    spec = [(5, 1, [(7, 3)]), (0, 0, []), (L - k, 1, []), (5, 0, [(44, 0), (5, 2)]), (0, 1, [(0, 1)])]
    reads, members = stack(L, k, spec, src=src, rid0=100)
    assert [int(y >> np.uint64(32)) for y in members] == [101, 104, 100, 103, 102]   # offset ascending (al descending), then rid
    for y in members.tolist():
        i, pos, d = (y >> 32) - 100, (y & 0xFFFFFFFF) >> 1, y & 1
        o, ds, ov = spec[i]
        want = src[o:o + L].copy()
        for c, b in ov:
            want[c - o] = ACGT[b]
        assert d == ds and np.array_equal(_oriented(reads[i], d), want)
        al = L - pos + k - 2 if d else pos
        assert al == (L - 1) - o and k - 1 <= pos <= L - 1
    # the consensus of clean members is the source
    reads, members = stack(L, k, [(0, 0, []), (3, 1, []), (L - k, 0, [])], src=src)
    keep, new, sv, ref = _construct_ref(reads, members, L, k, 0)
    assert all(keep) and sv == 0 and ref == src[:2 * L - k].tobytes()
    assert [(y & 0xFFFFFFFF) >> 1 for y in new] == [0, 3, L - k]


@pytest.mark.parametrize("L", [16, 33, 100])
def test_column_count_construct_ref2_equals_the_loop_and_the_oracle(L):
    import oracle
    rng = np.random.default_rng(L)
    reads = ACGT[rng.integers(0, 4, (200, L))]
    for n in (1, 2, 7, 150):
        off = np.sort(rng.integers(0, 5 * L, n)); off[0] = 0
        members = sorted(((int(rng.integers(0, 200)) << 32) | (int(o) << 1) | int(rng.integers(0, 2)) for o in off), key=lambda y: y & 0xFFFFFFFF)
        cnt = np.zeros((4, int(off[-1]) + L), dtype=np.int64)
        for y in members:
            o = _oriented(reads[y >> 32], y & 1)
            cnt[(o >> 1 ^ o >> 2) & 3, ((y & 0xFFFFFFFF) >> 1) + np.arange(L)] += 1
        ref, got = construct_ref2_cols(reads, members, L)
        assert np.array_equal(got, cnt) and len(ref) == int(off[-1]) + L
        assert ref == oracle.construct_ref2(reads, members)                     # uncovered columns read 'A' in both
