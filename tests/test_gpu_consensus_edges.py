"""The consensus kernels at the boundaries of their counters (include/mcom.h: mcom_group_consensus = construct_ref,
mcom_merge_consensus_jobs = construct_ref2).  Which of the six kernels runs depends on three constants, and every one of them is
pinned here with counters filled to their last value; whoever changes one of the constants finds the test to move by its name:

  BS_NMAX = 31  (consensus_bs.hip)  groups of up to 31 members take the bit-sliced kernel (5-bit counters), groups of 32 and more
                                    k_group_consensus_reg<NU> (32 members held in registers, the rest streamed)
                                    -> test_group_sizes_and_full_counters, test_unaligned_stride_takes_the_wave_per_group_kernel
  BS_KM = 7     (consensus_bs.hip)  a 32-column unit that more than 127 members reach hands its 512-column tile to k_merge_consensus_reg
                                    -> test_merge_consensus_at_the_depth_cap
  GC_BIG = 65535 (consensus.hip)    groups and jobs of 65 535 members and more are redone with 32-bit counters in LDS
                                    (k_group_consensus<false>, k_merge_consensus<false>)
                                    -> test_groups_at_gc_big, test_jobs_at_gc_big

Every case is a deterministic stack (consensus_reference.stack); every test first asserts on the reference alone that its case has
the property it was built for and only then looks at the device; every comparison is byte for byte."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from consensus_reference import ACGT, _construct_ref, _oriented, construct_ref2_cols, construct_ref_detail, stack

pytestmark = pytest.mark.gpu
A, C_, G, T = 0, 1, 2, 3


@pytest.fixture(scope="module")
def ctx():
    import minicom_amd
    c = minicom_amd.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- group cases --------------------------------------------------------------------------------------------------------------
def _source(L, k, seed):
    """2L random bases with T on the k-mer's columns: a counter that wraps there reads "empty", not "A wins anyway"."""
    src = ACGT[np.random.default_rng(seed).integers(0, 4, 2 * L)].copy()
    src[L - k:L] = ord("T")
    return src


def _case_full(L, k, e, n, seed):
    """n identical members at offset 0, both directions: every column counts n of one base."""
    src = _source(L, k, seed)
    src[0] = ord("T")

    def prop(r):
        assert r.keep.all() and r.sv == 0 and r.ref == src[:L].tobytes()
        assert (r.c1.sum(axis=0)[:L] == n).all() and (r.c1[T, L - k:L] == n).all() and r.c1[T, 0] == n
    return src, [(0, i & 1, []) for i in range(n)], prop


def _case_tie(L, k, e, n, seed, v):
    """All members at offset 0; one column in every 32-column unit (so: in every 64-column block, the last partial ones included)
    where the members split between two bases.  Odd n: ceil(n/2) of the larger code over floor(n/2) of the smaller one, which loses by
    one.  Even n: an exact tie (the smaller code wins), or n/2 : n/2 - 1 : 1 with a third base, where the smaller code loses by one.
    The losing members are the first or the last ones of the list in turn, so that nobody loses more than half of the columns."""
    src = _source(L, k, seed)
    cols = [min(32 * u + (7 * u + 5) % 32, L - 1) for u in range((L + 31) // 32)]
    pairs = [(T, G), (G, C_), (C_, A), (T, A), (G, A), (T, C_)]
    ov = [[] for _ in range(n)]
    want = []
    h = n // 2
    for j, c in enumerate(cols):
        hi, lo = pairs[(j + v) % 6]
        lose1 = n % 2 == 0 and n >= 4 and (j + v) % 2 == 1
        losers = range(n - h, n) if j % 2 else range(h)
        if n % 2 == 0 and not lose1:                                            # exact tie at full depth: the larger code loses
            for i in range(n):
                ov[i].append((c, hi if i in losers else lo))
            want.append((c, lo, {hi: h, lo: n - h}))
        elif not lose1:                                                         # odd n: the smaller code loses by one
            for i in range(n):
                ov[i].append((c, lo if i in losers else hi))
            want.append((c, hi, {hi: n - h, lo: h}))
        else:
            third = next(q for q in range(4) if q not in (hi, lo))
            for i in range(n):
                ov[i].append((c, hi if i not in losers else (third if i == losers[-1] else lo)))
            want.append((c, hi, {hi: h, lo: h - 1, third: 1}))

    def prop(r):
        for c, win, counts in want:
            assert r.first[c] == win and all(r.c1[q, c] == counts.get(q, 0) for q in range(4)), (c, r.c1[:, c])
        if e >= (len(cols) + 1) // 2:
            assert r.keep.all()
        elif n > 2:
            assert not r.keep.all() and r.keep.any()                            # e = 0: who lost a tie is rejected
        assert r.ref_len == L
    return src, [(0, i & 1, ov[i]) for i in range(n)], prop


def _case_reject(L, k, e, n, seed):
    """Member 0 alone at offset 0 and rejected, so sv > 0; everybody else at offset 1.  The rejected members (member 0 and the last
    (n-1)/4) hold T over the source's G at the same e + 1 columns; (n-1)/4 kept members hold C at e other columns: exactly e mismatches.
    At one more column X enough clean members hold C for C to win once the rejected members, who hold G, are taken out: the majority
    changes between the first and the second consensus.  (With e = 0 a kept member equals the first consensus wherever it lies, so no
    covered column can change: X is left out.)"""
    src = _source(L, k, seed)
    ncol = 2 * e + 2
    cols = [1 + (i * (L - 2)) // (ncol - 1) for i in range(ncol)]
    assert len(set(cols)) == ncol and cols[-1] == L - 1
    src[cols] = ord("G")
    pr, pk, X = cols[:e + 1], cols[e + 1:2 * e + 1], cols[2 * e + 1]
    nx = (n - 1) // 4
    rej = [0] + list(range(n - nx, n))
    kept_e = list(range(1, 1 + nx))
    clean = [i for i in range(n) if i not in rej and i not in kept_e]
    flip = e >= 1
    ov = [[] for _ in range(n)]
    for i in rej:
        ov[i] += [(c, T) for c in pr]
    for i in kept_e:
        ov[i] += [(c, C_) for c in pk]
    if flip and n == 2:
        ov[0].append((X, A))                                                    # A over G by the tie rule; alone, member 1 says G
    elif flip:
        b = (n - len(rej) + 1) // 2                                             # G wins with the rejected members, C wins (or ties) without
        assert b <= len(clean) and n - b > b and b >= n - b - len(rej)
        for i in clean[:b]:
            ov[i].append((X, C_))

    def prop(r):
        mask = np.zeros(n, dtype=bool); mask[rej] = True
        assert np.array_equal(r.keep, ~mask) and not r.keep[0] and r.sv == 1
        assert (r.dif[rej] == e + 1).all() and (r.dif[np.array(kept_e, dtype=np.int64)] == e).all()
        if flip:
            assert r.first[X] != r.second[X], (n, r.c1[:, X], r.c2[:, X])
    return src, [(0 if i == 0 else 1, i & 1, ov[i]) for i in range(n)], prop


def _case_span(L, k, e, n, seed):
    """Members at offset 0 and at offset L - k, both directions: the longest consensus there is, 2L - k."""
    src = _source(L, k, seed)

    def prop(r):
        assert r.keep.all() and r.sv == 0 and len(r.ref) == 2 * L - k and r.ref == src[:2 * L - k].tobytes()
    return src, [(0 if i < (n + 1) // 2 else L - k, (i + i // 2) & 1, []) for i in range(n)], prop


def _case_none_kept(L, k, e, seed):
    """Two members that differ at 2e + 2 columns, each with the smaller code at e + 1 of them: the first consensus takes the smaller
    code everywhere, both members miss it e + 1 times."""
    src = _source(L, k, seed)
    cols = [(i * (L - 1)) // (2 * e + 1) for i in range(2 * e + 2)]
    assert len(set(cols)) == 2 * e + 2
    src[cols] = ord("C")

    def prop(r):
        assert not r.keep.any() and r.ref == b"" and (r.dif == e + 1).all()
    return src, [(0, 0, [(c, A) for c in cols[0::2]]), (0, 1, [(c, A) for c in cols[1::2]])], prop


def _case_one_kept(L, k, e, seed, kept):
    """Two members that differ at e + 1 columns, the same one with the smaller code every time: it is kept, the other one is not."""
    src = _source(L, k, seed)
    cols = [(i * (L - 1)) // max(e, 1) for i in range(e + 1)] if e else [L // 2]
    assert len(set(cols)) == e + 1
    src[cols] = ord("C")

    def prop(r):
        assert r.keep.tolist() == [kept == 0, kept == 1] and r.dif[1 - kept] == e + 1 and len(r.ref) == L
    spec = [(0, 0, []), (0, 1, [])]
    spec[kept] = (0, kept, [(c, A) for c in cols])
    return src, spec, prop


SIZES = [33, 2, 64, 31, 8, 40, 3, 32, 9, 65, 30, 41]          # around BS_NMAX = 31 and around the 32 members k_group_consensus_reg holds; interleaved
GROUP_SHAPES = [(100, 31, 4), (33, 11, 1), (256, 31, 4), (16, 11, 0), (17, 11, 1), (32, 11, 2), (255, 31, 4),
                (65, 17, 2), (96, 31, 4), (129, 31, 4), (160, 31, 4), (161, 31, 4), (192, 31, 4), (193, 31, 4), (224, 31, 4)]   # NU = 3, 5, 6, 7 at both ends


def _assemble(L, k, e, cases, vectorised=False):
    """cases: (name, src, spec, prop).  One call's inputs, the reference's result for every group (property asserted), and what
    process_bucket makes of it (kthread_bucket.c:446-505)."""
    from minicom_amd.hip import pack_nt4
    reads, members, goff, names, res = [], [], [0], [], []
    nrid = 0
    for name, src, spec, prop in cases:
        r, m = stack(L, k, spec, src=src, rid0=nrid)
        nrid += len(r); reads.append(r); members.append(m); goff.append(goff[-1] + len(m)); names.append(name)
    reads = np.concatenate(reads); members = np.concatenate(members)
    contigs, rejects = [], []
    for g, (name, src, spec, prop) in enumerate(cases):
        a, b = goff[g], goff[g + 1]
        d = construct_ref_detail(reads, members[a:b], L, k, e)
        if not vectorised:                                                      # the per-member loop is the statement; the detail only adds what prop looks at
            keep, new, sv, ref = _construct_ref(reads, members[a:b], L, k, e)
            assert d.keep.tolist() == [bool(x) for x in keep] and d.new.tolist() == new and (d.sv, d.ref) == (sv, ref), name
        prop(d)                                                                 # the case is what it was built to be
        res.append(d)
        nk = int(d.keep.sum())
        if nk > 1:                                                              # :451 a contig, members re-based to sv
            contigs.append((d.ref, d.new[d.keep] - np.uint64(d.sv << 1)))
        if not (nk == b - a and nk > 1):                                        # the rejected ones first, then a contig of one dissolved
            rejects += [(int(y >> np.uint64(32)), g) for y in d.new[~d.keep]]
            if nk == 1:
                rejects += [(int(y >> np.uint64(32)), g) for y in d.new[d.keep]]
    return SimpleNamespace(L=L, k=k, e=e, reads=reads, packed=pack_nt4(reads), members=members, goff=np.array(goff, dtype=np.int32),
                           names=names, res=res, contigs=contigs, rejects=rejects)


@functools.lru_cache(maxsize=None)
def _group_call(L, k, e):
    cases, seed = [], 17 * L + e
    for n in SIZES:
        for name, made in (("full", _case_full(L, k, e, n, seed)), ("tie0", _case_tie(L, k, e, n, seed + 1, 0)), ("reject", _case_reject(L, k, e, n, seed + 2)),
                           ("tie1", _case_tie(L, k, e, n, seed + 3, 1)), ("span", _case_span(L, k, e, n, seed + 4))):
            cases.append(("%s n=%d" % (name, n),) + made)
            seed += 5
        if n == 40:
            cases.append(("none kept",) + _case_none_kept(L, k, e, seed))
            cases.append(("one kept: the first",) + _case_one_kept(L, k, e, seed + 1, 0))
    cases.append(("one kept: the second",) + _case_one_kept(L, k, e, seed + 2, 1))
    cases.append(("none kept",) + _case_none_kept(L, k, e, seed + 3))
    call = _assemble(L, k, e, cases)
    nk = [int(r.keep.sum()) for r in call.res]
    assert nk.count(0) == 2 and nk.count(1) >= 2 and any(r.sv > 0 for r in call.res)
    return call


def _run_groups(ctx, call, stride=None, contigs=True):
    """mcom_group_consensus (and mcom_groups_to_contigs behind it) on one call's groups, against the reference's results."""
    L, goff = call.L, call.goff
    d_packed, d_members, d_goff = _dev(call.packed.view(np.int64)), _dev(call.members.view(np.int64)), _dev(goff)
    gc = ctx.group_consensus(d_packed, d_members, d_goff, L, call.k, call.e, stride=stride)
    ctx.sync()
    st = gc["stride"]
    assert st == ((2 * L + 15) & ~15 if stride is None else stride)
    keep, mem = gc["keep"].cpu().numpy(), d_members.cpu().numpy().view(np.uint64)
    nkept, sv, reflen = gc["nkept"].cpu().numpy(), gc["sv"].cpu().numpy().view(np.uint16), gc["reflen"].cpu().numpy().view(np.uint16)
    refs = gc["refs"].cpu().numpy()
    strings = []
    for g, r in enumerate(call.res):
        a, b = goff[g], goff[g + 1]
        name = (g, call.names[g])
        assert np.array_equal(keep[a:b], r.keep.astype(np.uint8)), name
        assert np.array_equal(mem[a:b], r.new), name
        nk = int(r.keep.sum())
        assert int(nkept[g]) == nk and int(reflen[g]) == len(r.ref), name
        assert nk == 0 or int(sv[g]) == r.sv, name
        strings.append(refs[g * st: g * st + len(r.ref)].tobytes())
        assert strings[-1] == r.ref, name
    if contigs:
        out = ctx.groups_to_contigs(d_members, d_goff, gc, cap_chars=2 * L * len(goff), cap_members=len(call.members), cap_contigs=len(goff))
        nc, nch, nmm, nrj = out["counts"]
        assert nc == len(call.contigs) and nrj == len(call.rejects)
        soff, moff = out["soff"].cpu().numpy(), out["moff"].cpu().numpy()
        seq, cm = out["seq"].cpu().numpy().tobytes(), out["mem"].cpu().numpy().view(np.uint64)
        for c, (ref, mm) in enumerate(call.contigs):
            assert seq[soff[c]:soff[c + 1]] == ref and np.array_equal(cm[moff[c]:moff[c + 1]], mm), c
        assert list(zip(out["rej_rid"].cpu().numpy().tolist(), out["rej_group"].cpu().numpy().tolist())) == call.rejects
    return strings


@pytest.mark.parametrize("L,k,e", GROUP_SHAPES)
def test_group_sizes_and_full_counters(ctx, L, k, e):
    """Sizes on both sides of BS_NMAX = 31 and of the 32 (and 64) members the wave-per-group kernel takes per round, each as a pile that
    fills every counter to n, with ties at full depth, with kept and rejected members one mismatch apart, and at the greatest length;
    between them two-member groups that keep nobody and one member.  The sizes are interleaved, so that neither the order of the small
    groups nor the list of the others is the identity.  L: NU = 1 .. 8 column blocks, LG = 1 (L <= 16: 64 groups per wave), 2 (L = 17),
    and 2L exactly one wave wide (L = 32)."""
    call = _group_call(L, k, e)
    assert (np.diff(np.diff(call.goff) >= 32) != 0).sum() > 10                 # interleaved
    _run_groups(ctx, call)


@pytest.mark.parametrize("L,k,e", GROUP_SHAPES)
def test_unaligned_stride_takes_the_wave_per_group_kernel(ctx, L, k, e):
    """mcom_group_consensus leaves the bit-sliced kernel out when ref_stride is no multiple of 4 (it stores four characters at a time):
    every group, the small ones included, then takes k_group_consensus_reg without a group list.  Same groups, same results; with an
    even stride also the same strings as the default stride gives, group by group."""
    call = _group_call(L, k, e)
    base = _run_groups(ctx, call, contigs=False)
    for stride in (2 * L + 1, 2 * L + 2 if (2 * L + 2) % 4 else 2 * L + 3):
        assert stride % 4 and stride >= 2 * L
        got = _run_groups(ctx, call, stride=stride, contigs=stride == 2 * L + 1)
        if stride % 2 == 0:
            assert got == base


def test_groups_at_gc_big(ctx):
    """GC_BIG = 65535: a group of 65 534 members is the last one for the 16-bit counters of k_group_consensus_reg, groups of 65 535 and
    65 537 members are redone by k_group_consensus<false> with 32-bit counters; the small groups between them are done by the first
    launches and must be left alone by the last one.  Every member of a big group holds T on the k-mer's columns (the count is the group
    size: 65 536 would read as nothing in 16 bits), member 0 and a block of 300 members in the middle are rejected, and one column is
    split ceil(n/2) G : floor(n/2) C (even n: an exact tie)."""
    L, k, e = 33, 11, 1                                                         # the smallest shapes with two 64-column blocks
    tie, p1, p2 = 20, 10, 15

    def big(n, seed):
        src = _source(L, k, seed)
        src[[tie, p1, p2]] = ord("G")
        block = range(n // 2 - 150, n // 2 + 150)
        rej = [0] + list(block)
        spec = []
        for i in range(n):
            ov = [(tie, G if i < (n + 1) // 2 else C_)]
            if i == 0 or i in block:
                ov += [(p1, T), (p2, T)]
            spec.append((0 if i == 0 else 1 + (4 * (i - 1)) // (n - 1), i & 1, ov))

        def prop(r):
            assert (r.c1[T, L - k:L] == n).all() and r.c1[G, tie] == (n + 1) // 2 and r.c1[C_, tie] == n // 2
            assert r.first[tie] == (C_ if n % 2 == 0 else G)
            mask = np.ones(n, dtype=bool); mask[rej] = False
            assert np.array_equal(r.keep, mask) and r.sv == 1 and len(r.ref) == L + 3
            assert (r.c2[T, L - k:L] == n - 301).all()
        return src, spec, prop

    cases = [("reject n=5",) + _case_reject(L, k, e, 5, 1), ("big 65534",) + big(65534, 2), ("reject n=40",) + _case_reject(L, k, e, 40, 3),
             ("big 65535",) + big(65535, 4), ("span n=9",) + _case_span(L, k, e, 9, 5), ("full n=33",) + _case_full(L, k, e, 33, 6),
             ("big 65537",) + big(65537, 7), ("none kept",) + _case_none_kept(L, k, e, 8), ("tie n=64",) + _case_tie(L, k, e, 64, 9, 0)]
    call = _assemble(L, k, e, cases, vectorised=True)
    assert sorted(np.diff(call.goff).tolist())[-3:] == [65534, 65535, 65537]
    _run_groups(ctx, call)


# ---- merge cases --------------------------------------------------------------------------------------------------------------
def _sorted_members(lst):
    return sorted(lst, key=lambda y: y & 0xFFFFFFFF)                            # cmpcluster2; python's sort is stable


def _reach(off, L, c0, ce):
    """how many members' reads reach the columns [c0, ce)"""
    return int(((off + L > c0) & (off < ce)).sum())


def _depth_job(L, d, t, rng, reads):
    """Two parents whose merge has one 32-column unit that exactly d members reach, all of them over three columns c, c+1, c+2:
    ceil(d/2) reads that end at c + 2 and floor(d/2) that start at c, dealt out to the two parents in turn.  Everything else is a thin
    chain of reads that stay clear of that unit -- in the grid of the whole contig (units from column 0) and in the grid of the overlap
    (units from lo).  Column c: d times T.  Column c + 1: ceil(d/2) G over floor(d/2) C (even d: an exact tie, C wins).  Column c + 2:
    the smaller code loses by one (even d: d/2 G, d/2 - 1 C, one A; odd d: ceil(d/2) T, floor(d/2) G).
    With reads shorter than 27 columns the pile cannot cover its whole unit and nobody else may reach it: a few columns stay empty ('A')."""
    sh = 133                                                                    # the overlap's start lo: 5 past a multiple of 32, no multiple of 512
    t2 = t % 3 + 1
    lf, total = sh + 640 + t, 928 + t2                                          # the overlap [sh, lf) and the contig end in units of t and t2 columns
    c = 32 * ((sh + L + 31) // 32) + 10
    src = ACGT[rng.integers(0, 4, total)]
    step = max(L // 2, 1)
    left_end = c - 10 - L                                                       # last start of a read that ends before both grids' deep unit
    F = sorted(set(range(0, left_end + 1, step)) | {left_end} | set(range(c + 27, lf - L + 1, step)) | {lf - L})
    S = sorted(set(range(sh, left_end + 1, step)) | {left_end} | set(range(c + 27, total - L + 1, step)) | {total - L})
    assert left_end >= sh and lf - L >= c + 27
    mf, ms = [], []

    def add(lst, off, dr, ov):
        row = src[off:off + L].copy()
        for col, b in ov:
            row[col - off] = ACGT[b]
        lst.append((len(reads) << 32) | ((off - (sh if lst is ms else 0)) << 1) | dr)
        reads.append(_oriented(row, dr))                                         # stored as the read file holds it
    for i, off in enumerate(F):
        add(mf, off, i & 1, [])
    for i, off in enumerate(S):
        add(ms, off, (i + 1) & 1, [])
    na = (d + 1) // 2
    for i in range(d):
        if d % 2 == 0:
            third = G if i < d // 2 else (C_ if i < d - 1 else A)
        else:
            third = T if i < na else G
        ov = [(c, T), (c + 1, G if i < na else C_), (c + 2, third)]
        add(mf if i % 2 == 0 else ms, c + 3 - L if i < na else c, (i >> 1) & 1, ov)
    return SimpleNamespace(mf=_sorted_members(mf), ms=_sorted_members(ms), sh=sh, lf=lf, total=total, c=c, d=d, t=t, t2=t2)


@pytest.mark.parametrize("L,depths", [(100, (126, 127, 128, 129, 255, 256)), (256, (127, 128)), (16, (127, 128))])
def test_merge_consensus_at_the_depth_cap(ctx, L, depths):
    """BS_KM = 7: the bit-sliced merge kernel counts up to 127 members per unit; the 128th member hands the unit's 512-column tile to
    the wave-per-tile kernel, which also rewrites the tile's shallow units.  One job per depth d around 127 (and around 255), each
    with exactly one unit that d members reach (the reads that end or start in it make d/2 in its neighbours: below the cap up to
    d = 129, above it too for d = 255 and 256), in a contig of two tiles, with an overlap that starts at lo = 133 and ends in a unit of
    1, 2 or 3 columns like the contig itself (the byte tail of the four-at-a-time store).  Both call forms -- every column counted,
    and the overlap only with the rest copied from the parents -- against the column counts, against the oracle's construct_ref2 and
    against each other; again with the cap lowered to 1 (every tile handed over) and to 126 (d = 127 handed over as well)."""
    import oracle
    import torch
    from minicom_amd.hip import pack_nt4
    rng = np.random.default_rng(1000 + L)
    reads, jobs_d, mems, jobs = [], [], [], []
    for j, d in enumerate(depths):
        J = _depth_job(L, d, j % 3 + 1, rng, reads)
        jobs_d.append(J)
        if j % 2 == 0:                                                          # the first parent is ci or cj: both branches of the member merge
            mems += [J.mf, J.ms]; jobs.append((2 * j, 2 * j + 1, J.sh + 7, 7))
        else:
            mems += [J.ms, J.mf]; jobs.append((2 * j, 2 * j + 1, 7, J.sh + 7))
    reads = np.stack(reads)
    refs = [construct_ref2_cols(reads, m, L)[0] for m in mems]                  # a parent's string is the majority of its own members
    want_m, want_refs = [], []
    for J in jobs_d:
        lst = _sorted_members(J.mf + [y + (J.sh << 1) for y in J.ms])           # kthread_cb.c:297-325, :107
        ref, cnt = construct_ref2_cols(reads, lst, L)
        want_m.append(lst); want_refs.append(ref)
        # the case is what it was built to be
        off = (np.array(lst, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64) >> 1
        assert len(ref) == J.total > 512 and J.total % 32 == J.t2 and (J.lf - J.sh) % 32 == J.t and J.lf - J.sh > 512
        assert J.sh % 32 and J.sh % 512 and len(refs[mems.index(J.mf)]) == J.lf and len(refs[mems.index(J.ms)]) == J.total - J.sh
        for lo, hi in ((0, J.total), (J.sh, J.lf)):                             # the units of the whole contig, and of the overlap
            depth = [_reach(off, L, c0, min(c0 + 32, hi)) for c0 in range(lo, hi, 32)]
            deep = (J.c - lo) // 32
            assert depth[deep] == J.d and (J.c + 2 - lo) // 32 == deep
            others = depth[:deep] + depth[deep + 1:]
            assert max(others) <= (J.d + 1) // 2 + 16 and (J.d > 129 or max(others) < 100)
            assert deep * 32 // 512 == 0 and len(depth) > 16                    # one of two tiles
        d = J.d
        assert cnt[:, J.c].tolist() == [0, 0, 0, d] and ref[J.c:J.c + 1] == b"T"
        assert cnt[:, J.c + 1].tolist() == [0, d // 2, (d + 1) // 2, 0] and ref[J.c + 1:J.c + 2] == (b"G" if d % 2 else b"C")
        if d % 2 == 0:
            assert cnt[:, J.c + 2].tolist() == [1, d // 2 - 1, d // 2, 0] and ref[J.c + 2:J.c + 3] == b"G"
        else:
            assert cnt[:, J.c + 2].tolist() == [0, 0, d // 2, (d + 1) // 2] and ref[J.c + 2:J.c + 3] == b"T"
        assert (cnt.sum(axis=0) > 0).all() or L < 27
        assert oracle.construct_ref2(reads, lst) == ref
    soff = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int64)
    moff = np.concatenate([[0], np.cumsum([len(m) for m in mems])]).astype(np.int64)
    seq = np.frombuffer(b"".join(refs), dtype=np.uint8).copy(); mem = np.array([y for m in mems for y in m], dtype=np.uint64)
    d_seq, d_soff, d_jobs = _dev(seq), _dev(soff), _dev(np.array(jobs, dtype=np.int32))
    jm, jmoff, jroff, tot = ctx.merge_members(_dev(mem.view(np.int64)), _dev(moff), d_jobs, L, 14)
    assert jm.cpu().numpy().view(np.uint64).tolist() == [y for lst in want_m for y in lst]
    assert np.array_equal(jroff.cpu().numpy(), np.concatenate([[0], np.cumsum([len(r) for r in want_refs])]))
    d_packed = _dev(pack_nt4(reads).view(np.int64))
    want = b"".join(want_refs)
    try:
        for cap in (0, 1, 126):
            ctx.set_consensus_capacity(cap)
            full = ctx.merge_consensus_jobs(d_packed, jm, jmoff, jroff, tot[1], L)
            part = ctx.merge_consensus_jobs(d_packed, jm, jmoff, jroff, tot[1], L, jobs=d_jobs, seq=d_seq, soff=d_soff)
            got = full.cpu().numpy().tobytes()
            for j, J in enumerate(jobs_d):
                a = sum(len(r) for r in want_refs[:j])
                assert got[a:a + J.total] == want_refs[j], (cap, J.d, [i for i in range(J.total) if got[a + i] != want_refs[j][i]][:8])
            assert got == want and torch.equal(full, part), cap
    finally:
        ctx.set_consensus_capacity(0)


def test_jobs_at_gc_big(ctx):
    """GC_BIG = 65535 for the merge consensus: a job of 65 537 members is too deep for the bit-sliced units, is turned away by
    k_merge_consensus_reg (16-bit counters) and redone by k_merge_consensus<false>; a job 300 deep in the same call stays with the 16-bit
    tile kernel and must be left alone by the <false> launch; a job of five members stays bit-sliced.  In a second call the largest job
    has 65 534 members: the 16-bit counters' last value.  Column 25 holds T in every member that covers it (65 536 of them: nothing, in
    16 bits), column 30 is split half G, half C, column 31 likewise with one A, so that C loses by one."""
    import oracle
    from minicom_amd.hip import pack_nt4
    L = 33
    allT, tie, lose = 25, 30, 31
    rows, index = [], {}

    def rid_of(src_id, src, off, dr, ov):
        key = (src_id, off, dr, tuple(ov))
        if key not in index:
            row = src[off:off + L].copy()
            for col, b in ov:
                row[col - off] = ACGT[b]
            index[key] = len(rows)
            rows.append(_oriented(row, dr))
        return index[key]

    def job(src_id, piles, tail=None):
        """piles: (offset, count), all covering columns 25 .. 31; tail: one more read behind them that does not"""
        src = ACGT[np.random.default_rng(50 + src_id).integers(0, 4, 120)].copy()
        n = sum(cnt for _, cnt in piles)
        lst, i = [], 0
        for off, cnt in piles:
            assert off <= allT and lose < off + L
            for _ in range(cnt):
                ov = [(allT, T), (tie, G if i < (n + 1) // 2 else C_), (lose, G if i < (n + 1) // 2 else (A if i == n - 1 else C_))]
                dr = (i >> 2) & 1
                lst.append((rid_of(src_id, src, off, dr, ov) << 32) | (off << 1) | dr)
                i += 1
        if tail is not None:
            lst.append((rid_of(src_id, src, tail, 0, []) << 32) | (tail << 1))
        return _sorted_members(lst), n

    big, nb = job(0, [(0, 30000), (10, 20000), (20, 15536)], tail=40)
    deep, nd = job(1, [(0, 75), (1, 75), (2, 75), (3, 75)])
    small, ns = job(2, [(0, 1), (5, 1), (10, 1), (15, 1), (20, 1)])
    last, nl = job(3, [(0, 30000), (10, 20000), (20, 15534)])
    assert (len(big), nb, len(deep), len(small), len(last)) == (65537, 65536, 300, 5, 65534)
    reads = np.stack(rows)
    calls = []
    for lists in ((big, deep, small), (small, last, deep)):
        want = []
        for lst in lists:
            ref, cnt = construct_ref2_cols(reads, lst, L)
            n = len(lst) - (lst is big)
            # the case is what it was built to be
            assert cnt[:, allT].tolist() == [0, 0, 0, n] and ref[allT:allT + 1] == b"T"
            assert cnt[:, tie].tolist() == [0, n // 2, (n + 1) // 2, 0] and ref[tie:tie + 1] == (b"G" if n % 2 else b"C")
            assert cnt[:, lose].tolist() == [1, n // 2 - 1, (n + 1) // 2, 0] and ref[lose:lose + 1] == b"G"
            assert (cnt.sum(axis=0) > 0).all() and ref == oracle.construct_ref2(reads, lst)
            want.append(ref)
        calls.append((lists, want))
    d_packed = _dev(pack_nt4(reads).view(np.int64))
    for lists, want in calls:
        jm = np.array([y for lst in lists for y in lst], dtype=np.uint64)
        jmoff = np.concatenate([[0], np.cumsum([len(lst) for lst in lists])]).astype(np.int64)
        jroff = np.concatenate([[0], np.cumsum([len(r) for r in want])]).astype(np.int64)
        got = ctx.merge_consensus_jobs(d_packed, _dev(jm.view(np.int64)), _dev(jmoff), _dev(jroff), int(jroff[-1]), L).cpu().numpy().tobytes()
        for j, ref in enumerate(want):
            assert got[jroff[j]:jroff[j + 1]] == ref, (len(lists[j]), [i for i in range(len(ref)) if got[jroff[j] + i] != ref[i]][:8])


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_empty_calls_return(ctx):
    """L outside 1 .. 256, k_orig outside 1 .. 31 and a stride below 2L are turned away by the entry points before anything is
    launched; no groups and no jobs are no error."""
    import torch
    from minicom_amd.hip import McomError
    L, k, e = 33, 11, 1
    src, spec, _ = _case_span(L, k, e, 5, 1)
    reads, members = stack(L, k, spec, src=src)
    from minicom_amd.hip import pack_nt4
    big = np.zeros((len(reads), 9), dtype=np.uint64)                           # room for 257 bases a read, whatever the call believes
    big[:, :2] = pack_nt4(reads)
    d_packed, d_goff = _dev(big.view(np.int64)), _dev(np.array([0, len(members)], dtype=np.int32))
    fresh = lambda: _dev(members.view(np.int64))
    for bad in (dict(L=257), dict(L=0), dict(k_orig=0), dict(k_orig=32), dict(stride=2 * L - 1)):
        args = dict(L=L, k_orig=k, e=e); args.update(bad)
        d_members = fresh()
        with pytest.raises(McomError):
            ctx.group_consensus(d_packed, d_members, d_goff, **args)
        ctx.sync()
        assert np.array_equal(d_members.cpu().numpy().view(np.uint64), members), bad      # nothing ran
    lst = _sorted_members([(i << 32) | ((3 * i) << 1) | (i & 1) for i in range(5)])
    jm, jmoff, jroff = _dev(np.array(lst, dtype=np.uint64).view(np.int64)), _dev(np.array([0, 5], dtype=np.int64)), _dev(np.array([0, 12 + 257], dtype=np.int64))
    with pytest.raises(McomError):
        ctx.merge_consensus_jobs(d_packed, jm, jmoff, jroff, 12 + 257, 257)
    # ... and the calls still work afterwards
    gc = ctx.group_consensus(d_packed[:, :2].contiguous(), fresh(), d_goff, L, k, e)
    assert int(gc["nkept"][0]) == 5 and int(gc["reflen"][0]) == 2 * L - k
    # nothing to do
    none64, zero64 = torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    gc = ctx.group_consensus(d_packed, none64, torch.zeros(1, dtype=torch.int32, device="cuda"), L, k, e)
    ctx.sync()
    assert gc["stride"] == 80
    out = ctx.merge_consensus_jobs(d_packed, none64, zero64, zero64, 0, L)
    assert out.numel() == 0
