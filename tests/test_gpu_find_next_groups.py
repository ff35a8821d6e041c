"""GPU: the candidate search of the merge rounds (mcom_find_next_candidates, _new, _ord) stages the passing candidates from the
evaluation kernel itself and can test a (query, hit) pair with one lane or with a group of G lanes (mcom_set_eval_route,
include/mcom_test.h).  The default, every compiled G and the route with a flag per pair and k_fn_emit have to list, record for record,
what numpy assembles from two entry points this change does not touch: mcom_idx_get (the hits of every query, in index order) and
mcom_match_pro (the mismatches of every pair): a pair stays where the contigs differ, the strands agree and the mismatches do not exceed
cbthr -- in query order, then hit order.

The contigs are hand-built (minicom_amd.hip.pack_contigs), records are plain (key, contig << 32 | position << 1 | strand) words:
  * the GRID: one query with one hit per case -- overlaps of 1, G - 1, G, G + 1, 2 G, 2 G + 1 words for G = 4, 8, 16 and of 1, 31, 32, 33
    and 77 bases; anchored with d < 0, d = 0, d > 0, the shifted side starting on a word boundary (32, 64 bases) or inside a word (5, 37,
    63); the overlap ended by A or by B; 0, 1, 2, 3, 8, 9 mismatches with one of them in the first or in the last base of the overlap (the
    last sub-lane's last word), which cbthr = 0, 2, 8 put exactly at and one above the threshold; a contig of random letters (leaves the
    loop early); a hit on the query's own contig and one on the other strand.  The grid's last pair ends in the store's last contig.
  * the FAMILY: pieces of one sequence with a few substitutions, all holding one position, listed 1500 times under ONE key and queried
    three times (a query's pairs cross groups, waves and workgroups), plus queries without a hit.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
MAXU = np.uint64(0xFFFFFFFFFFFFFFFF)
ROUTES = (4, 8, 16, 0, 1)                    # every compiled G; the default (one lane per pair, staged emission); the flag route
SENTINEL = -0x0123456789ABCDEF
E_OVERFLOW = -4


@pytest.fixture(scope="module")
def ctx():
    import minicom_amd
    c = minicom_amd.Context(0)
    yield c
    c.set_eval_route(0)
    c.close()


def _y(contig, pos, strand=0):
    return (int(contig) << 32) | (int(pos) << 1) | int(strand)


def _mutate(rng, seq, at):
    for p in at:
        seq[p] = rng.choice([c for c in b"ACGT" if c != seq[p]])


def _grid(rng):
    """-> (contigs, query records, index records, mismatches planted per query)"""
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    words = sorted({w for g in (4, 8, 16) for w in (1, g - 1, g, g + 1, 2 * g, 2 * g + 1)})
    lengths = [1, 31, 32, 33, 77] + [32 * w for w in words] + [32 * w - 13 for w in words if w > 1]
    refs, qrec, irec, planted = [], [], [], []
    key = 1000
    for n in lengths:
        for d in (0, 32, -32, 64, -64, 5, -5, 37, -37, 63, -63):
            for a_ends in (True, False):
                lo = max(d, 0)
                if d >= 0:
                    len_a, len_b = (d + n, n + 11) if a_ends else (d + n + 11, n)
                else:
                    len_a, len_b = (n, n - d + 11) if a_ends else (n + 11, n - d)
                a = letters[rng.integers(0, 4, len_a)].copy()
                mid = sorted(set(rng.integers(1, max(n - 1, 2), 12).tolist()) - {0, n - 1})
                variants = [None, "self", "strand", [], [0], [n - 1], [0] + mid[:1], mid[:1] + [n - 1], [0] + mid[:2], mid[:2] + [n - 1],
                            [0] + mid[:7], mid[:7] + [n - 1], [0] + mid[:8], mid[:8] + [n - 1]]
                # (a third of the variants where the shift repeats another one's case; the very last pair, d = -63 ended by B, is a full one)
                for v in variants[(rng.integers(0, 3)):: 3] if n > 33 and abs(d) in (32, 37) else variants:
                    b = letters[rng.integers(0, 4, len_b)].copy()
                    if v is not None:
                        b[lo - d: lo - d + n] = a[lo: lo + n]
                        if not isinstance(v, str):
                            v = sorted({p for p in v if 0 <= p < n})
                            _mutate(rng, b, [lo - d + p for p in v])
                    i = lo + n // 2
                    ia = len(refs); refs.append(a.tobytes())
                    if v == "self":
                        ib = ia
                        i, j = (len_a - 1, len_a - 1 - abs(d)) if len_a > abs(d) else (0, 0)
                    else:
                        ib = len(refs); refs.append(b.tobytes())
                        j = i - d
                    qrec.append((key, _y(ia, i, key & 1)))
                    irec.append((key, _y(ib, j, (key & 1) ^ (v == "strand"))))
                    planted.append(len(v) if isinstance(v, list) else -1)
                    key += 1
    return refs, qrec, irec, np.array(planted)


def _family(rng, first_id):
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = letters[rng.integers(0, 4, 900)]
    refs, start = [], []
    for c in range(40):
        a0, b0 = int(rng.integers(0, 440)), int(rng.integers(460, 900))
        s = genome[a0:b0].copy()
        _mutate(rng, s, rng.integers(0, len(s), int(rng.integers(0, 4))).tolist())
        refs.append(s.tobytes()); start.append(a0)
    key = 77
    members = rng.integers(0, 40, 1500)
    irec = [(key, _y(first_id + c, 450 - start[c], rng.random() < 0.1)) for c in members]
    qrec = [(key, _y(first_id + c, 450 - start[c], 0)) for c in (3, 17, 29)]
    qrec.insert(1, (5, _y(first_id + 1, 7)))                       # a key the index does not hold
    qrec.insert(3, (int(MAXU), 0))                                 # the empty record
    return refs, qrec, irec


def _records(t):
    import torch
    a = np.array(t, dtype=np.uint64).reshape(-1, 2)
    return torch.from_numpy(a.view(np.int64)).cuda()


@pytest.fixture(scope="module")
def world(ctx):
    """Contigs, index and the queries with the mismatches of every (query, hit) pair, computed once."""
    import torch
    from minicom_amd.hip import pack_contigs, records_to_numpy
    rng = np.random.default_rng(19)
    frefs, fq, fi = _family(rng, 0)
    grefs, gq, gi, planted = _grid(rng)                             # the grid behind the family: its last pair ends in the store's last contig
    shift = len(frefs) << 32
    gq = [(x, y + shift) for x, y in gq]; gi = [(x, y + shift) for x, y in gi]
    refs = frefs + grefs
    cbits, coff, clen = pack_contigs(refs)
    cbits = cbits[: int(coff[-1]) + (2 * int(clen[-1]) + 63) // 64 + 1]     # nothing behind the last contig's padding word
    cg = {"cbits": torch.from_numpy(cbits.view(np.int64)).cuda(), "coff": torch.from_numpy(coff.view(np.int64)).cuda(),
          "clen": torch.from_numpy(clen.view(np.int32)).cuda()}
    idx = ctx.idx_build(_records(fi + gi), 31, b=0)
    srt = records_to_numpy(idx.records())
    w = {"ctx": ctx, "cg": cg, "idx": idx, "srt": srt, "n_contigs": len(refs), "n_family_q": len(fq), "planted": planted,
         "queries": np.array(fq + gq, dtype=np.uint64).reshape(-1, 2)}
    w["pairs"] = _pairs(w, w["queries"])
    yield w
    idx.close()


def _pairs(w, queries):
    """every (query, hit) pair of `queries` in query order, then index order: (query y, hit y, mismatches, query number)"""
    import torch
    ctx = w["ctx"]
    s, c = w["idx"].get(torch.from_numpy(queries[:, 0].copy().view(np.int64)).cuda())
    ctx.sync()
    s, c = s.cpu().numpy().astype(np.int64), c.cpu().numpy().astype(np.int64)
    qi = np.repeat(np.arange(len(queries)), c)
    u = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
    my, hy = queries[qi, 1], w["srt"]["y"][s[qi] + u]
    f = lambda v: torch.from_numpy(v.astype(np.int32)).cuda()
    pos = lambda y: (y & np.uint64(0xFFFFFFFF)) >> np.uint64(1)
    mis = ctx.match_pro(w["cg"], f(my >> np.uint64(32)), f(pos(my)), f(hy >> np.uint64(32)), f(pos(hy)))
    ctx.sync()
    return {"my": my, "hy": hy, "mis": mis.cpu().numpy().astype(np.int64), "qi": qi}


def _expected(pr, cbthr, is_new=None):
    ci, cj = (pr["my"] >> np.uint64(32)).astype(np.int64), (pr["hy"] >> np.uint64(32)).astype(np.int64)
    keep = (ci != cj) & (((pr["my"] ^ pr["hy"]) & np.uint64(1)) == 0) & (pr["mis"] <= cbthr)
    if is_new is not None:
        keep &= is_new(ci) | is_new(cj)
    return np.stack([pr["my"][keep], pr["hy"][keep]], 1)


def _call(w, queries, cbthr, route, cap=None, n_new=0, ord_form=None):
    """-> (rc, pairs listed, pairs passing, the whole output buffer as uint64 [cap + 64, 2]); ord_form = (rec, roff, ord, first_new, n_new)"""
    import torch
    ctx, cg, lib = w["ctx"], w["cg"], w["ctx"].lib
    ctx.set_eval_route(route)
    cap = 1 << 16 if cap is None else cap
    out = torch.full((cap + 64, 2), SENTINEL, dtype=torch.int64, device="cuda")
    cnt = (C.c_uint64 * 2)()
    vp = C.c_void_p
    if ord_form is None:
        q = torch.from_numpy(queries.copy().view(np.int64)).cuda()
        lib.mcom_find_next_candidates_new.restype = C.c_int
        lib.mcom_find_next_candidates_new.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, vp, C.c_int, C.c_uint32, vp, C.c_size_t, vp]
        rc = lib.mcom_find_next_candidates_new(ctx._h, w["idx"]._h, ctx._p(q), len(queries), ctx._p(cg["cbits"]), ctx._p(cg["coff"]), ctx._p(cg["clen"]),
                                               cbthr, n_new, ctx._p(out), cap, cnt)
    else:
        rec, roff, ord_, first_new, n_new = ord_form
        lib.mcom_find_next_candidates_ord.restype = C.c_int
        lib.mcom_find_next_candidates_ord.argtypes = [vp] * 5 + [C.c_size_t] + [vp] * 3 + [C.c_int, C.c_uint32, C.c_uint32, vp, C.c_size_t, vp]
        rc = lib.mcom_find_next_candidates_ord(ctx._h, w["idx"]._h, ctx._p(rec), ctx._p(roff), ctx._p(ord_), int(ord_.shape[0]), ctx._p(cg["cbits"]), ctx._p(cg["coff"]),
                                               ctx._p(cg["clen"]), cbthr, first_new, n_new, ctx._p(out), cap, cnt)
    ctx.sync()
    ctx.set_eval_route(0)
    return rc, int(cnt[0]), int(cnt[1]), out.cpu().numpy().view(np.uint64)


def _check(w, queries, cbthr, want, n_listed=None, **kw):
    for route in ROUTES:
        rc, listed, n_pass, out = _call(w, queries, cbthr, route, **kw)
        assert rc == 0, (route, rc)
        assert n_pass == len(want), (route, n_pass, len(want))
        if n_listed is not None:
            assert listed == n_listed, (route, listed, n_listed)
        bad = np.nonzero((out[:n_pass] != want).any(1))[0]
        assert bad.size == 0, (route, "first differing record", int(bad[0]), out[bad[0]].tolist(), want[bad[0]].tolist())
        assert (out[n_pass:].view(np.int64) == SENTINEL).all(), (route, "written behind the last candidate")


@pytest.mark.parametrize("cbthr", [0, 2, 8])
def test_every_route_lists_what_idx_get_and_match_pro_give(world, cbthr):
    w = world
    pr = w["pairs"]
    want = _expected(pr, cbthr)
    # the fixture is what the docstring says: more than 1024 hits for one query, both sides of the threshold, own-contig and other-strand hits
    grid = pr["qi"] >= w["n_family_q"]
    assert np.bincount(pr["qi"]).max() > 1024 and (np.bincount(pr["qi"], minlength=len(w["queries"])) == 0).sum() >= 2
    assert (pr["mis"][grid] == cbthr).sum() > 50 and (pr["mis"][grid] == cbthr + 1).sum() > 50
    assert np.array_equal(pr["mis"][grid][w["planted"] >= 0], w["planted"][w["planted"] >= 0])
    assert int(pr["hy"][-1] >> np.uint64(32)) == w["n_contigs"] - 1 and w["planted"][-1] > 0     # the last pair is compared, in the last contig
    assert 100 < len(want) < len(pr["my"]) - 100
    _check(w, w["queries"], cbthr, want, n_listed=len(pr["my"]))


@pytest.mark.parametrize("n_pairs", [1, 15, 16, 17, 31, 32, 33, 63, 64, 65])
def test_pair_counts_around_a_workgroup(world, n_pairs):
    """one pair, and one less than, exactly and one more than a workgroup's pairs (256 / G = 64, 32, 16): the grid's queries have one hit each"""
    w = world
    q = w["queries"][w["n_family_q"]:][7: 7 + n_pairs]
    pr = _pairs(w, q)
    assert len(pr["my"]) == n_pairs
    _check(w, q, 2, _expected(pr, 2), n_listed=n_pairs)


def test_no_pair_passing_and_every_pair_passing(world):
    w = world
    gq = w["queries"][w["n_family_q"]:]
    q = gq[w["planted"] > 0]
    pr = _pairs(w, q)
    want = _expected(pr, 0)
    assert len(want) == 0 and len(q) > 500
    _check(w, q, 0, want, n_listed=len(q))
    q = gq[w["planted"] >= 0]
    pr = _pairs(w, q)
    want = _expected(pr, 1 << 20)
    assert len(want) == len(q) > 500
    _check(w, q, 1 << 20, want, n_listed=len(q))


def test_capacity_exact_and_one_short(world):
    w = world
    want = _expected(w["pairs"], 2)
    n_pass = len(want)
    for route in ROUTES:
        rc, _, got, out = _call(w, w["queries"], 2, route, cap=n_pass)
        assert rc == 0 and got == n_pass and np.array_equal(out[:n_pass], want), route
        assert (out[n_pass:].view(np.int64) == SENTINEL).all(), route
        rc, listed, got, out = _call(w, w["queries"], 2, route, cap=n_pass - 1)
        assert rc == E_OVERFLOW and got == n_pass and listed == len(w["pairs"]["my"]), (route, rc, got)
        assert (out[n_pass - 1:].view(np.int64) == SENTINEL).all(), (route, "written at or beyond cap")


def test_new_old_filter_flat_and_ord(world):
    """pairs of two contigs that are not new are absent, everything else unchanged: contigs [0, n_new) new in the flat form, contigs
    from first_new on in the _ord form, whose queries are the records of a permuted list of contigs of a store"""
    import torch
    w = world
    q, pr = w["queries"], w["pairs"]
    n_new = w["n_contigs"] // 3
    want = _expected(pr, 2, lambda c: c < n_new)
    full = _expected(pr, 2)
    assert 50 < len(want) < len(full) - 50
    _check(w, q, 2, want, n_new=n_new)
    # the store: records by contig (the empty record has no contig), visited in a permuted order that leaves a tenth of the contigs out
    real = q[q[:, 0] != MAXU]
    cid = (real[:, 1] >> np.uint64(32)).astype(np.int64)
    order = np.argsort(cid, kind="stable")
    rec, roff = real[order], np.concatenate([[0], np.cumsum(np.bincount(cid, minlength=w["n_contigs"]))]).astype(np.int32)
    rng = np.random.default_rng(5)
    lst = rng.permutation(w["n_contigs"])[: w["n_contigs"] - w["n_contigs"] // 10].astype(np.int32)
    visit = np.concatenate([rec[roff[c]: roff[c + 1]] for c in lst])
    pv = _pairs(w, visit)
    first_new = w["n_contigs"] - n_new
    store = (torch.from_numpy(rec.copy().view(np.int64)).cuda(), torch.from_numpy(roff).cuda(), torch.from_numpy(lst).cuda())
    for fn, nn, is_new in ((0, 0, None), (first_new, n_new, lambda c: c >= first_new)):
        want = _expected(pv, 2, is_new)
        assert len(want) > 50
        _check(w, None, 2, want, ord_form=store + (fn, nn))
