"""Plain numpy restatements of the reference's two consensus steps, shared by tests/test_gpu_merge.py and
tests/test_gpu_consensus_edges.py (the same pattern as rans_reference.py and qual_reference.py):

  construct_ref  (kthread_bucket.c:69-377)  -- _construct_ref: the per-member loop, the primary statement;
                                               construct_ref_vec: the same counting in whole-array operations, for groups of 65 535
                                               members and more (tests/test_consensus_reference.py holds the two equal)
  construct_ref2 (kthread_cb.c:105-218)     -- construct_ref2_cols: column counts of a sorted member list, majority per column

and stack(), a deterministic builder of one minimizer group from offsets, directions and per-column overrides."""
from types import SimpleNamespace

import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.zeros(256, dtype=np.uint8); COMP[[65, 67, 71, 84]] = [84, 71, 67, 65]


def _oriented(read, d):
    return COMP[read][::-1] if d else read


def _majority(cols):
    """counts [4][n] -> base per column, ties to the smaller code A < C < G < T (strict '>' scan, kthread_bucket.c:129-141)."""
    best = np.zeros(cols.shape[1], dtype=np.int64); mx = cols[0].copy()
    for q in (1, 2, 3):
        m = cols[q] > mx
        best[m] = q; mx[m] = cols[q][m]
    return best, mx


def _construct_ref(reads, members, L, k, e):
    """construct_ref for one group (kthread_bucket.c:69-377): returns (keep flags, new member words, sv, consensus bytes)."""
    al, ds, rids = [], [], []
    for y in members.tolist():
        rid, pos, d = y >> 32, (y & 0xFFFFFFFF) >> 1, y & 1
        al.append(L - pos + k - 2 if d else pos); ds.append(d); rids.append(rid)
    offs = [al[0] - a for a in al]
    TL = 2 * L
    c1 = np.zeros((4, TL), dtype=np.int64)
    ors = [(_oriented(reads[r], d) >> 1 ^ _oriented(reads[r], d) >> 2) & 3 for r, d in zip(rids, ds)]
    for o, code in zip(offs, ors):
        c1[code, o + np.arange(L)] += 1
    first, mx = _majority(c1)
    ref_len = int(np.argmax(mx == 0)) if (mx == 0).any() else TL
    keep, c2, rend = [], np.zeros((4, TL), dtype=np.int64), 0
    for o, code in zip(offs, ors):
        cols = o + np.arange(L)
        dif = int(((cols >= ref_len) | (first[np.minimum(cols, TL - 1)] != code)).sum())
        kp = dif <= e                                                          # :189
        keep.append(kp)
        if kp:
            c2[code, cols] += 1; rend = max(rend, o + L)
    nk = sum(keep)
    new = [(r << 32) | (o << 1) | d for r, o, d in zip(rids, offs, ds)]
    if not nk:
        return keep, new, 0, b""
    cov = c2.sum(axis=0)[:ref_len] > 0
    sv = int(np.argmax(cov)) if cov.any() else ref_len
    second, _ = _majority(c2)
    return keep, new, sv, ACGT[second[sv:rend]].tobytes()


def construct_ref_detail(reads, members, L, k, e):
    """_construct_ref with the counting done on whole arrays (one bincount per table instead of one numpy call per member), and with
    everything in between kept: keep [m] bool, new [m] uint64, sv, ref bytes, and c1 / c2 [4][2L], first [2L], ref_len, dif [m], offs [m]."""
    y = np.asarray(members, dtype=np.uint64)
    rid = (y >> np.uint64(32)).astype(np.int64)
    low = (y & np.uint64(0xFFFFFFFF)).astype(np.int64)
    pos, d = low >> 1, low & 1
    al = np.where(d == 1, L - pos + k - 2, pos)
    offs = al[0] - al
    TL = 2 * L
    rows = reads[rid]
    rows = np.where(d[:, None] == 1, COMP[rows][:, ::-1], rows)
    code = ((rows >> 1) ^ (rows >> 2)).astype(np.int64) & 3
    cols = offs[:, None] + np.arange(L)[None, :]
    c1 = np.bincount((code * TL + cols).ravel(), minlength=4 * TL).reshape(4, TL)
    first, mx = _majority(c1)
    ref_len = int(np.argmax(mx == 0)) if (mx == 0).any() else TL
    dif = ((cols >= ref_len) | (first[np.minimum(cols, TL - 1)] != code)).sum(axis=1)
    keep = dif <= e                                                            # :189
    c2 = np.bincount((code[keep] * TL + cols[keep]).ravel(), minlength=4 * TL).reshape(4, TL)
    new = (rid.astype(np.uint64) << np.uint64(32)) | (offs.astype(np.uint64) << np.uint64(1)) | d.astype(np.uint64)
    out = SimpleNamespace(keep=keep, new=new, sv=0, ref=b"", c1=c1, c2=c2, first=first, ref_len=ref_len, dif=dif, offs=offs, second=None)
    if keep.any():
        rend = int(offs[keep].max()) + L
        cov = c2.sum(axis=0)[:ref_len] > 0
        out.sv = int(np.argmax(cov)) if cov.any() else ref_len
        out.second, _ = _majority(c2)
        out.ref = ACGT[out.second[out.sv:rend]].tobytes()
    return out


def construct_ref_vec(reads, members, L, k, e):
    """The four results of _construct_ref from construct_ref_detail: (keep [m] bool, new [m] uint64, sv, consensus bytes)."""
    r = construct_ref_detail(reads, members, L, k, e)
    return r.keep, r.new, r.sv, r.ref


def construct_ref2_cols(reads, members, L):
    """construct_ref2 (kthread_cb.c:105-218) as column counts: members (rid << 32 | offset << 1 | dir) laid at their offsets, majority per
    column, up to the last member's end.  Returns (consensus bytes, counts [4][len])."""
    y = np.asarray(members, dtype=np.uint64)
    rid = (y >> np.uint64(32)).astype(np.int64)
    low = (y & np.uint64(0xFFFFFFFF)).astype(np.int64)
    off, d = low >> 1, low & 1
    rows = reads[rid]
    rows = np.where(d[:, None] == 1, COMP[rows][:, ::-1], rows)
    code = ((rows >> 1) ^ (rows >> 2)).astype(np.int64) & 3
    cnt = np.zeros((4, int(off.max()) + L), dtype=np.int64)
    np.add.at(cnt, (code, off[:, None] + np.arange(L)[None, :]), 1)
    return ACGT[_majority(cnt)[0]].tobytes(), cnt


def stack(L, k, spec, src=None, rid0=0):
    """One minimizer group laid over one source string of 2L bases (src, ASCII; default: a fixed random one with T on the shared
    k-mer's columns L-k .. L-1).  spec: per member (o, d, overrides): the member is src[o : o + L] (0 <= o <= L - k, so that the
    k-mer lies inside it) with src column c replaced by "ACGT"[b] for every (c, b) of overrides, and is stored reverse-complemented
    when d = 1.  The record is what mcom_sort_group hands over (see _make_groups in test_gpu_merge.py): aligned position
    al = (L-1) - o, pos = al for d = 0 and L - al + k - 2 for d = 1; members in cmpcluster's order, al descending, then rid.
    Consensus columns are source columns minus the smallest o.  Returns (reads [n][L] in spec order: member i is read rid0 + i,
    members [n] uint64)."""
    if src is None:
        src = ACGT[np.random.default_rng(1000 * L + k).integers(0, 4, 2 * L)].copy()
        src[L - k:L] = ord("T")
    src = np.asarray(src, dtype=np.uint8)
    assert src.shape == (2 * L,)
    n = len(spec)
    o = np.array([s[0] for s in spec], dtype=np.int64)
    d = np.array([s[1] for s in spec], dtype=np.int64)
    assert n and o.min() >= 0 and o.max() <= L - k and set(np.unique(d).tolist()) <= {0, 1}
    rows = src[o[:, None] + np.arange(L)[None, :]]
    for i, s in enumerate(spec):
        for c, b in s[2]:
            assert o[i] <= c < o[i] + L, (i, c)
            rows[i, c - o[i]] = ACGT[b]
    al = (L - 1) - o
    pos = np.where(d == 1, L - al + k - 2, al)
    order = np.lexsort((np.arange(n), -al))                                     # al descending, then rid
    reads = np.where(d[:, None] == 1, COMP[rows][:, ::-1], rows)
    rid = (rid0 + np.arange(n)).astype(np.uint64)
    members = (rid << np.uint64(32)) | (pos.astype(np.uint64) << np.uint64(1)) | d.astype(np.uint64)
    return np.ascontiguousarray(reads), members[order]
