"""The independent statement of `minicom -a Q[:C]`, shared by tests/test_agree.py (host twins) and
tests/test_gpu_agree.py (device): the mask from explicit placements, a pure-Python parser of the stream files written from DESIGN.md
section 3.5, the transform with its report, and hand-made archives whose truth is known by construction.  Nothing here calls the C++."""
import functools

import numpy as np

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s: str) -> str:
    return "".join(COMP.get(c, "N") for c in reversed(s))


# ---- the mask from explicit placements ------------------------------------------------------------------------------------------------------
def mask_of(contigs, members, L, C):
    """contigs: strings of one stream set; members: (contig index, begin position, direction bit, decoded read) -- the read as the decoder
    writes it.  Returns bool [len(members), L]: column i agrees with the contig base it is aligned to and at least C members cover it."""
    cov = [np.zeros(len(c) + 1, np.int64) for c in contigs]
    for c, pos, _, _ in members:
        cov[c][pos] += 1; cov[c][pos + L] -= 1
    cov = [np.cumsum(v)[:-1] for v in cov]
    out = np.zeros((len(members), L), bool)
    for j, (c, pos, rev, read) in enumerate(members):
        assert len(read) == L
        for i in range(L):
            place = pos + L - 1 - i if rev else pos + i
            base = contigs[c][place]
            if rev:
                base = COMP[base]
            out[j, i] = read[i] == base and cov[c][place] >= C
    return out


def pack_mask(bits):
    """bool [n, L] -> uint8 [n, ceil(L / 8)], column i in bit i & 7 of byte i >> 3"""
    bits = np.asarray(bits, bool)
    if bits.shape[0] == 0:
        return np.zeros((0, (bits.shape[1] + 7) // 8), np.uint8)
    return np.packbits(bits, axis=1, bitorder="little")


def unpack_mask(packed, L):
    packed = np.asarray(packed, np.uint8)
    if packed.shape[0] == 0:
        return np.zeros((0, L), bool)
    return np.unpackbits(packed, axis=1, bitorder="little")[:, :L].astype(bool)


# ---- the transform ------------------------------------------------------------------------------------------------------------------------------
def transform(rows, mask_bits, Q):
    """rows uint8 [n, L], mask_bits bool [n, L] -> (new rows, report)"""
    rows = np.asarray(rows, np.uint8)
    out = rows.copy()
    out[mask_bits] = 33 + Q
    d = np.abs(out.astype(np.int64) - rows.astype(np.int64))
    return out, {"changed": int((d != 0).sum()), "sum_abs": int(d.sum()), "sum_sq": int((d * d).sum()), "max_abs": int(d.max()) if d.size else 0,
                 "mask_bits": int(np.asarray(mask_bits).sum())}


# ---- a parser of the stream files -------------------------------------------------------------------------------------
def _unpack2(b, n=None):
    """2 bits per base, low bits first"""
    a = np.frombuffer(b, np.uint8)
    codes = np.stack([(a >> s) & 3 for s in (0, 2, 4, 6)], axis=1).reshape(-1)
    s = "".join("ACGT"[c] for c in (codes if n is None else codes[:n]))
    return s


def _line(text, window):
    """digits: a run of bases taken from the window; a letter: a literal; the missing tail is the window's"""
    out, run = [], 0
    for ch in text.decode():
        if ch.isdigit():
            run = run * 10 + int(ch)
        else:
            out.extend(window[len(out):len(out) + run]); run = 0
            out.append(ch)
    out.extend(window[len(out):])
    assert len(out) == len(window), (text, len(out))
    return "".join(out)


def _ids(b):
    return np.cumsum(np.frombuffer(b, "<u4").astype(np.int64))


def parse_folder(d, C):
    """d: a folder of stream files, default mode or -p (ids.bin.0 present).  Returns (reads: list of str in the decoder's row order,
    mask bool [n, L], member rows: the rows of contig members)."""
    rd = lambda name: (d / name).read_bytes()
    info = (d / "info.txt").read_text().split()
    L, nth, na, nt, nn = (int(x) for x in info[:5])
    order = (d / "ids.bin.0").exists()
    rows = []                                                   # (row or None, read, mask row)
    zero = np.zeros(L, bool)

    def lst(reads, ids):
        for k, r in enumerate(reads):
            rows.append((int(ids[k]) if order else None, r, zero))

    for base, cnt, name in (("A", na, "allA"), ("T", nt, "allT"), ("N", nn, "allN")):
        lst([base * L] * cnt, _ids(rd(name + ".ids.bin")) if order else None)
    for base, name in (("A", "AA"), ("T", "TT"), ("N", "NN")):
        lst([_line(t, base * L) for t in rd(name + ".txt").split(b"\n")[:-1]], _ids(rd(name + ".ids.bin")) if order else None)
    nlines = [t.decode() for t in rd("single_N.seq").split(b"\n")[:-1]]
    sb = rd("single.seq")
    n_single = len(sb) * 4 // L
    sids = _ids(rd("singleFile.ids.bin")) if order else None
    if order:
        n_single = min(n_single, len(sids))
    bases = _unpack2(sb)
    singles = [bases[k * L:(k + 1) * L] for k in range(n_single)]
    if order:
        lst(singles, sids); lst(nlines, _ids(rd("Nfile.ids.bin")))
    else:
        lst(nlines, None); lst(singles, None)
    member_rows = []
    for t in range(nth):
        bpos, ref, dirb, dif = rd("beg_pos.bin.%d" % t), _unpack2(rd("ref.bin.%d" % t)), np.frombuffer(rd("dir.bin.%d" % t), np.uint8), rd("dif_char.txt.%d" % t).split(b"\n")
        ids = np.frombuffer(rd("ids.bin.%d" % t), "<u4") if order else None
        contigs, members, dest = [], [], []
        at, q, used = 0, 0, 0
        while at + 4 <= len(bpos):
            num = int(np.frombuffer(bpos[at:at + 4], "<u4")[0]); at += 4
            deltas = np.frombuffer(bpos[at:at + 2 * num], "<u2").astype(np.int64); at += 2 * num
            pos = np.cumsum(deltas)
            clen = int(pos[-1]) + L if num else 0
            contig = ref[used:used + clen]; used += clen
            assert len(contig) == clen
            contigs.append(contig)
            prev = 0
            for k in range(num):
                p = int(pos[k])
                rev = int((dirb[q >> 3] >> (q & 7)) & 1) if (q >> 3) < len(dirb) else 0
                read = _line(dif[q], contig[p:p + L])
                if rev:
                    read = revcomp(read)
                if order:
                    i = int(ids[q])
                    if deltas[k] == 0:
                        i = (i + prev) & 0xFFFFFFFF
                    prev = i
                    dest.append(i)
                members.append((len(contigs) - 1, p, rev, read))
                q += 1
        m = mask_of(contigs, members, L, C)                     # coverage never crosses stream sets
        for k, (_, _, _, read) in enumerate(members):
            rows.append((dest[k] if order else None, read, m[k]))
            member_rows.append(dest[k] if order else len(rows) - 1)
    n = len(rows)
    if order:
        assert sorted(r[0] for r in rows) == list(range(n))
        rows.sort(key=lambda r: r[0])
    return [r[1] for r in rows], (np.stack([r[2] for r in rows]) if n else np.zeros((0, L), bool)), np.asarray(member_rows, np.int64)


# ---- hand-made archives ---------------------------------------------------------------------------------------------------------------------------
def _pack2(s):
    codes = np.array(["ACGT".index(c) for c in s] + [0] * ((-len(s)) % 4), np.uint8).reshape(-1, 4)
    return (codes[:, 0] | (codes[:, 1] << 2) | (codes[:, 2] << 4) | (codes[:, 3] << 6)).astype(np.uint8).tobytes()


def _dif(literals, force_zero=False):
    """(column, letter) in ascending columns -> the line: the run in front of a literal as a decimal number (left out when zero)"""
    if not literals:
        return b"0" if force_zero else b""
    out, at = "", 0
    for col, ch in literals:
        if col > at:
            out += str(col - at)
        out += ch; at = col + 1
    return out.encode()


def _other(base, k):
    return [b for b in "ACGT" if b != base][k % 3]


class Set:
    """one stream set in the making: contigs as strings, members as (contig, pos, rev, literals, force_zero)"""
    def __init__(self):
        self.contigs, self.members = [], []


def _patterns(L, window, k):
    """the k-th edit pattern of a member, as literals in WINDOW coordinates"""
    k %= 9
    if k == 0: return [], False                                                        # an empty line
    if k == 1: return [], True                                                         # the line `0`
    if k == 2: return [(0, _other(window[0], 1))], False                               # a literal in the first column
    if k == 3: return [(L - 1, _other(window[L - 1], 2))], False                       # ... in the last one, behind a multi-digit run
    if k == 4: return [(L // 2, "N")], False                                           # an N
    if k == 5: return [(L // 3, window[L // 3])], False                                # a literal that equals the window base
    if k == 6: return [(11, _other(window[11], 0)), (12, _other(window[12], 1)), (L - 2, _other(window[L - 2], 2))], False
    if k == 7: return [(0, "N"), (L - 1, window[L - 1])], False
    return [(7, _other(window[7], 0))], False


@functools.lru_cache(maxsize=None)
def hand_made_sets(L, n_members, seed=1, second_set=False):
    """The stream sets of one hand-made archive with n_members members in the first set:
       contig 0: L + 130 bases, members at 0, 0, 7, 123, 130 -- coverage steps inside a read; contig 1: one member; contig 2: no member;
       contig 3: the rest, a few bases apart, in both directions.  second_set: a second set whose single contig starts where contig 0 of the
       first does -- its lone member would look covered if coverage leaked from one set into the next."""
    rng = np.random.default_rng(seed * 1000 + L)
    rnd = lambda n: "".join("ACGT"[c] for c in rng.integers(0, 4, n))
    s = Set()
    s.contigs.append(rnd(L + 130))
    for k, pos in enumerate((0, 0, 7, 123, 130)):
        s.members.append((0, pos, k & 1, k))
    s.contigs.append(rnd(L)); s.members.append((1, 0, 1, 6))
    s.contigs.append("")
    rest = n_members - len(s.members)
    assert rest >= 1
    pos = np.concatenate([[0], np.cumsum(rng.integers(0, 21, rest - 1))]).astype(int)
    s.contigs.append(rnd(int(pos[-1]) + L))
    for k in range(rest):
        s.members.append((3, int(pos[k]), int(rng.integers(0, 2)), k + 2))
    sets = [s]
    if second_set:
        t = Set(); t.contigs.append(rnd(L)); t.members.append((0, 0, 0, 0)); sets.append(t)
    return tuple(sets)


def _member_read(s, L, m):
    c, pos, rev, k = m
    window = s.contigs[c][pos:pos + L]
    lits, force = _patterns(L, window, k)
    read = list(window)
    for col, ch in lits:
        read[col] = ch
    read = "".join(read)
    return (revcomp(read) if rev else read), _dif(lits, force)


def write_hand_made(d, L, n_members, order, seed=1, second_set=False):
    """Writes the archive into the new folder d and returns (reads in the decoder's row order, truth(C) -> bool [n, L], rows of contig members).
    The lists: one counted read of each kind, two near-constant lines, one N read, two unclustered reads -- all rows of zeros."""
    rng = np.random.default_rng(seed * 7 + L + n_members)
    sets = hand_made_sets(L, n_members, seed, second_set)
    d.mkdir()
    lists = [("allA", ["A" * L], None), ("allT", ["T" * L], None), ("allN", ["N" * L], None),
             ("AA", ["A" * (L - 1) + "C"], b"%dC\n" % (L - 1)), ("TT", ["G" + "T" * (L - 1)], b"G\n"), ("NN", [], b"")]
    n_read = "ACGTN" * (L // 5) + "A" * (L % 5)
    singles = ["".join("ACGT"[c] for c in rng.integers(0, 4, L)) for _ in range(2)]
    reads = [r for _, rs, _ in lists for r in rs]
    reads += (singles + [n_read]) if order else ([n_read] + singles)
    n_lists = len(reads)
    per_set = []
    for s in sets:
        decoded = [_member_read(s, L, m) for m in s.members]
        per_set.append(decoded)
        reads += [r for r, _ in decoded]
    n = len(reads)
    perm = rng.permutation(n) if order else np.arange(n)                            # stream position -> row
    (d / "info.txt").write_text("%d %d 1 1 1%s\n" % (L, len(sets), " %d" % n if order else ""))
    at = 0

    placed = [None] * n

    def id_list(name, rs):
        """the next len(rs) stream positions: a list is sorted by id and delta coded"""
        nonlocal at
        ids = np.sort(perm[at:at + len(rs)]); at += len(rs)
        if order:
            (d / name).write_bytes(np.diff(np.concatenate([[0], ids])).astype("<u4").tobytes())
            for r, i in zip(rs, ids):
                placed[i] = r

    for name, rs, text in lists:
        if text is not None:
            (d / (name + ".txt")).write_bytes(text)
        id_list(name + ".ids.bin", rs)
    (d / "single.seq").write_bytes(_pack2("".join(singles)))
    (d / "single_N.seq").write_bytes(n_read.encode() + b"\n")
    id_list("singleFile.ids.bin", singles)
    id_list("Nfile.ids.bin", [n_read])
    member_rows, placements = [], []
    for t, (s, decoded) in enumerate(zip(sets, per_set)):
        bpos, dirbits, dif, idw = bytearray(), [], bytearray(), []
        q = 0
        rows_t = []
        for c in range(len(s.contigs)):
            ms = [(m, dr) for m, dr in zip(s.members, decoded) if m[0] == c]
            bpos += np.uint32(len(ms)).tobytes()
            prev_pos, prev_id = 0, 0
            for j, ((_, pos, rev, _), (read, line)) in enumerate(ms):
                bpos += np.uint16(pos - prev_pos).tobytes()
                dirbits.append(rev); dif += line + b"\n"
                row = int(perm[at]) if order else at
                at += 1
                if order:
                    # a member that begins where the one before it does carries the difference of the two ids (mod 2^32), every other its id
                    idw.append((row - prev_id) & 0xFFFFFFFF if j and pos == prev_pos else row)
                    prev_id = row
                    placed[row] = read
                prev_pos = pos
                rows_t.append(row)
                q += 1
        (d / ("beg_pos.bin.%d" % t)).write_bytes(bytes(bpos))
        (d / ("ref.bin.%d" % t)).write_bytes(_pack2("".join(s.contigs)))
        (d / ("dir.bin.%d" % t)).write_bytes(np.packbits(np.array(dirbits, np.uint8), bitorder="little").tobytes())
        (d / ("dif_char.txt.%d" % t)).write_bytes(bytes(dif))
        if order:
            (d / ("ids.bin.%d" % t)).write_bytes(np.array(idw, "<u4").tobytes())
        member_rows.append(rows_t)
        placements.append([(m[0], m[1], m[2], dr[0]) for m, dr in zip(s.members, decoded)])
    assert at == n
    out_reads = placed if order else reads
    assert all(r is not None for r in out_reads)

    def truth(C):
        bits = np.zeros((n, L), bool)
        for s, rows_t, pl in zip(sets, member_rows, placements):
            m = mask_of(s.contigs, pl, L, C)
            # mask_of takes the members in any order; the rows were handed out contig by contig
            by_contig = [k for c in range(len(s.contigs)) for k, mm in enumerate(s.members) if mm[0] == c]
            for row, k in zip(rows_t, by_contig):
                bits[row] = m[k]
        return bits

    return out_reads, truth, np.array([r for rows_t in member_rows for r in rows_t], np.int64), n_lists


HAND_L = (37, 40, 41, 150, 256)
HAND_MEMBERS = (15, 16, 17, 33)
HAND_C = (1, 2, 3, 4, 255)
