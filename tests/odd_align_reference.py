"""`minicom -p -V -A` restated in plain Python: the yardstick of tests/test_odd_align.py and tests/test_gpu_odd_align.py.

The rule: a dict of the grid's K-mers, brute force over both orientations and every offset; the member odd.aln written and read field by
field; and the cases.  Hits and member bytes of the twins and of the kernels must EQUAL what this module gives."""
import random
import struct
import zlib

K, G, M = 24, 8, 16
MIN_LEN = K + G - 1
NONE = (1 << 64) - 1
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def budget(l):
    return (l - 24) // 8


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


# ---- T: the bases of ref.bin images, 4 per byte, low bits first ----
def image(bases: str) -> bytes:
    out = bytearray((len(bases) + 3) // 4)
    for i, c in enumerate(bases):
        out[i >> 2] |= "ACGT".index(c) << (2 * (i & 3))
    return bytes(out)


def text_of(refs) -> str:
    """refs: (image, bases taken from it) per stream set"""
    return "".join("ACGT"[(img[i >> 2] >> (2 * (i & 3))) & 3] for img, n in refs for i in range(n))


def grid_of(T: str) -> dict:
    g = {}
    for q in range(0, len(T) - K + 1, G):
        g.setdefault(T[q:q + K], []).append(q)
    return g


def align(T: str, grid: dict, read: str) -> int:
    l = len(read)
    if l < MIN_LEN:
        return NONE
    best = NONE
    for s in (0, 1):
        r = revcomp(read) if s else read
        for o in range(l - K + 1):
            kmer = r[o:o + K]
            if "N" in kmer:
                continue
            places = grid.get(kmer, ())
            if len(places) > M:
                continue
            for q in places:
                p = q - o
                if p < 0 or p + l > len(T):
                    continue
                d = sum(1 for a, b in zip(r, T[p:p + l]) if a != b)
                if d <= budget(l):
                    best = min(best, d << 48 | s << 40 | p)
    return best


def align_all(T: str, reads) -> list:
    grid = grid_of(T)
    return [align(T, grid, r) for r in reads]


# ---- the member ----
def _bits(flags) -> bytes:
    out = bytearray((len(flags) + 7) // 8)
    for j, f in enumerate(flags):
        if f:
            out[j >> 3] |= 1 << (j & 7)
    return bytes(out)


def encode(T: str, reads, hits):
    """(member bytes -- b"" when no read is aligned --, residual bytes)"""
    full = "".join(reads).encode()
    aligned = [h != NONE for h in hits]
    if not any(aligned):
        return b"", full
    strand, ps, ds, offs, bases = [], [], [], [], []
    for r, h in zip(reads, hits):
        if h == NONE:
            continue
        d, s, p = h >> 48, (h >> 40) & 1, h & ((1 << 40) - 1)
        win = T[p:p + len(r)]
        win = revcomp(win) if s else win                     # the window in the read's own orientation
        mm = [j for j in range(len(r)) if r[j] != win[j]]
        assert len(mm) == d
        strand.append(s); ps.append(p); ds.append(d)
        offs += [j if k == 0 else j - mm[k - 1] - 1 for k, j in enumerate(mm)]
        bases += [ord(r[j]) for j in mm]
    residual = "".join(r for r, h in zip(reads, hits) if h == NONE).encode()
    head = b"MCOMOAL1" + struct.pack("<IIII", K, G, M, zlib.crc32(full)) + struct.pack("<QQQQQ", len(reads), len(ps), len(T), sum(ds), len(residual))
    planes = b"".join(bytes((p >> (8 * b)) & 255 for p in ps) for b in range(5))
    return head + _bits(aligned) + _bits(strand) + planes + bytes(ds) + bytes(offs) + bytes(bases), residual


def decode(member: bytes, T: str, residual: bytes, lengths) -> bytes:
    """the full odd text of a GOOD member (the refusals are the twins' to make: here anything odd is an AssertionError)"""
    assert member[:8] == b"MCOMOAL1" and struct.unpack_from("<III", member, 8) == (K, G, M)
    crc, = struct.unpack_from("<I", member, 20)
    n_odd, n_al, t_len, n_mm, res = struct.unpack_from("<QQQQQ", member, 24)
    assert n_odd == len(lengths) and t_len == len(T) and res == len(residual)
    at = 64
    ab = member[at:at + (n_odd + 7) // 8]; at += len(ab)
    sb = member[at:at + (n_al + 7) // 8]; at += len(sb)
    planes = [member[at + b * n_al:at + (b + 1) * n_al] for b in range(5)]; at += 5 * n_al
    ds = member[at:at + n_al]; at += n_al
    offs = member[at:at + n_mm]; at += n_mm
    bases = member[at:at + n_mm]; at += n_mm
    assert at == len(member)
    out, a, m, ro = [], 0, 0, 0
    for j, l in enumerate(lengths):
        if not (ab[j >> 3] >> (j & 7)) & 1:
            out.append(residual[ro:ro + l].decode()); ro += l
            continue
        p = sum(planes[b][a] << (8 * b) for b in range(5))
        s = (sb[a >> 3] >> (a & 7)) & 1
        assert l >= MIN_LEN and p + l <= len(T) and ds[a] <= budget(l)
        r = list(revcomp(T[p:p + l]) if s else T[p:p + l])
        pos = 0
        for k in range(ds[a]):
            pos = offs[m] if k == 0 else pos + 1 + offs[m]
            assert pos < l and chr(bases[m]) in "ACGTN" and r[pos] != chr(bases[m])
            r[pos] = chr(bases[m]); m += 1
        out.append("".join(r)); a += 1
    text = "".join(out).encode()
    assert a == n_al and m == n_mm and ro == len(residual) and zlib.crc32(text) == crc
    return text


# ---- the cases ----
def rand_bases(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def mutate(read, places):
    r = list(read)
    for j in places:
        r[j] = "ACGT"[("ACGT".index(r[j]) + 1) % 4]
    return "".join(r)


def hit(d, s, p):
    return d << 48 | s << 40 | p


def cases():
    """(name, refs, reads, expected hit words or None where the case states none)"""
    rng = random.Random(20)
    T = rand_bases(rng, 4096)
    one = [(image(T), len(T))]
    out = []
    out.append(("lengths", one, [T[100:100 + l] for l in (30, 31, 32, 255, 256)], [NONE] + [hit(0, 0, 100)] * 4))
    out.append(("ends_of_T", one, [T[:50], T[-50:], revcomp(T[:50]), revcomp(T[-50:])], [hit(0, 0, 0), hit(0, 0, 4046), hit(0, 1, 0), hit(0, 1, 4046)]))
    # two stream sets, the first ending in the middle of a byte: its image's padding bits are not bases of T
    two = [(image(T[:1001]), 1001), (image(T[1001:]), 3095)]
    assert text_of(two) == T
    out.append(("across_sets", two, [T[980:1040], T[1001:1060], T[940:1001]], [hit(0, 0, 980), hit(0, 0, 1001), hit(0, 0, 940)]))
    # the only clean seed of the read at every o % 8: 31 bases hold one grid place; 64 bases with the other grid seeds broken
    reads, want = [], []
    for r in range(8):
        p = 200 + r
        o0 = -p % 8
        reads += [T[p:p + 31], mutate(T[p:p + 64], [o0 + 24, o0 + 48])]
        want += [hit(0, 0, p), hit(2, 0, p)]
    out.append(("one_clean_seed", one, reads, want))
    out.append(("first_and_last_base", one, [mutate(T[300:380], [0]), mutate(T[300:380], [79]), revcomp(mutate(T[300:380], [0, 79]))], [hit(1, 0, 300), hit(1, 0, 300), hit(2, 1, 300)]))
    seven = [30, 35, 40, 45, 50, 55, 60]
    out.append(("budget", one, [mutate(T[304:384], seven), mutate(T[304:384], seven + [65])], [hit(7, 0, 304), NONE]))
    # a seed with exactly M and with M + 1 grid places: the read's only grid seed is R
    for copies in (M, M + 1):
        t = list(rand_bases(rng, 4096))
        R = rand_bases(rng, K)
        for k in range(copies):
            q = 80 + 8 * 29 * k
            t[q:q + K] = R
        t = "".join(t)
        out.append(("seed_%d_places" % copies, [(image(t), len(t))], [t[77:77 + 31]], [hit(0, 0, 77) if copies == M else NONE]))
    S = rand_bases(rng, 40)
    t = T[:400] + S + T[440:1200] + S + T[1240:]
    out.append(("tie_smaller_p", [(image(t), len(t))], [S], [hit(0, 0, 400)]))
    t = T[:400] + revcomp(S) + T[440:1200] + S + T[1240:]
    out.append(("tie_strand_0", [(image(t), len(t))], [S], [hit(0, 0, 1200)]))
    X = rand_bases(rng, 20)
    t = T[:800] + X + revcomp(X) + T[840:]
    out.append(("palindrome", [(image(t), len(t))], [X + revcomp(X)], [hit(0, 0, 800)]))
    r64 = T[1600:1664]
    n_out = r64[:60] + "N" + r64[61:]
    n_in = r64[:20] + "N" + r64[21:44] + "N" + r64[45:]
    out.append(("N_in_the_read", one, [n_out, n_in, revcomp(n_out)], [hit(1, 0, 1600), NONE, hit(1, 1, 1600)]))
    out.append(("random_read", one, [rand_bases(rng, 100)], [NONE]))
    short = rand_bases(rng, 20)
    out.append(("T_below_K", [(image(short), 20)], [rand_bases(rng, 40), short + short], [NONE, NONE]))
    out.append(("no_odd_records", one, [], []))
    out.append(("all_aligned", one, [T[100:160], revcomp(T[200:300])], [hit(0, 0, 100), hit(0, 1, 200)]))
    out.append(("none_aligned", one, [rand_bases(rng, 60), "ACGT"], [NONE, NONE]))
    # more than one workgroup: trimmed reads of either strand with a few substitutions and Ns, random reads and short ones among them
    reads = []
    for i in range(301):
        kind = i % 7
        if kind == 5:
            reads.append(rand_bases(rng, rng.randrange(1, 257)))
            continue
        l = rng.randrange(1, 31) if kind == 6 else rng.randrange(31, 257)
        p = rng.randrange(0, len(T) - l + 1)
        r = mutate(T[p:p + l], rng.sample(range(l), min(l, rng.randrange(0, 4))))
        if rng.random() < 0.1:
            j = rng.randrange(l); r = r[:j] + "N" + r[j + 1:]
        reads.append(revcomp(r) if rng.random() < 0.5 else r)
    out.append(("mixed_301", two, reads, None))
    return out


def case_ids():
    return [c[0] for c in cases()]


def offsets(reads):
    off = [0]
    for r in reads:
        off.append(off[-1] + len(r))
    return off
