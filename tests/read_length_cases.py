"""Shared inputs of the read-length tests (test_read_length_cases.py on the CPU, test_gpu_read_lengths.py on the device).  No GPU here.

Read length L (1 ... 256) selects W = ceil(L / 32) packed words per read and with it one of eight instantiations of most hot-path
kernels.  SWEEP holds the first, an interior and the last length of every word count; class_rows() holds one directed row for every
rule of the read classification (kthread_reads.c:84-224) at its boundary."""
import itertools

import numpy as np

# classes of include/mcom.h
SKETCH, ALLA, ALLT, ALLN, NEARA, NEART, NEARN, NHEAVY = range(8)

# 32W-31, 32W-13 (no multiple of 16: the 16-byte paths have a tail), 32W for W = 1 ... 8
SWEEP = [L for W in range(1, 9) for L in (32 * W - 31, 32 * W - 13, 32 * W)]

N_POSITIONS = (0, 31, 32, 63, 64, 127, 128)          # word boundaries of the packed row (32 bases) and of the N mask (64 flags)
TIE_ORDER = "ATGC"                                   # kthread_reads.c:185-201: the first of equal counts wins, in this order


def ks(L):
    """Both sides of the wide / narrow switch at k = 17 and both parities; for L < 31 k = L comes first (a read of one k-mer)."""
    out = [k for k in (31, 30, 17, 16, 15, 8) if k <= L]
    if L < 31 and L not in out:
        out.insert(0, L)
    return out


def n_heavy(cn, L):
    """kthread_reads.c:182: a read is kept while cN <= 0.4 L, in double arithmetic."""
    return not (float(cn) <= 0.4 * float(L))


def _row(s):
    return np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), dtype=np.uint8).copy()


def _random_read(rng, L):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, L)].copy()


def class_rows(L, e):
    """Directed rows over ACGTN: a list of (name, row uint8 [L], class, rep).  class is the class the row is built for; rep is the
    base every N of a kept row must turn into where the construction fixes it (else None).  A row that cannot be built at this
    (L, e) is left out."""
    rng = np.random.default_rng(1000 * L + e)
    rows = []

    def add(name, row, cls, rep=None):
        row = _row(row) if not isinstance(row, np.ndarray) else row
        assert row.shape == (L,)
        rows.append((name, row, cls, rep))

    add("all_A", "A" * L, ALLA)
    add("all_T", "T" * L, ALLT)
    add("all_N", "N" * L, ALLN)
    # all-C and all-G are ordinary reads -- unless the whole read is no more than e bases, which makes it "A with <= e others" (and
    # T and N with <= e others as well: the first of the else-if chain wins)
    add("all_C", "C" * L, SKETCH if L > e else NEARA)
    add("all_G", "G" * L, SKETCH if L > e else NEARA)

    # A, T, N backgrounds with exactly e and e + 1 foreign characters.  Built only where the background keeps more than e characters of
    # its own, so that the row cannot fall into an earlier near-class.
    if L - (e + 1) > e:
        for bg, near in (("A", NEARA), ("T", NEART), ("N", NEARN)):
            for m in (e, e + 1):
                for flavour in ("bases", "partN"):
                    if bg == "N" and flavour == "partN":
                        continue                                  # an N among N is no foreign character
                    if flavour == "partN" and m < 2:
                        continue                                  # needs one N and one base
                    row = np.full(L, ord(bg), dtype=np.uint8)
                    pos = rng.choice(L, m, replace=False)
                    others = [c for c in "ACGT" if c != bg]
                    fill = [others[i % len(others)] for i in range(m)]
                    if flavour == "partN":
                        for i in range(0, m, 2):
                            fill[i] = "N"
                        if all(c == "N" for c in fill):
                            fill[-1] = others[0]
                    row[pos] = [ord(c) for c in fill]
                    cn = int((row == ord("N")).sum())
                    if m == e:
                        cls, rep = near, None
                    elif n_heavy(cn, L):
                        cls, rep = NHEAVY, None
                    elif bg == "N":
                        cls, rep = SKETCH, None
                    else:
                        cls, rep = SKETCH, (bg if cn else None)   # L - m > e + 1 > m / 3: the background is the majority
                    add("near_%s_%d_%s" % (bg, m, flavour), row, cls, rep)

    # two near-classes at once: as many T as A (or one more).  No more than e characters differ from A and no more than e from T;
    # "A with <= e others" is tested first
    if 2 <= L <= 2 * e:
        add("near_A_and_T", "T" * ((L + 1) // 2) + "A" * (L // 2), NEARA)
    if L == 1:
        add("near_A_T_and_N", "C", NEARA)

    # floor(0.4 L) and floor(0.4 L) + 1 N in an otherwise random read (enough bases left for no near-class)
    f = int(0.4 * L)
    if f >= 1 and L - (f + 1) > e and L >= 16:
        for cn in (f, f + 1):
            row = _random_read(rng, L)
            row[rng.choice(L, cn, replace=False)] = ord("N")
            add("N_%d_of_%d" % (cn, L), row, NHEAVY if n_heavy(cn, L) else SKETCH)

    # one N at a word boundary of the packed row / of the N mask
    if L >= 16:
        for p in sorted(set(q for q in N_POSITIONS + (L - 1,) if q < L)):
            row = _random_read(rng, L)
            row[p] = ord("N")
            add("N_at_%d" % p, row, SKETCH)

    # the eleven ties among the counts of A, T, G, C: the tied letters share the largest count c, every other letter has c - 1, what
    # is left of L (one to four characters) is N, so the substituted base shows which letter won
    if L >= 16:
        for size in (2, 3, 4):
            for tied in itertools.combinations(TIE_ORDER, size):
                o = 4 - size
                c = (L - 1 + o) // 4
                cnt = {b: (c if b in tied else c - 1) for b in TIE_ORDER}
                cn = L - sum(cnt.values())
                assert 1 <= cn <= 4 and not n_heavy(cn, L) and c - 1 > 0
                row = _row("".join(b * cnt[b] for b in TIE_ORDER) + "N" * cn)
                rng.shuffle(row)
                add("tie_" + "".join(tied), row, SKETCH, tied[0])
    return rows


def class_matrix(L, e):
    rows = class_rows(L, e)
    return np.stack([r for _, r, _, _ in rows]), np.array([c for _, _, c, _ in rows], dtype=np.uint8)


def directed_sketch_rows(L):
    """The palindromic and homopolymer rows of test_gpu_reads.py::test_palindromic_and_homopolymer_reads, cut or tiled to L.  With an
    even k every k-mer of (AT)n and (GC)n equals its reverse complement: no minimizer."""
    units = ("AT", "ACGT", "C", "GC", "AATT", "ACGTACGTTGCA")
    return np.stack([_row((u * (L // len(u) + 1))[:L]) for u in units])


def sketch_reads_for(L):
    from minicom_amd import synth
    return synth.synth_reads(900 + L, 4000, L)


def position_coverage(y, k, L):
    """(position, strand) pairs of the records y (uint64, without the empty ones) among the four extremes: k-1 and L-1, each on both strands."""
    low = (y & np.uint64(0xFFFFFFFF)).astype(np.int64)
    have = set(zip((low >> 1).tolist(), (low & 1).tolist()))
    return {(p, z) for p in (k - 1, L - 1) for z in (0, 1)} & have


def encode_byte_cases(L, n=200, extra=40):
    """n (read, contig, window position, direction) cases for encode_byte (kthread_hash_realign.c:283-314): reads cut from random
    contigs, 0 ... 12 substitutions, both strands, windows at the first and the last position of a contig among them.  Twelve
    substitutions cost at most 48 characters, which stays under 0.4 L from L = 121 on, so `extra` more cases carry L/4 ... L/2
    substitutions: both answers occur at every length.
    Returns (reads uint8 [n + extra, L], contigs list of bytes, contig int32, pos int32, dirs uint8)."""
    n_light, n = n, n + extra
    rng = np.random.default_rng(77 + L)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    comp = np.zeros(256, dtype=np.uint8); comp[[65, 67, 71, 84]] = [84, 71, 67, 65]
    contigs = [acgt[rng.integers(0, 4, int(rng.integers(L, 3 * L + 40)))] for _ in range(24)]
    contigs[0] = contigs[0][:L]                                   # a contig of one window
    reads = np.zeros((n, L), dtype=np.uint8)
    cid = rng.integers(0, len(contigs), n).astype(np.int32)
    pos = np.zeros(n, dtype=np.int32); dirs = (rng.integers(0, 2, n)).astype(np.uint8)
    for i in range(n):
        c = contigs[cid[i]]
        last = len(c) - L
        pos[i] = (0, last, int(rng.integers(0, last + 1)))[i % 3]
        r = c[pos[i]:pos[i] + L].copy()
        subs = i % 13 if i < n_light else int(rng.integers(L // 4, L // 2 + 1))
        for q in rng.choice(L, subs, replace=False):
            r[q] = acgt[(int(np.flatnonzero(acgt == r[q])[0]) + 1 + int(rng.integers(0, 3))) % 4]
        reads[i] = comp[r][::-1] if dirs[i] else r
    return reads, [c.tobytes() for c in contigs], cid, pos, dirs
