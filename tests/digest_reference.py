"""The digest of DESIGN.md section 3.18 in plain Python integers: the reference for the device calls (csrc/digest.hip), their host twin
(host/mcom_digest.cpp) and the bytes of digest.txt.  Records are (name, sequence, plus text, qualities), all bytes, as in
tests/ragged_cases.py, whose makers the cases here use.

A line is the bytes of a FASTQ line without its newline and without the leading '@' / '+'.  Everything is mod 2^64 and computed once per
seed, so every value here is a pair."""
import random

import ragged_cases as rc

M = (1 << 64) - 1
SEEDS = (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F)
KEYS = ("seq.ordered.1", "qual.ordered.1", "name.ordered.1", "seq.ordered.2", "qual.ordered.2", "name.ordered.2", "seq.multiset", "rec.multiset")
F_NAME, F_PLUS, F_LENGTH, F_LONG = 1, 2, 4, 16          # MCOM_FASTQ_F_* of include/mcom.h
GROUP = rc.GROUP                                         # records per workgroup of the record kernel
REDUCE_BLOCK = 2048                                      # records per workgroup of the reduction


def mix(x):
    x &= M
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M
    x ^= x >> 31
    return x


def H(line: bytes):
    m = len(line)
    out = []
    for K in SEEDS:
        s = 0
        for j in range((m + 7) // 8):
            w = int.from_bytes(line[8 * j:8 * j + 8], "little")
            s += mix(w ^ mix(K + j))
        out.append(mix(s + m))
    return tuple(out)


def C(x, y):
    return tuple(mix(x[s] + mix(y[s] + K)) for s, K in enumerate(SEEDS))


def record_hashes(rec):
    """(hS, hQ, hN) of one record"""
    n, s, p, q = rec
    return H(s), H(q), C(H(n), H(p))


def ordered(hs):
    return tuple(sum(mix(h[s] + (i + 1) * K) for i, h in enumerate(hs)) & M for s, K in enumerate(SEEDS))


def multiset(rs):
    return tuple(sum(mix(r[s]) for r in rs) & M for s in range(2))


def sums(recs1, recs2=None, with_qual=True, with_names=True):
    """{key: (word, word)} of one file or of a pair, the keys the printer would write"""
    out = {}
    files = [recs1] if recs2 is None else [recs1, recs2]
    hashes = [[record_hashes(r) for r in recs] for recs in files]
    for f, hs in enumerate(hashes, 1):
        out["seq.ordered.%d" % f] = ordered([h[0] for h in hs])
        if with_qual:
            out["qual.ordered.%d" % f] = ordered([h[1] for h in hs])
        if with_names:
            out["name.ordered.%d" % f] = ordered([h[2] for h in hs])
    if recs2 is None:
        out["seq.multiset"] = multiset([h[0] for h in hashes[0]])
        if with_qual:
            out["rec.multiset"] = multiset([C(h[0], h[1]) for h in hashes[0]])
    else:
        out["seq.multiset"] = multiset([C(a[0], b[0]) for a, b in zip(*hashes)])
        if with_qual:
            out["rec.multiset"] = multiset([C(C(a[0], a[1]), C(b[0], b[1])) for a, b in zip(*hashes)])
    return out


def digest_text(recs1, recs2=None, with_qual=True, with_names=True) -> str:
    s = sums(recs1, recs2, with_qual, with_names)
    t = "minicom-digest 1\nfiles %d\nn %d\n" % (1 if recs2 is None else 2, len(recs1))
    for k in KEYS:
        if k in s:
            t += "%s %016x %016x\n" % (k, s[k][0], s[k][1])
    return t


def sums16(s):
    """the sixteen words of the reduce calls from a dict of sums (0 where a key is absent)"""
    out = []
    for k in KEYS:
        out += list(s.get(k, (0, 0)))
    return out


def flags_of(rec):
    """the flag bits of a record as the record kernel sets them (0: a good record)"""
    n, s, p, q = rec
    bad = 0
    if len(s) != len(q) or not 1 <= len(s) <= 256:
        bad |= F_LENGTH
    if not bad and (len(n) > 255 or len(p) > 255):
        bad |= F_LONG
    return bad


# ---- cases ----
def _names(seed, lengths):
    rng = random.Random(seed)
    return [bytes(rng.randrange(33, 127) for _ in range(l)) for l in lengths]


def with_texts(recs, name_lengths, plus_lengths, seed=5):
    """the records with names and plus texts of the given lengths (cycled)"""
    nm = _names(seed, [name_lengths[i % len(name_lengths)] for i in range(len(recs))])
    pl = _names(seed + 1, [plus_lengths[i % len(plus_lengths)] for i in range(len(recs))])
    return [(nm[i], s, pl[i], q) for i, (_, s, _, q) in enumerate(recs)]


def cases():
    """(id, records): every sequence length at which a lane or a word begins or ends, name and plus texts of 0, 1, 16 and 255 bytes, the
    record counts around a workgroup, N-rich reads"""
    out = []
    out.append(("line_lengths", with_texts(rc.make_records(31, [1, 7, 8, 9, 15, 16, 17, 255, 256]), [0, 1, 16, 255], [255, 16, 1, 0])))
    out.append(("texts_0_1_16_255", with_texts(rc.make_records(32, [100] * 8), [0, 1, 16, 255, 255, 0], [0, 0, 1, 16, 255, 255])))
    out.append(("N_rich", rc.make_records(33, [100, 33, 150, 1, 256, 75], n_rate=0.6)))
    out.append(("all_N", [(b"n%d" % i, b"N" * l, b"", b"#" * l) for i, l in enumerate([1, 8, 16, 24, 100])]))
    for n in (1, GROUP - 1, GROUP, GROUP + 1, 5000):
        ls = [(37 + 11 * i) % 256 + 1 for i in range(n)] if n <= 17 else [150 if i % 7 else (i * 31) % 256 + 1 for i in range(n)]
        out.append(("n_%d" % n, rc.make_records(200 + n, ls)))
    return out


def case_ids():
    return [c[0] for c in cases()]


def mate_of(recs, seed=9):
    """a second file for a pair: as many records, other bases and qualities, names that end in /2"""
    other = rc.make_records(seed, [len(r[1]) for r in recs][::-1])
    return [(n[:253] + b"/2", s, p, q) for (n, _, p, _), (_, s, _, q) in zip(recs, other)]


def bad_records():
    """(id, text, number of the first bad record from 1, flag bits): what every route refuses"""
    good = rc.make_records(40, [100, 37, 100, 100, 52, 100])
    n, s, p, q = good[3]

    def with_record(k, rec):
        r = list(good)
        r[k] = rec
        return rc.text_of(r)

    t = rc.text_of(good)
    no_at = t.replace(b"@" + good[2][0], b"#" + good[2][0], 1)
    first_plus = t.index(b"\n+") + 1
    no_plus = t[:first_plus] + b"-" + t[first_plus + 1:]
    return [
        ("length_0", with_record(3, (n, b"", p, b"")), 4, F_LENGTH),
        ("length_257", with_record(2, (n, b"A" * 257, p, b"I" * 257)), 3, F_LENGTH),
        ("unequal_lengths", with_record(4, (n, s, p, q[:-1])), 5, F_LENGTH),
        ("name_256", with_record(1, (b"x" * 256, s, p, q)), 2, F_LONG),
        ("plus_256", with_record(5, (n, s, b"y" * 256, q)), 6, F_LONG),
        ("no_at", no_at, 3, F_NAME),
        ("no_plus", no_plus, 1, F_PLUS),
    ]
