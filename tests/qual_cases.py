"""Shared inputs of the quality-coder tests (tests/test_qual.py on the host, tests/test_gpu_qual.py on the device): the synthetic
quality generator, the degenerate matrices, the hostile corpus and a FASTQ writer.  Everything is made once per process and handed out
unchanged."""
import functools

import numpy as np

import qual_reference as QR


def synth_quals(seed, n, L, binned=False):
    rng = np.random.default_rng(seed); q = np.empty((n, L), np.int64)
    base = rng.choice(np.array([38, 34, 28]), size=n, p=[.6, .3, .1]); cur = base.copy()
    for j in range(L):
        drop = rng.random(n) < (0.01 + 0.10 * j / L); rec = rng.random(n) < 0.5
        down = np.maximum(2, cur - rng.integers(5, 25, n)); up = np.minimum(base, cur + rng.integers(1, 8, n))
        cur = np.where(drop, down, np.where(rec, up, cur)); q[:, j] = cur
    if binned: q = np.array([2, 12, 23, 37])[np.digitize(q, [10, 20, 30])]
    return (q + 33).astype(np.uint8)


def _alphabet(seed, n, L, values):
    """rows over exactly the given byte values (every one occurs when n * L >= len(values))"""
    rng = np.random.default_rng(seed)
    values = np.asarray(values, dtype=np.uint8)
    q = values[rng.integers(0, len(values), (n, L))]
    flat = q.reshape(-1)
    flat[:min(len(values), flat.size)] = values[:flat.size]
    return q


R100 = QR.default_rps(100)          # 20 rows per segment at L = 100


@functools.lru_cache(maxsize=None)
def degenerate():
    """(name, matrix) pairs: n = 0 and 1; L = 1, 37, 100, 150, 256; alphabets of 1, 2, 4, 41 and all 94 values; n = R - 1, R, R + 1 and
    64 R + 1 rows for R = rows_per_seg"""
    c = [("n0", np.zeros((0, 100), np.uint8)), ("n1", synth_quals(11, 1, 100))]
    for L in (1, 37, 100, 150, 256):
        c.append(("L%d" % L, synth_quals(20 + L, 70, L)))
    c.append(("A1", np.full((33, 50), 70, np.uint8)))
    c.append(("A2", _alphabet(31, 40, 75, [35, 73])))
    c.append(("A4", synth_quals(32, 90, 100, binned=True)))
    c.append(("A41", _alphabet(33, 90, 100, range(33, 74))))
    c.append(("A94", _alphabet(34, 120, 100, range(33, 127))))
    for name, n in (("R-1", R100 - 1), ("R", R100), ("R+1", R100 + 1), ("64R+1", 64 * R100 + 1)):
        c.append((name, synth_quals(40 + n, n, 100)))
    for _, q in c:
        q.setflags(write=False)
    return tuple(c)


# ---- the hostile corpus ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small():
    """(matrix, member): a small member of model 2 with three segments, the base of the truncations and bit flips"""
    q = synth_quals(3, 9, 37, binned=True)
    q.setflags(write=False)
    return q, QR.ref_encode(q, model=QR.P, rows_per_seg=4)


def truncations():
    m = small()[1]
    return [m[:k] for k in range(len(m))]


def bit_flips(count=200, seed=77):
    m = small()[1]
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        b = bytearray(m)
        at = int(rng.integers(0, len(m) * 8))
        b[at >> 3] ^= 1 << (at & 7)
        out.append(bytes(b))
    return out


def _parts(member):
    h = QR.parse_header(member)
    t0 = QR.HEADER; l0 = t0 + h["table_bytes"]; r0 = l0 + 2 * h["n_seg"]
    return h, bytearray(member[:t0]), bytearray(member[t0:l0]), [int.from_bytes(member[l0 + 2 * s:l0 + 2 * s + 2], "little") for s in range(h["n_seg"])], bytearray(member[r0:])


def _join(head, tables, lens, runs, fix=True):
    head = bytearray(head)
    if fix:
        head[28:32] = len(tables).to_bytes(4, "little")
        head[7:12] = len(runs).to_bytes(5, "little")
    return bytes(head) + bytes(tables) + b"".join(v.to_bytes(2, "little") for v in lens) + bytes(runs)


def _set(member, at, value: bytes):
    b = bytearray(member); b[at:at + len(value)] = value
    return bytes(b)


@functools.lru_cache(maxsize=None)
def crafted():
    """(name, the rule of qual_reference.ref_decode that refuses it, member): one member per refusal rule of section 3.9.  The embedded
    members of kind 1 are passed in by the caller of ref_decode, so those that need a valid one are made in the tests."""
    q, m = small()
    h, head, tables, lens, runs = _parts(m)
    A = len(QR.map_values(h["map"]))
    out = [("magic", "header", _set(m, 0, b"MCQW")), ("version", "header", _set(m, 4, b"\x02")), ("kind", "header", _set(m, 5, b"\x02")),
           ("model", "header", _set(m, 6, b"\x05")), ("L0", "header", _set(m, 24, b"\x00\x00")), ("L257", "header", _set(m, 24, b"\x01\x01")),
           ("rps0", "header", _set(m, 26, b"\x00\x00")), ("rps*L", "header", _set(m, 26, (900).to_bytes(2, "little"))),
           ("n_rows", "header", _set(m, 16, (1 << 32).to_bytes(8, "little"))), ("longer", "header", m + b"\x00"),
           ("table_bytes", "header", _set(m, 28, (h["table_bytes"] + 1).to_bytes(4, "little"))),
           ("no map", "header", _set(m, 32, bytes(32))), ("stored size", "header", _set(m, 6, b"\x00")),
           ("rows of a coded member", "header", _set(m, 16, (0).to_bytes(8, "little"))),
           ("kind 1 with a map", "header", _set(_set(m, 5, b"\x01"), 6, b"\x00")),
           ("crc", "crc", _set(m, 12, ((h["crc"] ^ 1).to_bytes(4, "little"))))]
    # payload < 4 n_seg: three runs of 1 byte
    out.append(("4 bytes per run", "header", _join(head, tables, [1, 1, 1], runs[:3])))
    # tables: the first row is `n u16` then n entries of (symbol, freq u16)
    n0 = int.from_bytes(tables[0:2], "little")
    assert n0 >= 2
    t = bytearray(tables); t[2] = A; out.append(("symbol >= A", "tables", _join(head, t, lens, runs)))
    t = bytearray(tables); t[5] = t[2]; out.append(("symbols not ascending", "tables", _join(head, t, lens, runs)))
    t = bytearray(tables); f0 = int.from_bytes(t[3:5], "little"); f1 = int.from_bytes(t[6:8], "little")
    t[3:5] = (f0 + f1).to_bytes(2, "little"); t[6:8] = b"\x00\x00"; out.append(("frequency 0", "tables", _join(head, t, lens, runs)))
    t = bytearray(tables); t[3:5] = (f0 + 1).to_bytes(2, "little") if f0 < 4096 else (f0 - 1).to_bytes(2, "little"); out.append(("sum != 4096", "tables", _join(head, t, lens, runs)))
    t = bytearray(tables); t[0:2] = (A + 1).to_bytes(2, "little"); out.append(("row longer than A", "tables", _join(head, t, lens, runs)))
    out.append(("tables with bytes left over", "tables", _join(head, tables + b"\x00\x00", lens, runs)))
    # run lengths and runs
    out.append(("lengths", "lengths", _join(head, tables, [lens[0] + 1, lens[1], lens[2]], runs)))
    out.append(("run<4", "run<4", _join(head, tables, [3, lens[1] + lens[0] - 3, lens[2]], runs)))
    r = bytearray(runs); r[0:4] = (STATE_LOW).to_bytes(4, "little"); out.append(("state below 2^23", "state", _join(head, tables, lens, r)))
    r = bytearray(runs); r[3] |= 0x80; out.append(("state from 2^31", "state", _join(head, tables, lens, r)))
    out.append(("exhausted", "exhausted", _join(head, tables, [lens[0], lens[1], lens[2] - 1], runs[:-1])))
    out.append(("end", "end", _join(head, tables, [lens[0], lens[1], lens[2] + 1], runs + b"\x00")))
    # a context that the data reaches, with an empty row: context 0 (the first column of every row) loses its row
    t = bytearray(tables[2 + 3 * n0:]); out.append(("slot", "slot", _join(head, b"\x00\x00" + t, lens, runs)))
    return tuple(out)


STATE_LOW = (1 << 23) - 1


# ---- FASTQ ------------------------------------------------------------------------------------------------------------------------------
def fastq_bytes(reads, quals, last_newline=True) -> bytes:
    """records `@<i+1>`, read, `+`, qualities -- the form the decoders write back"""
    assert reads.shape == quals.shape
    out = bytearray()
    for i in range(reads.shape[0]):
        out += b"@%d\n" % (i + 1) + reads[i].tobytes() + b"\n+\n" + quals[i].tobytes() + b"\n"
    return bytes(out if last_newline else out[:-1])


def tricky_fastq(seed=5, n=120, L=37):
    """(reads, quals, text): quality lines that begin with '@' and with '+', and one made of '@' alone"""
    rng = np.random.default_rng(seed)
    reads = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, L))]
    quals = synth_quals(seed, n, L).copy()
    quals[3, 0] = ord("@"); quals[4, 0] = ord("+"); quals[5, :] = ord("@"); quals[n - 1, 0] = ord("+")
    return reads, quals, fastq_bytes(reads, quals)


def bad_fastqs():
    """name -> the tricky FASTQ with record 18 (from 1) replaced by one the rules refuse; "shifted" keeps the file's total of quality
    bytes a multiple of L (a short quality line balanced by a long one), which a check of the byte count alone would let through"""
    reads, quals, text = tricky_fastq()
    lines = [l + b"\n" for l in text[:-1].split(b"\n")]
    rec = lambda i: b"".join(lines[4 * i:4 * i + 4])
    q17, r17, q18, r18 = quals[17].tobytes(), reads[17].tobytes(), quals[18].tobytes(), reads[18].tobytes()

    def with_records(new):
        return b"".join(new.get(k, rec(k)) for k in range(len(lines) // 4))
    one = lambda r: with_records({17: r})
    return {"crlf": one(b"@18\n" + r17 + b"\n+\n" + q17 + b"\r\n"), "short": one(b"@18\n" + r17 + b"\n+\n" + q17[:-1] + b"\n"),
            "127": one(b"@18\n" + r17 + b"\n+\n" + q17[:5] + b"\x7f" + q17[6:] + b"\n"), "space": one(b"@18\n" + r17 + b"\n+\n" + b" " + q17[1:] + b"\n"),
            "no @": one(b"18\n" + r17 + b"\n+\n" + q17 + b"\n"), "no +": one(b"@18\n" + r17 + b"\n-\n" + q17 + b"\n"), "long read": one(b"@18\n" + r17 + b"A\n+\n" + q17 + b"\n"),
            "shifted": with_records({17: b"@18\n" + r17 + b"\n+\n" + q17[:-1] + b"\n", 18: b"@19\n" + r18 + b"\n+\n" + q17[-1:] + q18 + b"\n"})}
