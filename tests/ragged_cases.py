"""FASTQ texts with reads of differing lengths, from a seed, and the split of DESIGN.md section 3.16 in plain Python: the reference for
the device calls (csrc/ragged.hip) and for their host twins (host/mcom_ragged.cpp).

A case is a list of records (name, sequence, plus text, qualities), all bytes.  `split` states the rule: L is the modal sequence length
(ties: the larger one); a record of that length is even and becomes a row, every other record is odd and its lines are appended to the
odd texts; len.bin holds length - 1 per record; the slot of a record is its rank among the even records, or its offset into the odd
text with bit 63 set."""
import gzip
import random

ODD = 1 << 63
GROUP = 16                      # records per workgroup of the sixteen-lanes-per-record kernels (256 threads)


def make_records(seed, lengths, names=None, n_rate=0.02):
    """one record per entry of `lengths`; N now and then; every third quality line starts with '@' or '+'"""
    rng = random.Random(seed)
    recs = []
    for i, l in enumerate(lengths):
        seq = bytes(rng.choice(b"ACGT") if rng.random() >= n_rate else ord("N") for _ in range(l))
        qual = bytearray(rng.randrange(33, 127) for _ in range(l))
        if i % 3 == 0:
            qual[0] = ord("@") if i % 2 else ord("+")
        name = (b"r%d/%d len=%d" % (seed, i, l)) if names is None else names[i]
        plus = b"" if i % 4 else name[:7]
        recs.append((name, seq, plus, bytes(qual)))
    return recs


def text_of(recs, final_newline=True) -> bytes:
    t = b"".join(b"@" + n + b"\n" + s + b"\n+" + p + b"\n" + q + b"\n" for n, s, p, q in recs)
    return t if final_newline else t[:-1]


def modal_length(lengths) -> int:
    hist = {}
    for l in lengths:
        hist[l] = hist.get(l, 0) + 1
    return max(hist, key=lambda l: (hist[l], l))


def split(recs):
    """dict: L, len_bin, slots, even_seq / even_qual (lists of rows), odd_seq / odd_qual (bytes), n_even, n_odd"""
    L = modal_length([len(r[1]) for r in recs]) if recs else 0
    out = {"L": L, "len_bin": bytes(len(r[1]) - 1 for r in recs), "slots": [], "even_seq": [], "even_qual": [], "odd_seq": b"", "odd_qual": b""}
    for _, s, _, q in recs:
        if len(s) == L:
            out["slots"].append(len(out["even_seq"]))
            out["even_seq"].append(s)
            out["even_qual"].append(q)
        else:
            out["slots"].append(ODD | len(out["odd_seq"]))
            out["odd_seq"] += s
            out["odd_qual"] += q
    out["n_even"] = len(out["even_seq"])
    out["n_odd"] = len(recs) - out["n_even"]
    return out


def name_text(recs):
    """the name text of section 3.10 (name line and '+' text without their first bytes, each with its newline) and its record offsets"""
    text, off = b"", [0]
    for n, _, p, _ in recs:
        text += n + b"\n" + p + b"\n"
        off.append(len(text))
    return text, off


def numbered(recs):
    """the records as a decoder without name.mcn writes them"""
    return b"".join(b"@%d\n" % (i + 1) + s + b"\n+\n" + q + b"\n" for i, (_, s, _, q) in enumerate(recs))


def reads_only(recs):
    return b"".join(s + b"\n" for _, s, _, _ in recs)


def _mixed(seed, n, L=100, share=0.1, extra=()):
    rng = random.Random(seed)
    ls = [L if rng.random() >= share else rng.randrange(30, L) for _ in range(n)]
    for k, l in enumerate(extra):
        ls[(7 + 13 * k) % n] = l
    return ls


def cases():
    """(id, records): the smallest shapes at which the kernels and the scans can go wrong"""
    out = []
    # the lane stride of sixteen and both ends of the length byte, among reads of L = 100
    out.append(("stride_and_byte_ends", make_records(1, [100, 1, 100, 15, 16, 100, 17, 255, 100, 256, 100, 100])))
    out.append(("L_is_1", make_records(2, [1, 1, 5, 1, 256, 1])))
    out.append(("L_is_256", make_records(3, [256, 256, 1, 256, 255, 256])))
    out.append(("first_odd", make_records(4, [37, 100, 100, 100])))
    out.append(("last_odd", make_records(5, [100, 100, 100, 37])))
    out.append(("odd_neighbours", make_records(6, [100, 100, 40, 41, 100, 100, 100])))
    out.append(("all_but_one_odd", make_records(7, [50, 100, 51, 52, 53, 54, 55])))            # every length once: L is the largest
    out.append(("one_length_twice", make_records(8, [60, 61, 62, 62, 63, 64])))
    out.append(("tie_goes_to_the_larger", make_records(9, [80, 90, 80, 90, 70])))
    out.append(("N_everywhere", make_records(10, [100] * 6 + [33, 34] + [100] * 3, n_rate=0.4)))
    for n in (1, GROUP - 1, GROUP, GROUP + 1, 5000):
        out.append(("n_%d" % n, make_records(100 + n, _mixed(100 + n, n, extra=(1, 256) if n > 30 else (17,) if n > 1 else ()))))
    return out


def case_ids():
    return [c[0] for c in cases()]


def gz_members(text: bytes, n_members: int) -> bytes:
    """the text as a gzip file of n_members members, cut at arbitrary bytes (inside records too)"""
    cut = [len(text) * k // n_members for k in range(n_members + 1)]
    return b"".join(gzip.compress(text[cut[k]:cut[k + 1]], 6) for k in range(n_members))


def bad_records():
    """(id, text, number of the first bad record, 1-based): what every route refuses"""
    good = make_records(20, [100, 37, 100, 100, 52, 100])

    def with_record(k, rec):
        r = list(good)
        r[k] = rec
        return text_of(r)

    n, s, p, q = good[3]
    return [
        ("length_0", with_record(3, (n, b"", p, b"")), 4),
        ("length_257", with_record(2, (n, b"A" * 257, p, b"I" * 257)), 3),
        ("unequal_lengths", with_record(4, (n, s, p, q[:-1])), 5),
        ("base_outside_ACGTN", with_record(1, (n, s[:50] + b"a" + s[51:], p, q)), 2),
        ("quality_below_33", with_record(5, (n, s, p, q[:99] + b" ")), 6),
        ("quality_above_126", with_record(0, (n, s, p, b"\x7f" + q[1:])), 1),
    ]


# ---- the file calls (host twins with device=None, the GPU routes with a device) against the split above ----
def split_files(tmp_path, fastq, device=None, piece_bytes=0):
    """(n, L, n_odd, len.bin, even reads, odd.seq, even quality rows of qual.mcq, odd.qual, rows of the raw quality split, its odd text)"""
    from minicom_amd import pipeline
    t = tmp_path
    n, L, n_odd = pipeline.fastq_lengths(str(fastq), str(t / "len.bin"), device, piece_bytes)
    ne1 = pipeline.fastq_ragged_files(str(fastq), 1, L, str(t / "len.bin"), str(t / "rows1"), str(t / "odd1"), device, piece_bytes)
    ne3 = pipeline.fastq_ragged_files(str(fastq), 3, L, str(t / "len.bin"), str(t / "rows3"), str(t / "odd3"), device, piece_bytes)
    neq = pipeline.fastq_quality_member_ragged(str(fastq), L, str(t / "len.bin"), str(t / "qual.mcq"), str(t / "odd.qual"), device)
    assert ne1 == ne3 == neq == n - n_odd
    return n, L, n_odd, (t / "len.bin").read_bytes(), (t / "rows1").read_bytes(), (t / "odd1").read_bytes(), (t / "qual.mcq").read_bytes(), (t / "odd.qual").read_bytes(), \
        (t / "rows3").read_bytes(), (t / "odd3").read_bytes()


def check_against_python(recs, got):
    """what _split_files returns against the split in plain Python"""
    import numpy as np
    from minicom_amd import pipeline
    want = split(recs)
    n, L, n_odd, len_bin, rows1, odd1, mcq, odd_qual, rows3, odd3 = got
    assert (n, L, n_odd) == (len(recs), want["L"], want["n_odd"])
    assert len_bin == want["len_bin"]
    assert rows1 == b"".join(want["even_seq"]) and odd1 == want["odd_seq"]
    assert rows3 == b"".join(want["even_qual"]) and odd3 == want["odd_qual"] and odd_qual == want["odd_qual"]
    assert mcq == pipeline.qual_encode(np.frombuffer(b"".join(want["even_qual"]), dtype=np.uint8).reshape(want["n_even"], L))
    assert pipeline.ragged_index(len_bin, L) == (want["slots"], want["n_even"], want["n_odd"], len(want["odd_seq"]))
