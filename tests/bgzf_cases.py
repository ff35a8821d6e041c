"""Shared inputs of the BGZF tests (tests/test_bgzf.py on the host twin, tests/test_gpu_bgzf.py on the device): the smallest texts at
which each stage of the encoder can go wrong.  Everything is made once per process and handed out unchanged."""
import functools
import struct
import zlib

import numpy as np

BLOCK = 65280
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
LENGTHS = (0, 1, 2, 3, 4, 5, 255, 256, 257, 65279, 65280, 65281, 2 * 65280 + 1)


def bound(n: int) -> int:
    return n + 31 * ((n + BLOCK - 1) // BLOCK) + 28


def _dna(seed: int, n: int) -> bytes:
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def _lines(seed: int, n: int) -> bytes:
    """text with repeats at many distances: lines of DNA drawn from a small pool, and runs"""
    rng = np.random.default_rng(seed)
    pool = [_dna(seed * 100 + i, int(rng.integers(5, 80))) + b"\n" for i in range(40)]
    out = bytearray()
    while len(out) < n:
        out += pool[int(rng.integers(0, 40))] if rng.random() < 0.8 else bytes([int(rng.integers(33, 75))]) * int(rng.integers(1, 40))
    return bytes(out[:n])


def _no_repeat(seed: int, limit: int) -> bytes:
    """over 16 byte values, no 4-gram twice and no byte three times in a row: not one match, yet well worth a dynamic block"""
    rng = np.random.default_rng(seed)
    alpha = b"0123456789abcdef"
    out = bytearray(b"012")
    seen = set()
    while len(out) < limit:
        for c in rng.permutation(16):
            g = bytes(out[-3:]) + alpha[c:c + 1]
            if g not in seen and not (out[-1] == out[-2] == alpha[c]):
                seen.add(g); out += alpha[c:c + 1]
                break
        else:
            break
    return bytes(out)


def fibonacci_literals() -> bytes:
    """24 byte values: 22 in Fibonacci proportion and two seen once, 46369 bytes, shuffled.  As LITERALS these counts would need a code 23
    bits deep, but no parse leaves them literals: the three commonest values are three quarters of the text, so most 4-grams are made of
    them alone, of which there are 81 -- they repeat, the parse finds some ten thousand matches and the histogram it codes is 13 bits
    deep.  The text is kept for what it is, a skewed text full of short matches; fibonacci_after_parse is the one whose histogram AFTER the
    parse is Fibonacci-shaped."""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    counts = fib + [1, 1]
    a = np.repeat(np.arange(24, dtype=np.uint8) + 65, counts)
    np.random.default_rng(3).shuffle(a)
    return a.tobytes()


def _spread(counts, seed: int, alphabet: bytes) -> bytes:
    """alphabet[i] exactly counts[i] times, each value spread evenly over the text, no 4-gram twice and no byte three times in a row: a
    text with a given histogram in which the parse finds not one match"""
    rng = np.random.default_rng(seed)
    total = np.array(counts, dtype=np.float64)
    left = total.copy()
    out, seen = bytearray(), set()
    for _ in range(int(total.sum())):
        for i in np.argsort(-((left - 1 + rng.random(len(left))) / total)):
            b = alphabet[i]
            g = bytes(out[-3:]) + bytes([b])
            if left[i] <= 0 or (len(out) > 1 and out[-1] == b and out[-2] == b) or (len(g) == 4 and g in seen):
                continue
            seen.add(g); out.append(b); left[i] -= 1
            break
        else:
            break
    # what the walk could not place at its end goes in between, where it repeats no 4-gram and makes no run of three
    for i in np.flatnonzero(left > 0):
        while left[i] > 0:
            for at in rng.permutation(np.arange(4, len(out) - 4)):
                t = bytes(out[at - 3:at]) + bytes([alphabet[i]]) + bytes(out[at:at + 3])
                new, old = [t[k:k + 4] for k in range(4)], [bytes(out[at - 3 + k:at + 1 + k]) for k in range(3)]
                if len(set(new)) == 4 and not any(g in seen and g not in old for g in new) and not any(t[k] == t[k + 1] == t[k + 2] for k in range(5)):
                    seen.difference_update(old); seen.update(new); out.insert(int(at), alphabet[i]); left[i] -= 1
                    break
            else:
                raise AssertionError("no room for value %d" % alphabet[i])
    assert len({bytes(out[i:i + 4]) for i in range(len(out) - 3)}) == len(out) - 3
    return bytes(out)


# how many byte values take a code of each length in fibonacci_code_lengths (the end-of-block code is one more of length 11)
CODE_LENGTH_COUNTS = {3: 2, 4: 2, 5: 7, 6: 1, 7: 21, 8: 12, 9: 57, 10: 55, 11: 29}


def fibonacci_code_lengths() -> bytes:
    """2047 literals and not one match (_spread), the byte values with dyadic frequencies 2^(11 - l): CODE_LENGTH_COUNTS[l] values take a
    code of exactly l bits, whatever the ties, since only these lengths reach the entropy.  Values of different lengths alternate, so no
    run hides them, and the header transmits the lengths 3 .. 11 with the counts 2 2 7 1 21 12 57 55 30, the length 1 twice (the two
    padded distance codes) and two runs of zeros: a histogram whose own Huffman code is 8 bits deep, one more than the 7 that the code of
    the code lengths may have."""
    n_of = CODE_LENGTH_COUNTS
    assert sum(c << (11 - l) for l, c in n_of.items()) + 1 == 1 << 11                  # Kraft sum 1 with the end-of-block code
    lens = sorted((l for l, c in n_of.items() for _ in range(c)), reverse=True)
    half = (len(lens) + 1) // 2
    order = [v for pair in zip(lens[:half], lens[half:] + [None]) for v in pair if v is not None]     # long, short, long, short ...
    return _spread([1 << (11 - l) for l in order], 0, bytes(range(40, 40 + len(order))))


# (match length, number of pieces) of fibonacci_after_parse: each count is the smallest that makes the Huffman code of the block's
# literal/length histogram one bit deeper than the counts before it do (the histogram also holds 24 symbols seen once, the match of every
# tile, 202 times, and 101 more matches of 4)
AFTER_PARSE_PIECES = ((19, 17), (17, 25), (15, 42), (13, 67), (11, 109), (10, 285), (9, 488), (7, 773), (6, 1261), (5, 2034), (4, 3193))


def fibonacci_after_parse() -> bytes:
    """A block whose literal/length histogram AFTER the parse is Fibonacci-shaped: its Huffman code is 17 bits deep, so the 15-bit limit
    bites.  The heavy symbols have to be match lengths (see fibonacci_literals), and the parse rule is used to place every match:
    the text is made of prefixes of one word W of 20 distinct bytes, so every piece begins with the same 4-gram, and the one table
    candidate of a piece is the last piece that began before its tile.  That piece is always a whole W (put wherever a tile has at most
    20 bytes left), so a prefix of l < 20 bytes is matched for exactly l: W[l] is not W[0], which follows.  A whole W is matched against the
    W of the tile before; the pieces behind the two are 4 and 8 bytes long in turn, so that match is always 24 long and leaves W[4:8] of
    every other one, a match of 4.  The first tile, which has no candidates, is one run and W: 21 literals and one match at distance 1."""
    W = bytes(range(97, 117))
    todo = np.repeat([l for l, _ in AFTER_PARSE_PIECES], [c for _, c in AFTER_PARSE_PIECES])
    np.random.default_rng(1).shuffle(todo)
    out = bytearray(b"z" * (256 - len(W)) + W)
    after_w, tiles, i = True, 0, 0
    while i < len(todo):
        if after_w:
            out += W[:4 if tiles & 1 else 8]; after_w = False
        elif 256 - len(out) % 256 <= len(W):
            out += W; after_w = True; tiles += 1
        else:
            out += W[:todo[i]]; i += 1
    assert len(out) <= BLOCK
    return bytes(out)


def synthetic_fastq(seed: int, n: int, L: int = 100) -> bytes:
    """four-line records: Illumina names, reads of a synthetic genome, synthetic qualities"""
    import name_cases
    import qual_cases
    from minicom_amd import synth
    names = name_cases.illumina(seed, n)
    reads = synth.synth_reads(seed, n, L)
    quals = qual_cases.synth_quals(seed, n, L)
    return b"".join(b"@" + names[i] + b"\n" + reads[i].tobytes() + b"\n+\n" + quals[i].tobytes() + b"\n" for i in range(n))


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    import qual_cases
    c = {"len%d" % n: _lines(n + 1, n) for n in LENGTHS}
    c["equal"] = b"A" * BLOCK
    c["no_repeat"] = _no_repeat(7, 30000)
    c["random"] = np.random.default_rng(8).integers(0, 256, BLOCK, dtype=np.uint8).tobytes()
    c["runs"] = _dna(9, 300) + b"x" * 259 + _dna(10, 200) + b"y" * 260 + _dna(11, 250) + b"z" * 516 + _dna(12, 100)
    c["period32768"] = (_dna(13, 32768) * 2)[:BLOCK]
    c["period32769"] = (_dna(14, 32769) * 2)[:BLOCK]
    head = _dna(15, 1000)
    c["repeat_to_end"] = head + head[:300]
    first = _dna(16, BLOCK)
    c["repeat_of_previous_block"] = first + first[:5000]
    c["fib_literals"] = fibonacci_literals()
    c["fib_code_lengths"] = fibonacci_code_lengths()
    c["fib_after_parse"] = fibonacci_after_parse()
    c["fastq"] = synthetic_fastq(21, 900)
    c["tricky_fastq"] = qual_cases.tricky_fastq()[2] * 9
    return c


@functools.lru_cache(maxsize=None)
def size_texts() -> dict:
    """the three texts of about 4 MB the size check runs over: full synthetic FASTQ, a reads-only file, a tricky FASTQ text"""
    import qual_cases
    from minicom_amd import synth
    reads = synth.synth_reads(52, 40000, 100)
    return {"fastq": synthetic_fastq(51, 15000), "reads": b"".join(r.tobytes() + b"\n" for r in reads), "tricky_fastq": qual_cases.tricky_fastq(53, 48000, 37)[2]}


def twin_and_zlib1(data: bytes):
    """(bytes of the twin's DEFLATE blocks, bytes of raw DEFLATE at zlib level 1 of the same 65280-byte blocks): headers, trailers and the
    empty member, which are the same on both sides, are left out"""
    from minicom_amd import pipeline
    z = pipeline.bgzf_encode(data)
    twin = sum(size - 26 for _, size in members(z))
    z1 = 0
    for at in range(0, len(data), BLOCK):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        z1 += len(c.compress(data[at:at + BLOCK]) + c.flush())
    return twin, z1


def size_margin(twin: int, z1: int) -> float:
    """the room the size check leaves above zlib level 1: the measured excess rounded up to a whole percent, plus two points (two points
    alone where the twin is not larger)"""
    import math
    return (math.ceil(max(0.0, 100.0 * (twin - z1) / z1)) + 2) / 100.0


def members(z: bytes):
    """walks a BGZF file by each header's BSIZE: [(offset, size)] of the members in front of the last, empty one.  Asserts the fixed header
    bytes, every size <= 65536, and that the walk lands exactly on the 28 bytes of the empty member at the file's end."""
    out, at = [], 0
    while at < len(z) - len(EOF):
        assert z[at:at + 16] == EOF[:16], "header at %d" % at
        size = struct.unpack_from("<H", z, at + 16)[0] + 1
        assert 26 < size <= 65536
        out.append((at, size)); at += size
    assert at == len(z) - len(EOF) and z[at:] == EOF
    return out


def check_structure(z: bytes, data: bytes) -> None:
    """every member's ISIZE and CRC-32 against its 65280 bytes of `data`, each member decoded on its own by zlib, the total within bound"""
    ms = members(z)
    assert len(ms) == (len(data) + BLOCK - 1) // BLOCK and len(z) <= bound(len(data))
    for k, (at, size) in enumerate(ms):
        want = data[k * BLOCK:(k + 1) * BLOCK]
        crc, isize = struct.unpack_from("<II", z, at + size - 8)
        assert isize == len(want) and crc == zlib.crc32(want), "member %d" % k
        d = zlib.decompressobj(31)
        assert d.decompress(z[at:at + size]) == want and d.eof and not d.unused_data, "member %d" % k


def dynamic_header(member: bytes):
    """(HLIT, HDIST, HCLEN, the code-length code's lengths in transmission order) of a member that is one dynamic block, None if stored"""
    bits = int.from_bytes(member[18:18 + 12], "little")
    if (bits >> 1) & 3 != 2:
        return None
    hlit, hdist, hclen = 257 + ((bits >> 3) & 31), 1 + ((bits >> 8) & 31), 4 + ((bits >> 13) & 15)
    return hlit, hdist, hclen, [(bits >> (17 + 3 * i)) & 7 for i in range(hclen)]


def huffman_depth(freqs) -> int:
    """the longest code of the SHALLOWEST Huffman code of the symbols with freq > 0 (a tie goes to the shallower subtree): what a code
    without a length limit needs at the least"""
    import heapq
    h = [(f, 0) for f in freqs if f]
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1]


def histograms(member: bytes) -> dict:
    """Reads a member that is one dynamic block with a small inflater of its own.  cl_len, ll_len, d_len: the three codes' lengths as the
    header gives them; cl_freq, ll_freq, d_freq: how often the block uses each symbol of the three alphabets; n: the bytes it decodes to."""
    v, at = int.from_bytes(member[18:-8], "little"), 0

    def get(n):
        nonlocal at
        r = (v >> at) & ((1 << n) - 1); at += n
        return r

    def decoder(lens):                                                             # {(length, code): symbol} of the canonical code
        code, out = 0, {}
        for l in range(1, 16):
            for s, x in enumerate(lens):
                if x == l:
                    out[(l, code)] = s; code += 1
            code <<= 1
        return out

    def sym(dec):
        code = 0
        for l in range(1, 16):
            code = (code << 1) | get(1)
            if (l, code) in dec:
                return dec[(l, code)]
        raise AssertionError("no such code")

    assert get(1) == 1 and get(2) == 2
    hlit, hdist, hclen = 257 + get(5), 1 + get(5), 4 + get(4)
    cl_len = [0] * 19
    for i in range(hclen):
        cl_len[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[i]] = get(3)
    dec, lens, cl_freq = decoder(cl_len), [], [0] * 19
    while len(lens) < hlit + hdist:
        s = sym(dec); cl_freq[s] += 1
        lens += [s] if s < 16 else [lens[-1]] * (3 + get(2)) if s == 16 else [0] * (3 + get(3)) if s == 17 else [0] * (11 + get(7))
    assert len(lens) == hlit + hdist
    ll_len, d_len = lens[:hlit], lens[hlit:]
    ll_dec, d_dec = decoder(ll_len), decoder(d_len)
    base = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
    ll_freq, d_freq, n = [0] * 286, [0] * 30, 0
    while True:
        s = sym(ll_dec); ll_freq[s] += 1
        if s == 256:
            break
        if s < 256:
            n += 1; continue
        n += base[s - 257] + get(0 if s < 265 or s == 285 else (s - 261) >> 2)
        d = sym(d_dec); d_freq[d] += 1; get(0 if d < 4 else (d >> 1) - 1)
    return dict(cl_len=cl_len, ll_len=ll_len, d_len=d_len, cl_freq=cl_freq, ll_freq=ll_freq, d_freq=d_freq, n=n)
