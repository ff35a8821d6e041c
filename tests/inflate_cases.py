"""Shared inputs of the inflate tests (tests/test_inflate.py on the host twin, tests/test_gpu_inflate.py on the device; DESIGN.md section
3.15): DEFLATE payloads with what the standard library's zlib says about each.  Nothing of the project is the checker here:
zlib.decompressobj(-15) decodes, zlib.crc32 checks.  Payloads come from zlib at several levels, strategies and flush modes, from a small
fixed-Huffman token writer (so the tokens are known exactly), from hand-made dynamic headers, and from damage done to good payloads.
Everything is made once per process and handed out unchanged."""
import collections
import functools
import struct
import zlib

import numpy as np

import bgzf_cases as BC

OK, CORRUPT, TRUNCATED, ROOM, CHECK = 0, 1, 2, 3, 4
MEMBER_DTYPE = np.dtype([("in_off", "<u8"), ("in_bytes", "<u8"), ("out_off", "<u8"), ("isize", "<u4"), ("crc", "<u4")])

# want: the status the rules of DESIGN.md section 3.15 give the case; text: what zlib decodes (None: zlib refuses the payload or does not reach its end)
Case = collections.namedtuple("Case", "name payload isize crc want text")


# ---- the checker ----
def zlib_text(payload: bytes):
    """the text of a raw DEFLATE payload that ends with its last block, or None"""
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(payload)
    except zlib.error:
        return None
    return text if d.eof and not d.unused_data else None


def good(name: str, payload: bytes) -> Case:
    text = zlib_text(payload)
    assert text is not None, name
    return Case(name, payload, len(text), zlib.crc32(text), OK, text)


def bad(name: str, payload: bytes, want: int, isize: int = 0, crc: int = 0) -> Case:
    assert zlib_text(payload) is None, name
    return Case(name, payload, isize, crc, want, None)


# ---- BGZF wrapping ----
def bgzf_member(payload: bytes, crc: int, isize: int, extra: bytes = b"", name: bytes = b"") -> bytes:
    """header with the BC field (other FEXTRA subfields in `extra` go in front of it, `name` becomes an FNAME field), payload, CRC, ISIZE"""
    xlen = len(extra) + 6
    size = 12 + xlen + (len(name) + 1 if name else 0) + len(payload) + 8
    assert size <= 65536, "not BGZF-sized"
    head = struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, 4 | (8 if name else 0), 0, 0, 0xff, xlen) + extra + b"BC" + struct.pack("<HH", 2, size - 1)
    return head + (name + b"\0" if name else b"") + payload + struct.pack("<II", crc, isize)


def fits_bgzf(c: Case) -> bool:
    return len(c.payload) + 26 <= 65536


# ---- payloads from zlib ----
def deflate(text: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, flush_every: int = 0, flush_mode: int = zlib.Z_FULL_FLUSH) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if not flush_every:
        return c.compress(text) + c.flush()
    out = b""
    for at in range(0, len(text), flush_every):
        out += c.compress(text[at:at + flush_every]) + c.flush(flush_mode)          # an empty stored block, at a bit position that is rarely a multiple of 8
    return out + c.flush()


def fibonacci_text() -> bytes:
    """22 byte values with the counts 1, 1, 2, 3, ... 17711 (46367 bytes), shuffled: as literals alone their Huffman code is 21 deep, so
    zlib's length-limited code reaches 15 bits"""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    a = np.repeat(np.arange(22, dtype=np.uint8) + 65, fib)
    assert len(a) == 46367
    np.random.default_rng(5).shuffle(a)
    return a.tobytes()


# ---- a reader of dynamic headers (for assertions about what zlib wrote) ----
class _Bits:
    def __init__(self, data: bytes):
        self.v, self.at = int.from_bytes(data, "little"), 0

    def take(self, n: int) -> int:
        r = (self.v >> self.at) & ((1 << n) - 1)
        self.at += n
        return r


def _canonical(lens):
    """{(length, code): symbol} of a canonical code"""
    code, out = 0, {}
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                out[(l, code)] = s
                code += 1
        code <<= 1
    return out


def dynamic_code_lengths(payload: bytes):
    """(literal/length code lengths, distance code lengths) of a payload whose first block is dynamic"""
    b = _Bits(payload[:400])
    b.take(1)
    assert b.take(2) == 2
    hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    order = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
    cl = [0] * 19
    for i in range(hclen):
        cl[order[i]] = b.take(3)
    table = _canonical(cl)
    lens = []
    while len(lens) < hlit + hdist:
        l, code = 0, 0
        while (l, code) not in table:
            code = (code << 1) | b.take(1)
            l += 1
            assert l <= 7
        s = table[(l, code)]
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + b.take(2))
        elif s == 17:
            lens += [0] * (3 + b.take(3))
        else:
            lens += [0] * (11 + b.take(7))
    assert len(lens) == hlit + hdist
    return lens[:hlit], lens[hlit:]


# ---- the token writer: fixed Huffman, and the pieces of a dynamic header ----
class BitWriter:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value: int, bits: int):
        """least significant bit first (extra bits, header fields)"""
        self.v |= value << self.n
        self.n += bits

    def code(self, code: int, bits: int):
        """a Huffman code: most significant bit first"""
        for i in range(bits - 1, -1, -1):
            self.put((code >> i) & 1, 1)

    def bytes(self) -> bytes:
        return self.v.to_bytes((self.n + 7) // 8, "little")


LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def _fixed_symbol(w: BitWriter, s: int):
    if s < 144:
        w.code(0x30 + s, 8)
    elif s < 256:
        w.code(0x190 + s - 144, 9)
    elif s < 280:
        w.code(s - 256, 7)
    else:
        w.code(0xC0 + s - 280, 8)


def fixed_block(tokens, final: bool = True, w: BitWriter = None) -> BitWriter:
    """tokens: ints (literals) and (length, distance) pairs, coded as one fixed-Huffman block with its end code"""
    w = w or BitWriter()
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    for t in tokens:
        if isinstance(t, int):
            _fixed_symbol(w, t)
            continue
        length, dist = t
        i = 28 if length == 258 else max(k for k in range(28) if LEN_BASE[k] <= length)
        _fixed_symbol(w, 257 + i)
        w.put(length - LEN_BASE[i], LEN_EXTRA[i])
        j = max(k for k in range(30) if DIST_BASE[k] <= dist)
        w.code(j, 5)
        w.put(dist - DIST_BASE[j], DIST_EXTRA[j])
    _fixed_symbol(w, 256)
    return w


def expand(tokens) -> bytes:
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


# the code-length code of the hand-made dynamic headers: symbols 0 .. 12 in 4 bits, 13 .. 18 in 5 (Kraft sum 1)
_CL_LENS = [4] * 13 + [5] * 6
_CL_CODES = {s: (l, c) for (l, c), s in _canonical(_CL_LENS).items()}
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def dynamic_header(hlit: int, hdist: int, items) -> BitWriter:
    """a last block's dynamic header: items are code-length symbols 0 .. 15, or (16 | 17 | 18, repeat count)"""
    w = BitWriter()
    w.put(1, 1); w.put(2, 2)
    w.put(hlit - 257, 5); w.put(hdist - 1, 5); w.put(19 - 4, 4)
    for s in _CL_ORDER:
        w.put(_CL_LENS[s], 3)
    for it in items:
        s, rep = (it, 0) if isinstance(it, int) else it
        l, c = _CL_CODES[s]
        w.code(c, l)
        if s == 16:
            w.put(rep - 3, 2)
        elif s == 17:
            w.put(rep - 3, 3)
        elif s == 18:
            w.put(rep - 11, 7)
    return w


def _zeros(n: int):
    """n zero lengths as repeat codes 18 and 17 and plain zeros"""
    out = []
    while n >= 11:
        c = min(n, 138); out.append((18, c)); n -= c
    if n >= 3:
        out.append((17, n)); n = 0
    return out + [0] * n


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    rng = np.random.default_rng(77)
    out = []
    texts = {"empty": b"", "one_byte": b"Q", "fastq": BC.synthetic_fastq(71, 300)}
    texts.update(("bgzf_" + k, v) for k, v in BC.cases().items())
    fq = BC.synthetic_fastq(72, 1200)
    assert len(fq) > 200000
    texts["text65280"] = fq[:65280]
    texts["text65536"] = fq[:65536]
    for name, text in sorted(texts.items()):
        for tag, level, strategy in (("l0", 0, zlib.Z_DEFAULT_STRATEGY), ("l1", 1, zlib.Z_DEFAULT_STRATEGY), ("l6", 6, zlib.Z_DEFAULT_STRATEGY), ("l9", 9, zlib.Z_DEFAULT_STRATEGY),
                                     ("fixed", 6, zlib.Z_FIXED), ("huffman", 6, zlib.Z_HUFFMAN_ONLY), ("rle", 6, zlib.Z_RLE)):
            out.append(good("%s_%s" % (name, tag), deflate(text, level, strategy)))
    # several blocks in one member
    out.append(good("fastq_full_flush", deflate(texts["fastq"], 6, flush_every=7001, flush_mode=zlib.Z_FULL_FLUSH)))
    out.append(good("fastq_sync_flush", deflate(texts["fastq"], 1, flush_every=5003, flush_mode=zlib.Z_SYNC_FLUSH)))
    out.append(good("fastq_sync_flush_fixed", deflate(texts["fastq"][:9000], 6, zlib.Z_FIXED, flush_every=1009, flush_mode=zlib.Z_SYNC_FLUSH)))
    # one member of about 200 KB: not BGZF-sized, its table entry is made by hand
    out.append(good("big200k", deflate(fq[:200003], 6)))
    out.append(good("big200k_l0", deflate(fq[:200003], 0)))
    # literal codes of 15 bits, a distance code of one used length
    fib = good("fibonacci_huffman_only", deflate(fibonacci_text(), 6, zlib.Z_HUFFMAN_ONLY))
    ll, dd = dynamic_code_lengths(fib.payload)
    assert max(ll) == 15 and len({l for l in dd if l}) == 1, (max(ll), dd)                # (zlib pads the unused distance code to two codes of one bit)
    out.append(fib)
    # hand-made tokens, fixed Huffman
    lits = lambda n: [int(x) for x in rng.integers(0, 256, n)]
    hand = {"match258_dist1": [65, (258, 1)]}
    for d in (2, 3, 7, 63, 64, 65):
        hand["dist%d_overlap" % d] = lits(d) + [(min(258, 3 * d + 5), d), 10, (d + 1, d)]
    hand["dist32768"] = lits(32768) + [(100, 32768), 33, (258, 32768)]
    hand["batch_of_70_then_match"] = lits(70) + [(20, 50), (5, 1), 7, (64, 64), (258, 95)]
    for name, toks in hand.items():
        c = good("hand_" + name, fixed_block(toks).bytes())
        assert c.text == expand(toks), name
        out.append(c)
    two = fixed_block([1, 2, 3, (6, 3)], final=False)
    out.append(good("hand_two_fixed_blocks", fixed_block([(9, 9), 4], w=two).bytes()))                # a match that reaches into the block before
    out.append(bad("hand_dist_one_too_far", fixed_block(lits(5) + [(3, 6)]).bytes(), CORRUPT, 8))
    out.append(bad("hand_match_first", fixed_block([(3, 1)]).bytes(), CORRUPT, 3))
    for s in (286, 287):
        w = BitWriter(); w.put(1, 1); w.put(1, 2); _fixed_symbol(w, 65); _fixed_symbol(w, s); _fixed_symbol(w, 256)
        out.append(bad("hand_symbol_%d" % s, w.bytes(), CORRUPT, 4))
    for ds in (30, 31):
        w = BitWriter(); w.put(1, 1); w.put(1, 2); _fixed_symbol(w, 65); _fixed_symbol(w, 257); w.code(ds, 5); _fixed_symbol(w, 256)
        out.append(bad("hand_distance_symbol_%d" % ds, w.bytes(), CORRUPT, 8))
    # hand-made dynamic headers
    w = dynamic_header(257, 1, [1, 1] + _zeros(254) + [1, 1]); w.put(0, 16)
    out.append(bad("dyn_oversubscribed", w.bytes(), CORRUPT, 4))
    w = dynamic_header(257, 1, [1, 1] + _zeros(255) + [1]); w.put(0, 16)
    out.append(bad("dyn_no_end_code", w.bytes(), CORRUPT, 4))
    w = dynamic_header(257, 1, [(16, 3)] + _zeros(253) + [1, 1]); w.put(0, 16)
    out.append(bad("dyn_repeat_first", w.bytes(), CORRUPT, 4))
    w = dynamic_header(257, 1, [1, 1] + [(18, 138), (18, 138)]); w.put(0, 16)
    out.append(bad("dyn_repeat_past_the_end", w.bytes(), CORRUPT, 4))
    # 'A' and the end code in one bit each; the run of 12 zeros covers the last literal/length length and the first 11 distance lengths
    w = dynamic_header(258, 13, _zeros(65) + [1] + _zeros(190) + [1, (18, 12), 1, 1])
    for _ in range(5):
        w.code(0, 1)
    w.code(1, 1)
    c = good("dyn_repeat_across_the_border", w.bytes())
    assert c.text == b"AAAAA"
    out.append(c)
    # damage
    base = {c.name: c for c in out}
    l6, l0, fx = base["fastq_l6"], base["fastq_l0"], base["fastq_fixed"]
    stored = b"\x01" + struct.pack("<HH", 5, 0xFFFF ^ 5) + b"hello"
    assert zlib_text(stored) == b"hello"
    out.append(bad("stored_len_nlen", b"\x01" + struct.pack("<HH", 5, 0xFFFF ^ 4) + b"hello", CORRUPT, 5, zlib.crc32(b"hello")))
    out.append(bad("btype3", b"\x07\x00\x00", CORRUPT, 4))
    for c in (l6, l0, fx):
        out.append(bad(c.name + "_cut_by_one", c.payload[:-1], TRUNCATED, c.isize, c.crc))
        out.append(bad(c.name + "_cut_in_the_middle", c.payload[:len(c.payload) // 2], TRUNCATED, c.isize, c.crc))
        out.append(bad(c.name + "_garbage_behind", c.payload + b"\x5a", CORRUPT, c.isize, c.crc))
        out.append(Case(c.name + "_crc_bit", c.payload, c.isize, c.crc ^ 0x00010000, CHECK, c.text))
        out.append(Case(c.name + "_isize_plus_one", c.payload, c.isize + 1, c.crc, CHECK, c.text))
        out.append(Case(c.name + "_isize_minus_one", c.payload, c.isize - 1, c.crc, ROOM, c.text))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


def interleaved():
    """every case in a list in which each bad one has a good one on either side"""
    goods = [c for c in cases() if c.want == OK]
    bads = [c for c in cases() if c.want != OK]
    out, g = [], 0
    for b in bads:
        out += [goods[g % len(goods)], b]
        g += 1
    out += goods[g:] if g < len(goods) else [goods[0]]
    return out


def layout(cs, guard: int = 5, shuffle_payloads: bool = False):
    """(data, table, out_bytes): the payloads of `cs` each behind 18 bytes that stand for a header and in front of 8 for a trailer, and
    their slots `guard` bytes apart"""
    data, tab, at = bytearray(), np.zeros(len(cs), dtype=MEMBER_DTYPE), guard
    for i, c in enumerate(cs):
        data += b"\xEE" * 18
        tab[i] = (len(data), len(c.payload), at, c.isize, c.crc)
        data += c.payload + b"\xEE" * 8
        at += c.isize + guard
    return bytes(data), tab, at


def check(cs, tab, out: bytes, statuses: bytes, fill: int, what=""):
    """statuses as the rules say; the text of every member that is OK is zlib's; every byte outside the slots still holds `fill`"""
    mask = np.ones(len(out), dtype=bool)
    buf = np.frombuffer(out, dtype=np.uint8)
    for i, c in enumerate(cs):
        a, n = int(tab[i]["out_off"]), int(tab[i]["isize"])
        mask[a:a + n] = False
        assert statuses[i] == c.want, (what, c.name, statuses[i], c.want)
        if c.want == OK:
            assert out[a:a + n] == c.text, (what, c.name)
    assert (buf[mask] == fill).all(), (what, "a byte outside the slots changed")
