"""An independent statement of the `.bwt` member format, written from DESIGN.md section 3.8 alone: plain Python and numpy, a naive
suffix sort (`sorted` on slices, so blocks of at most 2^12 bytes), sequential move-to-front, tests/rans_reference.py for the embedded
member and zlib.crc32 for the checksum.  It shares no code with csrc/bwt_model.hpp, csrc/bwt.hip or host/mcom_bwt.cpp."""
import math
import zlib

import numpy as np

import rans_reference as rr

HEADER = 40
BLK_LOG2, ANC_LOG2 = 20, 12            # what the encoders write
PLAIN, BWT = 0, 1
CANDIDATES = ((0, 1), (1, 1), (1, 2), (1, 4), (2, 1), (2, 2), (2, 4))      # the `.rans` models, simpler first (section 3.6)


class BwtRefused(ValueError):
    """ref_decode: the member is one that section 3.8 says is refused; .rule names the first rule it breaks"""
    def __init__(self, rule, detail=""):
        super().__init__(rule + (": " + detail if detail else ""))
        self.rule = rule


# ---- the embedded member: section 3.6's choice of a model from the estimated sizes ----------------------------------------------------
def rans_choice(raw: bytes):
    """(model, stride) with the smallest estimate 32 + tables + ceil(bits / 8) + 8 per segment; stored costs 32 + n; ties: the earlier"""
    best, pick = 32 + len(raw), (0, 1)
    if not raw:
        return pick
    d = np.frombuffer(raw, dtype=np.uint8).astype(np.int64)
    i = np.arange(d.size)
    n_seg = -(-len(raw) // (1 << rr.SEG_LOG2))
    for model, stride in CANDIDATES[1:]:
        freq = rr.ref_tables(raw, model, stride)
        ctx = np.zeros(d.size, dtype=np.int64)
        if model == rr.ORDER1:
            ctx[stride:] = d[:-stride]
            ctx[(i % (1 << rr.SEG_LOG2)) < stride] = 0
        f = freq[i % stride, ctx, d]
        # summed per table row in symbol order, as the format's estimate is defined: count * log2(4096 / f)
        bits = 0.0
        flat = ((i % stride) * freq.shape[1] + ctx) * 256 + d
        cnt = np.bincount(flat, minlength=freq.size).reshape(freq.shape)
        for pl in range(freq.shape[0]):
            for c in range(freq.shape[1]):
                for s in np.flatnonzero(freq[pl, c]):
                    bits += float(cnt[pl, c, s]) * math.log2(4096.0 / float(freq[pl, c, s]))
        est = 32 + len(rr._serialise(freq)) + math.ceil(bits / 8.0) + 8 * n_seg
        if est < best:
            best, pick = est, (model, stride)
    return pick


def rans_member(raw: bytes) -> bytes:
    return rr.ref_encode(raw, *rans_choice(raw))


# ---- the stages ---------------------------------------------------------------------------------------------------------------------
def transform_block(t: bytes, anc_log2: int):
    """(transformed bytes, index rows): rows 0 .. len, row 0 the empty suffix, then the suffixes ascending (a shorter suffix that is a
    prefix of a longer one comes first: the end of the block is below every byte); the row of the suffix at 0 has no byte"""
    n = len(t)
    assert 0 < n <= 1 << 12
    order = sorted(range(n), key=lambda p: t[p:])
    row_of = {p: j + 1 for j, p in enumerate(order)}
    out = bytearray([t[n - 1]])
    for p in order:
        if p:
            out.append(t[p - 1])
    index = [row_of[k << anc_log2] for k in range(-(-n // (1 << anc_log2)))]
    return bytes(out), index


def mtf(data: bytes) -> bytes:
    lst = list(range(256))
    out = bytearray()
    for c in data:
        k = lst.index(c)
        out.append(k)
        lst.insert(0, lst.pop(k))
    return bytes(out)


def unmtf(ranks: bytes) -> bytes:
    lst = list(range(256))
    out = bytearray()
    for k in ranks:
        c = lst.pop(k)
        out.append(c)
        lst.insert(0, c)
    return bytes(out)


def ref_stages(raw: bytes, blk_log2: int, anc_log2: int):
    """(transformed bytes of all blocks, index as a list of rows, ranks of all blocks)"""
    tr, index, ranks = bytearray(), [], bytearray()
    for a in range(0, len(raw), 1 << blk_log2):
        o, ix = transform_block(raw[a:a + (1 << blk_log2)], anc_log2)
        tr += o; index += ix; ranks += mtf(o)
    return bytes(tr), index, bytes(ranks)


def ref_header(kind, blk_log2, anc_log2, raw_len, crc, index_bytes, member_bytes) -> bytes:
    return (b"MCBW" + bytes([1, kind, blk_log2, anc_log2]) + raw_len.to_bytes(8, "little") + crc.to_bytes(4, "little") + bytes(4)
            + index_bytes.to_bytes(8, "little") + member_bytes.to_bytes(8, "little"))


def ref_encode(raw, blk_log2: int = BLK_LOG2, anc_log2: int = ANC_LOG2, kind=None) -> bytes:
    """raw bytes -> the member.  kind None: the smaller of the two payloads, plain on a tie; PLAIN / BWT force one (decoder tests)"""
    raw = bytes(raw)
    crc = zlib.crc32(raw) if raw else 0
    plain = rans_member(raw) if kind in (None, PLAIN) else None
    coded = None
    if raw and kind in (None, BWT):
        _, index, ranks = ref_stages(raw, blk_log2, anc_log2)
        coded = b"".join(r.to_bytes(4, "little") for r in index), rans_member(ranks)
    if kind is None:
        kind = BWT if coded is not None and len(coded[0]) + len(coded[1]) < len(plain) else PLAIN
    if kind == BWT:
        return ref_header(BWT, blk_log2, anc_log2, len(raw), crc, len(coded[0]), len(coded[1])) + coded[0] + coded[1]
    return ref_header(PLAIN, blk_log2, anc_log2, len(raw), crc, 0, len(plain)) + plain


def parse_header(member: bytes):
    bad = lambda why: BwtRefused("header", why)
    if len(member) < HEADER or member[:4] != b"MCBW" or member[4] != 1:
        raise bad("magic / version / shorter than a header")
    h = {"kind": member[5], "blk_log2": member[6], "anc_log2": member[7], "raw_len": int.from_bytes(member[8:16], "little"),
         "crc": int.from_bytes(member[16:20], "little"), "zero": int.from_bytes(member[20:24], "little"),
         "index_bytes": int.from_bytes(member[24:32], "little"), "member_bytes": int.from_bytes(member[32:40], "little")}
    if h["kind"] > BWT or h["zero"]:
        raise bad("kind / reserved word")
    if not 8 <= h["blk_log2"] <= 23 or not 4 <= h["anc_log2"] <= 23:
        raise bad("block or anchor size")
    if h["raw_len"] > 0xFFFFFFFE or (h["kind"] == BWT and h["raw_len"] == 0):
        raise bad("raw length")
    B, A = 1 << h["blk_log2"], 1 << h["anc_log2"]
    h["blocks"] = [min(B, h["raw_len"] - a) for a in range(0, h["raw_len"], B)]
    n_anchors = sum(-(-l // A) for l in h["blocks"])
    if h["index_bytes"] != (4 * n_anchors if h["kind"] == BWT else 0):
        raise bad("index size")
    if len(member) != HEADER + h["index_bytes"] + h["member_bytes"] or h["member_bytes"] < 32:
        raise bad("length")
    return h


def ref_decode(member) -> bytes:
    """the member -> its raw bytes; BwtRefused for everything section 3.8 refuses"""
    member = bytes(member)
    h = parse_header(member)
    emb = member[HEADER + h["index_bytes"]:]
    try:
        eh = rr.parse_header(emb)
    except rr.RansRefused as e:
        raise BwtRefused("embedded", str(e))
    if eh["raw_len"] != h["raw_len"] or (h["kind"] == PLAIN and eh["crc"] != h["crc"]):
        raise BwtRefused("embedded", "raw length or CRC differ from the outer header's")
    A = 1 << h["anc_log2"]
    index, at = [], HEADER
    if h["kind"] == BWT:
        for l in h["blocks"]:
            rows = [int.from_bytes(member[at + 4 * k:at + 4 * k + 4], "little") for k in range(-(-l // A))]
            at += 4 * len(rows)
            if any(not 1 <= r <= l for r in rows):
                raise BwtRefused("index", "a row outside 1 .. block length")
            index.append(rows)
    try:
        inner = rr.ref_decode(emb)
    except rr.RansRefused as e:
        raise BwtRefused("embedded", str(e))
    if h["kind"] == PLAIN:
        return inner
    out = bytearray()
    pos = 0
    for l, rows in zip(h["blocks"], index):
        o = unmtf(inner[pos:pos + l]); pos += l
        below = np.concatenate([[0], np.cumsum(np.bincount(np.frombuffer(o, dtype=np.uint8), minlength=256))])
        seen = [0] * 256
        follow = []
        for c in o:
            follow.append(1 + int(below[c]) + seen[c]); seen[c] += 1
        r0 = rows[0]
        t = bytearray(l)
        for k in range(len(rows)):
            lo, hi = k * A, min(l, (k + 1) * A)
            r = 0 if hi == l else rows[k + 1]
            for p in range(hi - 1, lo - 1, -1):
                if r == r0 or r > l:
                    raise BwtRefused("walk", "stretch %d reaches the row without a byte" % k)
                j = r if r < r0 else r - 1
                t[p] = o[j]; r = follow[j]
            if r != rows[k]:
                raise BwtRefused("chain", "stretch %d ends in row %d, the index says %d" % (k, r, rows[k]))
        out += t
    if zlib.crc32(bytes(out)) != h["crc"]:
        raise BwtRefused("crc")
    return bytes(out)
