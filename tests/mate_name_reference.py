"""An independent reference for `.mcn` kind 2, a name text coded against the name text of its mate file, written from DESIGN.md
section 3.12 and from nothing else: it shares no code with csrc/name_model.hpp.  The token rule, the header's first 88 bytes and
everything about kinds 0 and 1 are name_reference.py's (section 3.10); the embedded `.bwt` / `.rans` coders are handed in, as there.

    ref_streams_mate(text, n, mate)                                   -> the seven raw streams of kind 2
    ref_encode_mate(text, n, mate, bwt_encode, rans_encode, kind=None) -> the member: kind 2 only where strictly smaller (kind=2 forces it)
    ref_decode_mate(member, mate, bwt_decode, rans_decode)             -> the name text; NameRefused(rule) for every member the section refuses

`python tests/mate_name_reference.py` runs the self-check below with stand-in coders (no library, no GPU).
"""
import struct
import zlib

import name_reference as NR
from name_reference import DELTA, END, INC, MATCH, NUM, TEXT, NAME_MAX, STREAMS, TOKEN_CAP, VALUE_END, NameRefused

KIND_MATE = 2


def _crc(b: bytes) -> int:
    return zlib.crc32(b) & 0xFFFFFFFF if b else 0


def mate_names(mate: bytes, n: int):
    """the n names of a mate text: its even lines.  NameRefused("mate") unless it is 2 n complete lines of at most 255 bytes"""
    if mate and not mate.endswith(b"\n"):
        raise NameRefused("mate", "no last newline")
    lines = mate.split(b"\n")[:-1] if mate else []
    if len(lines) != 2 * n:
        raise NameRefused("mate", "%d lines for %d records" % (len(lines), n))
    if any(len(l) > NAME_MAX for l in lines):
        raise NameRefused("mate", "a line above 255 bytes")
    return lines[0::2]


def ref_streams_mate(text: bytes, n: int, mate: bytes):
    lines = NR.split_lines(text, n)
    mnames = mate_names(mate, n)
    s = {k: bytearray() for k in STREAMS}
    lit_len, lit_bytes = bytearray(), bytearray()
    for r in range(n):
        name, plus = lines[2 * r], lines[2 * r + 1]
        if len(name) > NAME_MAX or len(plus) > NAME_MAX:
            raise ValueError("record %d: a line above 255 bytes" % (r + 1))
        ref = NR.tokens(mnames[r])                                     # the mate's name r, cut anew; its '+' line is not looked at
        for t, (num, b) in enumerate(NR.tokens(name)):
            p = ref[t] if t < len(ref) else None
            if p is not None and p == (num, b):
                s["ops"].append(MATCH)
            elif p is not None and num and p[0] and int(b) == int(p[1]) + 1:
                s["ops"].append(INC)
            elif p is not None and num and p[0] and 2 <= int(b) - int(p[1]) <= 255:
                s["ops"].append(DELTA); s["delta"].append(int(b) - int(p[1]))
            elif num:
                s["ops"].append(NUM); s["num"] += struct.pack("<I", int(b))
            else:
                s["ops"].append(TEXT); s["tlen"].append(len(b)); s["text"] += b
        s["ops"].append(END)
        if not plus:
            s["plus"].append(0)
        elif plus == name:
            s["plus"].append(1)
        else:
            s["plus"].append(2); lit_len.append(len(plus)); lit_bytes += plus
    s["ptext"] = lit_len + lit_bytes
    return {k: bytes(v) for k, v in s.items()}


def mate_header(n, text_len, crc, mate_crc, lens, recs_per_seg=1):
    return NR.ref_header(KIND_MATE, n, text_len, crc, recs_per_seg, lens)[:88] + struct.pack("<II", mate_crc, 0)


def member_of_streams_mate(streams, n, text_len, crc, mate_crc, bwt_encode, recs_per_seg=1):
    """a kind-2 member of given raw streams (tests craft hostile ones through this)"""
    parts = [bwt_encode(streams[k]) if streams[k] else b"" for k in STREAMS]
    return mate_header(n, text_len, crc, mate_crc, [len(p) for p in parts], recs_per_seg) + b"".join(parts)


def ref_encode_mate(text: bytes, n: int, mate: bytes, bwt_encode, rans_encode, kind=None) -> bytes:
    """the member without a mate is made as well; kind 2 is kept only where it is strictly smaller"""
    m2 = member_of_streams_mate(ref_streams_mate(text, n, mate), n, len(text), _crc(text), _crc(mate), bwt_encode)
    if kind == KIND_MATE:
        return m2
    alone = NR.ref_encode(text, n, bwt_encode, rans_encode, kind=kind)
    return m2 if kind is None and len(m2) < len(alone) else alone


def ref_decode_mate(member: bytes, mate: bytes, bwt_decode, rans_decode) -> bytes:
    if len(member) < NR.HEADER or member[:4] != b"MCNM" or member[4] != 1:
        raise NameRefused("header", "magic or version")
    if member[5] != KIND_MATE:
        return NR.ref_decode(member, bwt_decode, rans_decode)          # kinds 0 and 1 do not look at the mate
    cap, zero = member[6], member[7]
    n, text_len, crc, rps, zero2 = struct.unpack_from("<QQIHH", member, 8)
    lens = struct.unpack_from("<7Q", member, 32)
    mate_crc, zero3 = struct.unpack_from("<II", member, 88)
    if cap != TOKEN_CAP or zero or zero2 or zero3:
        raise NameRefused("header", "token cap or reserved bytes")
    if rps != 1:
        raise NameRefused("header", "recs_per_seg %d with kind 2" % rps)
    if n > NR.N_MAX or text_len > NR.RAW_MAX or not 2 * n <= text_len <= 512 * n:
        raise NameRefused("header", "ranges")
    rest = member[NR.HEADER:]
    if sum(lens) != len(rest) or any(0 < l < 72 for l in lens):
        raise NameRefused("header", "member lengths")
    mnames = mate_names(mate, n)
    if _crc(mate) != mate_crc:
        raise NameRefused("mate", "crc")
    parts, at = {}, 0
    for k, l in zip(STREAMS, lens):
        parts[k] = rest[at:at + l]; at += l
    raw = {k: NR._bwt_raw_len(parts[k]) if parts[k] else 0 for k in STREAMS}
    if any(parts[k] and raw[k] == 0 for k in STREAMS):
        raise NameRefused("raw lengths", "an empty member")
    if raw["plus"] != n or not n <= raw["ops"] <= 25 * n or raw["num"] % 4:
        raise NameRefused("raw lengths", "ops, plus or num")
    if raw["delta"] + raw["num"] // 4 + raw["tlen"] > raw["ops"] - n or raw["text"] > text_len - 2 * n or raw["ptext"] > text_len - n:
        raise NameRefused("raw lengths", "more than the tokens allow")
    s = {}
    for k in STREAMS:
        if not parts[k]:
            s[k] = b""
            continue
        try:
            s[k] = bwt_decode(parts[k])
        except Exception as e:
            raise NameRefused("embedded", f"{k}: {e}")
        if len(s[k]) != raw[k]:
            raise NameRefused("embedded", f"{k}: length")
    ops = s["ops"]
    if any(o > END for o in ops):
        raise NameRefused("op above 5")
    if ops.count(END) != n or (n and ops[-1] != END):
        raise NameRefused("END count")
    if ops.count(DELTA) != len(s["delta"]) or 4 * ops.count(NUM) != len(s["num"]) or ops.count(TEXT) != len(s["tlen"]):
        raise NameRefused("op counts")
    if sum(s["tlen"]) != len(s["text"]):
        raise NameRefused("tlen sum")
    if any(p > 2 for p in s["plus"]):
        raise NameRefused("plus kind")
    K = s["plus"].count(2)
    if K > len(s["ptext"]) or K + sum(s["ptext"][:K]) != len(s["ptext"]):
        raise NameRefused("ptext")
    if b"\n" in s["text"] or b"\n" in s["ptext"][K:]:
        raise NameRefused("newline")
    out = bytearray()
    io = idl = inum = itl = itx = 0
    lit, lit_at = 0, K
    for r in range(n):
        ref = NR.tokens(mnames[r])
        cur = []
        while True:
            op = ops[io]; io += 1
            if op == END:
                break
            t = len(cur)
            if t == TOKEN_CAP:
                raise NameRefused("25th token")
            if op in (MATCH, INC, DELTA):
                if t >= len(ref):
                    raise NameRefused("no mate token")
                num, b = ref[t]
                if op != MATCH:
                    if not num:
                        raise NameRefused("no mate token", "wrong class")
                    d = 1
                    if op == DELTA:
                        d = s["delta"][idl]; idl += 1
                    v = int(b) + d
                    if v >= VALUE_END:
                        raise NameRefused("value")
                    b = b"%d" % v
                cur.append(b)
            elif op == NUM:
                v = struct.unpack_from("<I", s["num"], 4 * inum)[0]; inum += 1
                if v >= VALUE_END:
                    raise NameRefused("value")
                cur.append(b"%d" % v)
            else:
                l = s["tlen"][itl]; itl += 1
                cur.append(s["text"][itx:itx + l]); itx += l
            if sum(len(b) for b in cur) > NAME_MAX:
                raise NameRefused("name above 255")
        name = b"".join(cur)
        p = s["plus"][r]
        if p == 0:
            plus = b""
        elif p == 1:
            plus = name
        else:
            l = s["ptext"][lit]; lit += 1
            plus = s["ptext"][lit_at:lit_at + l]; lit_at += l
        out += name + b"\n" + plus + b"\n"
        if len(out) > text_len:
            raise NameRefused("text length")
    if len(out) != text_len:
        raise NameRefused("text length")
    if _crc(bytes(out)) != crc:
        raise NameRefused("crc")
    return bytes(out)


# ---- self-check: no library, stand-in coders that only frame the bytes ---------------------------------------------------------------------
def _frame(b: bytes) -> bytes:
    return b"MCBW" + bytes(4) + struct.pack("<Q", len(b)) + bytes(56) + b


def _unframe(m: bytes) -> bytes:
    return m[72:]


def self_check(frame=_frame, unframe=_unframe):
    """frame / unframe: the coders of the embedded members (the stand-ins by default).  Returns (a kind-2 member, its mate, its text)."""
    names2 = [b"r%d/2" % i for i in range(300)] + [b"", b"x7", b"a1b2c3", b"k10", b"k300", b"lead007", b"same"]
    names1 = [b"r%d/1" % i for i in range(300)] + [b"y", b"", b"a1", b"k8", b"k44", b"lead007", b"same"]
    plus2 = [b"" if i % 3 == 0 else nm if i % 3 == 1 else b"lit%d" % i for i, nm in enumerate(names2)]
    text = b"".join(a + b"\n" + p + b"\n" for a, p in zip(names2, plus2))
    mate = b"".join(a + b"\nmate plus\n" for a in names1)
    n = len(names2)
    s = ref_streams_mate(text, n, mate)
    assert s["ops"][:4] == bytes([MATCH, MATCH, MATCH, INC]) and s["ops"][4] == END
    assert s["ops"].count(DELTA) == 1 and s["delta"] == bytes([2])            # k8 -> k10; k44 -> k300 is +256: NUM
    m = ref_encode_mate(text, n, mate, frame, lambda b: bytes(32) + b, kind=2)
    assert m[5] == 2 and struct.unpack_from("<H", m, 28)[0] == 1 and struct.unpack_from("<I", m, 88)[0] == _crc(mate)
    assert ref_decode_mate(m, mate, unframe, None) == text
    for bad_mate, rule in ((mate[:-1] + b"x\n", "mate"), (mate + b"a\n\n", "mate"), (mate[:mate.rindex(b"same")], "mate")):
        try:
            ref_decode_mate(m, bad_mate, unframe, None)
        except NameRefused as e:
            assert e.rule == rule, e.rule
        else:
            raise AssertionError("a mate that is not the member's was taken")
    try:
        NR.ref_decode(m, unframe, None)
    except NameRefused as e:
        assert e.rule == "header"
    else:
        raise AssertionError("kind 2 was taken without a mate")
    # a MATCH where the mate has no token: the second record of a two-record text against a mate whose second name is empty
    text2, mate2 = b"ab\n\nab\n\n", b"ab\n\n\n\n"
    hostile = member_of_streams_mate(dict(ops=bytes([0, 5, 0, 5]), delta=b"", num=b"", tlen=b"", text=b"", plus=bytes(2), ptext=b""), 2, len(text2), _crc(text2), _crc(mate2), frame)
    try:
        ref_decode_mate(hostile, mate2, unframe, None)
    except NameRefused as e:
        assert e.rule == "no mate token"
    else:
        raise AssertionError("MATCH past the mate's tokens was taken")
    return m, mate, text


if __name__ == "__main__":
    self_check()
    print("mate_name_reference: self-check passed")
