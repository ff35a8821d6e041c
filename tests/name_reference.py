"""An independent reference for the `.mcn` member format, written from DESIGN.md section 3.10 and from nothing else: it shares no
code with csrc/name_model.hpp.  The embedded `.bwt` and `.rans` members are not its business: the caller hands it coders for them
(bwt_encode / bwt_decode / rans_encode / rans_decode: bytes -> bytes), as qual_reference.py is handed the `.rans` member.

    ref_streams(text, n, recs_per_seg)      -> the seven raw streams
    ref_encode(text, n, bwt_encode, rans_encode, recs_per_seg=256, kind=None) -> the member
    ref_decode(member, bwt_decode, rans_decode) -> the name text; NameRefused(rule) for every member the section refuses
"""
import re
import struct
import zlib

HEADER = 96
STREAMS = ("ops", "delta", "num", "tlen", "text", "plus", "ptext")
MATCH, INC, DELTA, NUM, TEXT, END = range(6)
TOKEN_CAP, NAME_MAX, VALUE_END = 24, 255, 10 ** 9
N_MAX = 0xFFFFFFFF // 25
RAW_MAX = 0xFFFFFFFE
_RUNS = re.compile(rb"[0-9]+|[^0-9]+", re.S)


class NameRefused(Exception):
    def __init__(self, rule, detail=""):
        super().__init__(f"{rule}: {detail}" if detail else rule)
        self.rule = rule


def tokens(name: bytes):
    """[(is_numeric, bytes)]: maximal digit runs and maximal other runs; a digit run of at most 9 digits without a leading zero (or
    the single digit 0) is numeric; at most 24 tokens, the 24th is the whole rest as text"""
    out, at = [], 0
    for m in _RUNS.finditer(name):
        if len(out) == TOKEN_CAP - 1:
            break
        run = m.group()
        numeric = run[:1].isdigit() and len(run) <= 9 and (run == b"0" or run[:1] != b"0")
        out.append((numeric, run))
        at = m.end()
    if at < len(name):
        out.append((False, name[at:]))
    return out


def split_lines(text: bytes, n: int):
    if text and not text.endswith(b"\n"):
        raise ValueError("the name text does not end with a newline")
    lines = text.split(b"\n")[:-1] if text else []
    if len(lines) != 2 * n:
        raise ValueError("%d lines, not two per record" % len(lines))
    return lines


def ref_streams(text: bytes, n: int, recs_per_seg: int = 256):
    lines = split_lines(text, n)
    s = {k: bytearray() for k in STREAMS}
    lit_len, lit_bytes = bytearray(), bytearray()
    prev = []
    for r in range(n):
        name, plus = lines[2 * r], lines[2 * r + 1]
        if len(name) > NAME_MAX or len(plus) > NAME_MAX:
            raise ValueError("record %d: a line above 255 bytes" % (r + 1))
        if r % recs_per_seg == 0:
            prev = []
        cur = tokens(name)
        for t, (num, b) in enumerate(cur):
            p = prev[t] if t < len(prev) else None
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
        prev = cur
        if not plus:
            s["plus"].append(0)
        elif plus == name:
            s["plus"].append(1)
        else:
            s["plus"].append(2); lit_len.append(len(plus)); lit_bytes += plus
    s["ptext"] = lit_len + lit_bytes
    return {k: bytes(v) for k, v in s.items()}


def ref_header(kind, n, text_len, crc, recs_per_seg, lens, cap=TOKEN_CAP):
    return b"MCNM" + bytes([1, kind, cap, 0]) + struct.pack("<QQIHH", n, text_len, crc, recs_per_seg, 0) + struct.pack("<7Q", *lens) + bytes(8)


def member_of_streams(streams, n, text_len, crc, recs_per_seg, bwt_encode):
    """a kind-0 member of given raw streams (tests craft hostile ones through this)"""
    parts = [bwt_encode(streams[k]) if streams[k] else b"" for k in STREAMS]
    return ref_header(0, n, text_len, crc, recs_per_seg, [len(p) for p in parts]) + b"".join(parts)


def ref_encode(text: bytes, n: int, bwt_encode, rans_encode, recs_per_seg: int = 256, kind=None) -> bytes:
    crc = zlib.crc32(text) & 0xFFFFFFFF if text else 0
    m0 = member_of_streams(ref_streams(text, n, recs_per_seg), n, len(text), crc, recs_per_seg, bwt_encode)
    if n == 0 or kind == 0:
        return m0
    m1 = ref_header(1, n, len(text), crc, 256, [0] * 7) + rans_encode(text)
    if kind == 1 or (kind is None and len(m1) < len(m0)):
        return m1
    return m0


def _bwt_raw_len(member: bytes) -> int:
    if len(member) < 72 or member[:4] != b"MCBW":
        raise NameRefused("embedded", "not a .bwt header")
    return struct.unpack_from("<Q", member, 8)[0]


def ref_decode(member: bytes, bwt_decode, rans_decode) -> bytes:
    if len(member) < HEADER or member[:4] != b"MCNM" or member[4] != 1:
        raise NameRefused("header", "magic or version")
    kind, cap, zero = member[5], member[6], member[7]
    n, text_len, crc, rps, zero2 = struct.unpack_from("<QQIHH", member, 8)
    lens = struct.unpack_from("<7Q", member, 32)
    if kind > 1 or cap != TOKEN_CAP or zero or zero2 or member[88:96] != bytes(8):
        raise NameRefused("header", "kind, token cap or reserved bytes")
    if not 1 <= rps <= 4096 or n > N_MAX or text_len > RAW_MAX or not 2 * n <= text_len <= 512 * n:
        raise NameRefused("header", "ranges")
    rest = member[HEADER:]
    if kind == 1:
        if n == 0 or any(lens):
            raise NameRefused("header", "kind 1 with streams or without records")
        try:
            text = rans_decode(rest)
        except Exception as e:
            raise NameRefused("embedded", str(e))
        if len(text) != text_len or (zlib.crc32(text) & 0xFFFFFFFF) != crc or struct.unpack_from("<I", rest, 16)[0] != crc:
            raise NameRefused("embedded", "length or CRC")
        lines = text.split(b"\n")
        if lines[-1] != b"" or len(lines) - 1 != 2 * n or any(len(l) > NAME_MAX for l in lines):
            raise NameRefused("lines")
        return text
    if sum(lens) != len(rest) or any(0 < l < 72 for l in lens):
        raise NameRefused("header", "member lengths")
    s, at = {}, 0
    parts = {}
    for k, l in zip(STREAMS, lens):
        parts[k] = rest[at:at + l]; at += l
    raw = {k: _bwt_raw_len(parts[k]) if parts[k] else 0 for k in STREAMS}
    # what can be told before a stream is decoded
    tokens_in_all = raw["ops"] - n
    if any(parts[k] and raw[k] == 0 for k in STREAMS):
        raise NameRefused("raw lengths", "an empty member")
    if raw["plus"] != n or not n <= raw["ops"] <= 25 * n or raw["num"] % 4:
        raise NameRefused("raw lengths", "ops, plus or num")
    if raw["delta"] + raw["num"] // 4 + raw["tlen"] > tokens_in_all or raw["text"] > text_len - 2 * n or raw["ptext"] > text_len - n:
        raise NameRefused("raw lengths", "more than the tokens allow")
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
    prev = []
    for r in range(n):
        if r % rps == 0:
            prev = []
        cur = []
        while True:
            op = ops[io]; io += 1
            if op == END:
                break
            t = len(cur)
            if t == TOKEN_CAP:
                raise NameRefused("25th token")
            if op in (MATCH, INC, DELTA):
                if t >= len(prev):
                    raise NameRefused("no previous token")
                num, b = prev[t]
                if op != MATCH:
                    if not num:
                        raise NameRefused("no previous token", "wrong class")
                    d = 1
                    if op == DELTA:
                        d = s["delta"][idl]; idl += 1
                    v = int(b) + d
                    if v >= VALUE_END:
                        raise NameRefused("value")
                    b = b"%d" % v
                cur.append((num, b))
            elif op == NUM:
                v = struct.unpack_from("<I", s["num"], 4 * inum)[0]; inum += 1
                if v >= VALUE_END:
                    raise NameRefused("value")
                cur.append((True, b"%d" % v))
            else:
                l = s["tlen"][itl]; itl += 1
                cur.append((False, s["text"][itx:itx + l])); itx += l
            if sum(len(b) for _, b in cur) > NAME_MAX:
                raise NameRefused("name above 255")
        name = b"".join(b for _, b in cur)
        prev = cur
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
    if (zlib.crc32(bytes(out)) & 0xFFFFFFFF if out else 0) != crc:
        raise NameRefused("crc")
    return bytes(out)
