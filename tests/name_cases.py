"""Inputs for the read-name coder's tests (tests/test_names.py, tests/test_gpu_names.py): generators with fixed seeds, the degenerate
name texts of DESIGN.md section 3.10 and one crafted member per refusal rule.  A case is (id, names, plus): two lists of bytes."""
import functools
import struct
import zlib

import numpy as np

import name_reference as NR


def text_of(names, plus=None) -> bytes:
    plus = [b""] * len(names) if plus is None else plus
    return b"".join(a + b"\n" + b + b"\n" for a, b in zip(names, plus))


def illumina(seed: int, n: int):
    """A00123:45:HXXXXDSXX:<lane>:<tile>:<x>:<y> 1:N:0:ACGTACGT+TTGCAAGC -- x creeps up by 0 .. 39, tile and lane roll over, y uniform"""
    rng = np.random.default_rng(seed)
    step = rng.integers(0, 40, n); y = rng.integers(1000, 200001, n)
    out, lane, tile, x = [], 1, 1101, 1000
    for i in range(n):
        x += int(step[i])
        if x > 32000:
            x = 1000 + int(step[i]); tile += 1
            if tile > 1120:
                tile = 1101; lane = lane % 4 + 1
        out.append(b"A00123:45:HXXXXDSXX:%d:%d:%d:%d 1:N:0:ACGTACGT+TTGCAAGC" % (lane, tile, x, int(y[i])))
    return out


def sra(seed: int, n: int):
    """SRR001666.<i> 071112_SLXA-EAS1_s_7:5:<i/5000+1>:<0..999>:<0..999> length=36"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1000, n); b = rng.integers(0, 1000, n)
    return [b"SRR001666.%d 071112_SLXA-EAS1_s_7:5:%d:%d:%d length=36" % (i + 1, i // 5000 + 1, int(a[i]), int(b[i])) for i in range(n)]


def mixed_plus(names, seed: int = 5):
    """third lines that are bare, equal to the name and other text, mixed"""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 3, len(names))
    return [b"" if k == 0 else nm if k == 1 else b"lit %d\t+@" % i for i, (k, nm) in enumerate(zip(kind, names))]


@functools.lru_cache(maxsize=None)
def degenerate():
    """(id, names, plus) -- every one a name text the coder must take"""
    c = []
    for n in (0, 1, 255, 256, 257, 513):
        nm = illumina(n + 1, n)
        c.append(("n%d" % n, nm, mixed_plus(nm, n)))
    c.append(("empty_names", [b"", b"", b"a", b""], [b"", b"x", b"", b""]))
    c.append(("len255", [b"r" * 255, b"q" * 254 + b"7", b"1" * 255], [b"r" * 255, b"p" * 255, b""]))
    tok24 = b".".join(b"%d" % k for k in range(12)) + b"."                # 12 numeric + 12 text: exactly 24 tokens
    tok25 = tok24 + b"5"                                                   # a 25th run: token 23 is ".5"
    tok30 = b".".join(b"%d" % (k + 3) for k in range(15))
    assert len(NR._RUNS.findall(tok24)) == 24 and len(NR._RUNS.findall(tok25)) == 25
    c.append(("tokens_24_25", [tok24, tok24, tok25, tok25, tok30, tok24, b"x"], None))
    c.append(("number_edges", [b"a999999999", b"a1000000000", b"a007", b"a0", b"a1", b"a999999998", b"a999999999", b"a1000000000", b"a0", b"a00", b"0", b"01", b"1"], None))
    c.append(("steps", [b"r10", b"r11", b"r13", b"r268", b"r524", b"r523", b"r523", b"r778", b"r779"], None))
    c.append(("class_changes", [b"ab:12", b"12:ab", b"ab:12", b"77", b"zz", b"5x", b"x5"], None))
    c.append(("token_counts", [b"a1b2c3", b"a1", b"a1b2c3d4e5", b"", b"a1b2", b"a"], None))
    c.append(("bytes", [b"\xff\xfe1\x80", b"a\tb 1", b"@x+y@", b"+", b"@", b"\x00\x01", b"\xff\xfe2\x80"], [b"\xff", b"a\tb 1", b"+", b"", b"@@", b"", b"\xff\xfe2\x80"]))
    nm = sra(3, 40)
    c.append(("plus_mixed", nm, mixed_plus(nm, 9)))
    c.append(("plus_all_name", nm, list(nm)))
    c.append(("plus_all_literal", nm, [b"x%d" % i for i in range(40)]))
    return tuple(c)


def refused_inputs():
    """(id, text, n, the record the encoder must name or None)"""
    long_name = text_of([b"ok", b"n" * 256, b"m" * 300])
    long_plus = text_of([b"ok", b"ok2"], [b"", b"p" * 256])
    return [("name256", long_name, 3, 1), ("plus256", long_plus, 2, 1), ("odd_lines", b"a\n\nb\n", 2, None), ("no_last_newline", b"a\n\nb\nc", 2, None),
            ("too_few_lines", b"a\n\n", 2, None)]


# ---- hostile members -----------------------------------------------------------------------------------------------------------------------
def _bwt(b: bytes) -> bytes:
    from minicom_amd import pipeline
    return pipeline.bwt_encode(b)


def _rans(b: bytes) -> bytes:
    from minicom_amd import pipeline
    return pipeline.rans_encode(b)


def small():
    """(text, n, the kind-0 member of it): 300 records, two segments, every stream in use"""
    nm = illumina(11, 300)
    nm[7] = b"other:name"; nm[8] = b"other:name"
    text = text_of(nm, mixed_plus(nm, 2))
    return text, 300, NR.ref_encode(text, 300, _bwt, _rans, kind=0)


def _member(streams, text, n, rps=256):
    return NR.member_of_streams(streams, n, len(text), zlib.crc32(text) & 0xFFFFFFFF, rps, _bwt)


def noncanonical():
    """(id, member, text): well-formed members the canonical encoder would not write; they decode"""
    out = []
    # TEXT ops for digits, NUM where MATCH applies, a DELTA of 1 and of 0
    names = [b"r12", b"r12", b"r13", b"r13"]
    text = text_of(names)
    s = dict(ops=bytes([4, 4, 5, 4, 3, 5, 0, 2, 5, 0, 2, 5]), delta=bytes([1, 0]), num=struct.pack("<I", 12), tlen=bytes([1, 2, 1]), text=b"r12r",
             plus=bytes(4), ptext=b"")
    out.append(("text_for_digits", _member(s, text, 4), text))
    # plus = 1 on an empty name, a literal that equals the name, an empty literal, an empty text token
    names = [b"", b"ab", b"cd", b"x"]; plus = [b"", b"ab", b"", b"x"]
    text = text_of(names, plus)
    s = dict(ops=bytes([5, 4, 5, 4, 5, 4, 4, 5]), delta=b"", num=b"", tlen=bytes([2, 2, 0, 1]), text=b"abcdx", plus=bytes([1, 2, 2, 1]), ptext=bytes([2, 0]) + b"ab")
    out.append(("plus_forms", _member(s, text, 4), text))
    return out


@functools.lru_cache(maxsize=None)
def crafted():
    """(id, the rule name_reference.py names, member): one member per refusal rule of section 3.10, each a well-formed container"""
    text, n, base = small()
    S = NR.ref_streams(text, n)
    out = []

    def put(name, rule, **chg):
        s = dict(S); s.update(chg)
        out.append((name, rule, _member(s, text, n)))

    ops = bytearray(S["ops"])
    first_end = ops.index(5)
    put("op6", "op above 5", ops=bytes(ops[:2]) + b"\x06" + bytes(ops[3:]))
    put("end_missing", "END count", ops=bytes(ops[:first_end]) + b"\x00" + bytes(ops[first_end + 1:]))
    put("last_not_end", "END count", ops=bytes(ops[:-2]) + bytes([5, 0]))
    put("delta_count", "op counts", delta=S["delta"] + b"\x05")
    put("num_count", "op counts", num=S["num"] + struct.pack("<I", 7))
    put("tlen_count", "op counts", tlen=S["tlen"] + b"\x01", text=S["text"] + b"x")
    put("tlen_sum", "tlen sum", text=S["text"] + b"x")
    put("plus_short", "raw lengths", plus=S["plus"][:-1])
    put("plus_kind3", "plus kind", plus=b"\x03" + S["plus"][1:])
    put("ptext_left_over", "ptext", ptext=S["ptext"] + b"z")
    put("ptext_short", "ptext", ptext=S["ptext"][:-1])
    put("newline_in_text", "newline", text=S["text"][:3] + b"\n" + S["text"][4:])
    k = S["plus"].count(2)
    put("newline_in_literal", "newline", ptext=S["ptext"][:k] + b"\n" + S["ptext"][k + 1:])
    # MATCH at the first record of the second segment: no previous token there
    seg2 = 0
    ends = 0
    for i, o in enumerate(ops):
        ends += o == 5
        if ends == 256:
            seg2 = i + 1; break
    assert ops[seg2] == 4
    tl, tx = _drop_tlen(S, ops, seg2)
    put("match_without_previous", "no previous token", ops=bytes(ops[:seg2]) + b"\x00" + bytes(ops[seg2 + 1:]), tlen=tl, text=tx)
    # small hand-made members for the walk's own rules
    def tiny(name, rule, names_text, n_rec, **s):
        full = dict(ops=b"", delta=b"", num=b"", tlen=b"", text=b"", plus=bytes(n_rec), ptext=b"")
        full.update(s)
        out.append((name, rule, _member(full, names_text, n_rec)))
    tiny("inc_on_text", "no previous token", b"ab\n\nab\n\n", 2, ops=bytes([4, 5, 1, 5]), tlen=b"\x02", text=b"ab")
    tiny("delta_on_text", "no previous token", b"ab\n\nab\n\n", 2, ops=bytes([4, 5, 2, 5]), tlen=b"\x02", text=b"ab", delta=b"\x03")
    tiny("match_beyond_previous", "no previous token", b"ab\n\nabab\n\n", 2, ops=bytes([4, 5, 0, 0, 5]), tlen=b"\x02", text=b"ab")
    tiny("num_1e9", "value", b"1000000000\n\n", 1, ops=bytes([3, 5]), num=struct.pack("<I", 10 ** 9))
    tiny("inc_to_1e9", "value", b"999999999\n\n1000000000\n\n", 2, ops=bytes([3, 5, 1, 5]), num=struct.pack("<I", 10 ** 9 - 1))
    tiny("delta_to_1e9", "value", b"999999990\n\n1000000000\n\n", 2, ops=bytes([3, 5, 2, 5]), num=struct.pack("<I", 10 ** 9 - 10), delta=b"\x0a")
    t25 = b"".join(b"a" for _ in range(25))
    tiny("token_25", "25th token", t25 + b"\n\n\n\n", 2, ops=bytes([4] * 25 + [5, 5]), tlen=bytes([1] * 25), text=t25)
    tiny("name_256", "name above 255", b"x" * 256 + b"\n\n", 1, ops=bytes([4, 4, 5]), tlen=bytes([200, 56]), text=b"x" * 256)
    tiny("text_len_short", "text length", b"ab\n\n", 1, ops=bytes([4, 5]), tlen=b"\x01", text=b"a")
    # the container itself
    crc_bad = bytearray(base); crc_bad[24] ^= 1
    out.append(("crc", "crc", bytes(crc_bad)))
    for name, at, val in (("magic", 0, ord("X")), ("version", 4, 2), ("kind", 5, 2), ("token_cap", 6, 23), ("reserved7", 7, 1), ("rps0", 28, 0), ("reserved88", 90, 1)):
        b = bytearray(base); b[at] = val
        if name == "rps0":
            b[29] = 0
        out.append((name, "header", bytes(b)))
    b = bytearray(base); b[28:30] = struct.pack("<H", 4097); out.append(("rps4097", "header", bytes(b)))
    b = bytearray(base); b[8:16] = struct.pack("<Q", n + 1); out.append(("another_n", "raw lengths", bytes(b)))
    b = bytearray(base); b[32:40] = struct.pack("<Q", struct.unpack_from("<Q", base, 32)[0] + 1); out.append(("member_lengths", "header", bytes(b)))
    b = bytearray(base); b[96 + 8:96 + 16] = struct.pack("<Q", struct.unpack_from("<Q", base, 96 + 8)[0] + 4); out.append(("embedded_raw_len", "embedded", bytes(b)))
    return tuple(out)


def _drop_tlen(S, ops, at):
    """the tlen and text streams without the entry of the TEXT op at ops[at]"""
    k = bytes(ops[:at]).count(4)
    off = sum(S["tlen"][:k]); l = S["tlen"][k]
    return S["tlen"][:k] + S["tlen"][k + 1:], S["text"][:off] + S["text"][off + l:]


def truncations():
    _, _, base = small()
    return [base[:k] for k in sorted(set(list(range(0, 200, 7)) + [95, 96, 97, len(base) // 2, len(base) - 1]))] + [base + b"\x00"]


def bit_flips(count: int = 200, seed: int = 77):
    _, _, base = small()
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        b = bytearray(base)
        at = int(rng.integers(0, len(b))); b[at] ^= 1 << int(rng.integers(0, 8))
        out.append(bytes(b))
    return out
