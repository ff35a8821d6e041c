"""Inputs for the tests of `.mcn` kind 2 (tests/test_mate_names.py, tests/test_gpu_mate_names.py): pairs of name
texts with fixed seeds, one crafted member per refusal rule, truncations and bit flips.  A case is (id, names, plus, mate names, mate plus):
four lists of bytes, `names` the second file's and `mate names` the first file's."""
import functools
import struct
import zlib

import numpy as np

import mate_name_reference as MR
import name_cases as nc
import name_reference as NR

text_of = nc.text_of


def illumina_pair(seed: int, n: int):
    """(file 1, file 2): `... 1:N:0:...` and `... 2:N:0:...`"""
    a = nc.illumina(seed, n)
    return a, [x.replace(b" 1:N:0:", b" 2:N:0:") for x in a]


def slash_pair(seed: int, n: int):
    """(file 1, file 2): `<name>/1` and `<name>/2`"""
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 30000, n); y = rng.integers(1, 30000, n)
    base = [b"HWUSI-EAS100R:6:73:%d:%d#0" % (int(a), int(b)) for a, b in zip(x, y)]
    return [b + b"/1" for b in base], [b + b"/2" for b in base]


def sra_pair(seed: int, n: int):
    """(file 1, file 2): the same names in both files"""
    a = nc.sra(seed, n)
    return a, list(a)


STYLES = (("illumina", illumina_pair), ("slash", slash_pair), ("sra", sra_pair))


@functools.lru_cache(maxsize=None)
def cases():
    c = []
    for n in (0, 1, 2, 255, 256, 257, 1000):
        a, b = illumina_pair(n + 3, n)
        c.append(("n%d" % n, b, nc.mixed_plus(b, n), a, None))
    a, b = sra_pair(2, 300)
    c.append(("identical", b, None, a, None))
    a, b = slash_pair(4, 300)
    c.append(("inc", b, None, a, None))
    steps = [0, 1, 2, 3, 17, 254, 255, 256, 257, 1000, -1, -2]
    c.append(("steps", [b"run%d:x" % (5000 + s) for s in steps] * 30, None, [b"run5000:x"] * (30 * len(steps)), None))
    c.append(("text_differs", [b"tile%d.fwd:9" % i for i in range(200)], None, [b"tile%d.rev:9" % i for i in range(200)], None))
    c.append(("mate_fewer_tokens", [b"a1b2c3d4"] * 100 + [b"q7:8:9"], None, [b"a1b2"] * 100 + [b"q7"], None))
    c.append(("mate_more_tokens", [b"a1b2"] * 100 + [b"q7"], None, [b"a1b2c3d4"] * 100 + [b"q7:8:9"], None))
    c.append(("empty_against_name", [b"", b"", b"x1"] * 40, None, [b"r5", b"", b""] * 40, None))
    c.append(("name_against_empty", [b"r5", b"", b""] * 40, None, [b"", b"", b"x1"] * 40, None))
    run23 = b".".join(b"%d" % (k + 2) for k in range(12))                  # 12 numeric + 11 text: 23 runs
    run24 = run23 + b"."
    run30 = b".".join(b"%d" % (k + 3) for k in range(15)) + b"."
    assert [len(NR._RUNS.findall(x)) for x in (run23, run24, run30)] == [23, 24, 30]
    caps = [run23, run24, run30, run30 + b"tail9", run24 + b"7"]
    c.append(("token_cap", caps * 20, None, (caps[1:] + caps[:1]) * 20, None))
    c.append(("token_cap_same", caps * 20, None, caps * 20, None))
    long2 = [b"r" * 255, b"q" * 250 + b"12345", b"1" * 255, b"s" * 255]
    long1 = [b"r" * 255, b"q" * 250 + b"12344", b"1" * 255, b"t" * 255]
    c.append(("len255", long2 * 10, [b"p" * 255, b"", b"1" * 255, b"s" * 255] * 10, long1 * 10, [b"m" * 255] * 40))
    zeros2 = [b"a007", b"a0", b"a00", b"a1234567890", b"a999999999", b"a1000000000", b"a0999", b"a10"]
    zeros1 = [b"a007", b"a00", b"a0", b"a1234567889", b"a999999998", b"a999999999", b"a999", b"a010"]
    c.append(("digit_runs", zeros2 * 15, None, zeros1 * 15, None))
    a, b = illumina_pair(9, 400)
    c.append(("plus_mixed", b, nc.mixed_plus(b, 9), a, None))
    c.append(("plus_all_name", b, list(b), a, None))
    c.append(("mate_plus_nonempty", b, None, a, nc.mixed_plus(a, 4)))
    c.append(("bytes", [b"\xff\xfe1\x80", b"a\tb 1", b"@x+y@", b"+", b"\x00\x01"] * 30, None, [b"\xff\xfe0\x80", b"a\tb 1", b"@x+y", b"@", b"\x00\x02"] * 30, None))
    c.append(("unrelated", nc.sra(5, 300), None, nc.illumina(6, 300), None))
    return tuple(c)


# ---- hostile members -----------------------------------------------------------------------------------------------------------------------
def _bwt(b: bytes) -> bytes:
    from minicom_amd import pipeline
    return pipeline.bwt_encode(b)


def _rans(b: bytes) -> bytes:
    from minicom_amd import pipeline
    return pipeline.rans_encode(b)


def _crc(b: bytes) -> int:
    return zlib.crc32(b) & 0xFFFFFFFF if b else 0


@functools.lru_cache(maxsize=None)
def small():
    """(text, n, mate, the kind-2 member of it): 300 records, every stream in use"""
    a, b = illumina_pair(11, 300)
    b[7] = b"other:name"; b[8] = b"x%s" % b[8]; b[9] = b[9].replace(b":45:", b":47:"); b[10] = b[10].replace(b":45:", b":4500:")
    text, mate = text_of(b, nc.mixed_plus(b, 2)), text_of(a, nc.mixed_plus(a, 5))
    m = MR.ref_encode_mate(text, 300, mate, _bwt, _rans, kind=2)
    assert all(struct.unpack_from("<7Q", m, 32))
    return text, 300, mate, m


def _tiny(names_text, n, mate, **s):
    full = dict(ops=b"", delta=b"", num=b"", tlen=b"", text=b"", plus=bytes(n), ptext=b"")
    full.update(s)
    return MR.member_of_streams_mate(full, n, len(names_text), _crc(names_text), _crc(mate), _bwt)


@functools.lru_cache(maxsize=None)
def crafted():
    """(id, the rule mate_name_reference.py names, member, mate): one per refusal rule of section 3.12, each a well-formed container"""
    text, n, mate, base = small()
    out = []
    b = bytearray(base); b[88] ^= 1
    out.append(("mate_crc", "mate", bytes(b), mate))
    a1, _ = illumina_pair(11, 301)
    out.append(("mate_n_plus_1", "mate", base, text_of(a1, nc.mixed_plus(a1, 5))))
    out.append(("mate_n_minus_1", "mate", base, text_of(a1[:299], nc.mixed_plus(a1, 5)[:299])))
    out.append(("mate_no_last_newline", "mate", base, mate[:-1]))
    out.append(("mate_empty", "mate", base, b""))
    b = bytearray(base); b[28:30] = struct.pack("<H", 256)
    out.append(("rps256", "header", bytes(b), mate))
    b = bytearray(base); b[92] = 1
    out.append(("reserved92", "header", bytes(b), mate))
    b = bytearray(base); b[5] = 3
    out.append(("kind3", "header", bytes(b), mate))
    # the walk's own rules, small hand-made members
    def tiny(name, rule, names_text, n_rec, mate_text, **s):
        out.append((name, rule, _tiny(names_text, n_rec, mate_text, **s), mate_text))
    tiny("match_past_mate", "no mate token", b"ab\n\nabab\n\n", 2, b"ab\n\nab\n\n", ops=bytes([0, 5, 0, 0, 5]))
    tiny("match_on_empty_mate", "no mate token", b"ab\n\n", 1, b"\n\n", ops=bytes([0, 5]))
    tiny("inc_on_text", "no mate token", b"ab\n\n", 1, b"ab\n\n", ops=bytes([1, 5]))
    tiny("delta_on_text", "no mate token", b"ab\n\n", 1, b"ab\n\n", ops=bytes([2, 5]), delta=b"\x03")
    tiny("inc_past_mate", "no mate token", b"a2\n\n", 1, b"a\n\n", ops=bytes([0, 1, 5]))
    tiny("delta_to_1e9", "value", b"1000000000\n\n", 1, b"999999990\n\n", ops=bytes([2, 5]), delta=b"\x0a")
    tiny("inc_to_1e9", "value", b"1000000000\n\n", 1, b"999999999\n\n", ops=bytes([1, 5]))
    tiny("num_1e9", "value", b"1000000000\n\n", 1, b"5\n\n", ops=bytes([3, 5]), num=struct.pack("<I", 10 ** 9))
    t25 = b"a" * 25
    tiny("token_25", "25th token", t25 + b"\n\n\n\n", 2, b"z\n\n\n\n", ops=bytes([4] * 25 + [5, 5]), tlen=bytes([1] * 25), text=t25)
    # a name of 256 bytes: token 0 matched, 255 bytes from the mate text, then one digit more
    tiny("name_256_by_match", "name above 255", b"m" * 255 + b"7\n\n", 1, b"m" * 255 + b"\n\n", ops=bytes([0, 3, 5]), num=struct.pack("<I", 7))
    tiny("text_len_short", "text length", b"ab\n\n", 1, b"a\n\n", ops=bytes([0, 5]))
    tiny("op6", "op above 5", b"ab\n\n", 1, b"ab\n\n", ops=bytes([6, 5]))
    tiny("last_not_end", "END count", b"ab\n\n", 1, b"ab\n\n", ops=bytes([5, 0]))
    tiny("newline_in_text", "newline", b"a\nbcd\n\n\n", 2, b"x\n\ny\n\n", ops=bytes([4, 5, 5]), tlen=b"\x03", text=b"a\nb")
    tiny("plus_kind3", "plus kind", b"ab\n\n", 1, b"ab\n\n", ops=bytes([0, 5]), plus=b"\x03")
    tiny("delta_overrun", "op counts", b"a7\n\n", 1, b"a5\n\n", ops=bytes([0, 2, 5]))
    tiny("ptext_short", "ptext", b"ab\nxy\n", 1, b"ab\n\n", ops=bytes([0, 5]), plus=b"\x02", ptext=b"\x02x")
    b = bytearray(base); b[24] ^= 1
    out.append(("crc", "crc", bytes(b), mate))
    b = bytearray(base); b[8:16] = struct.pack("<Q", n + 1)
    out.append(("another_n", "mate", bytes(b), mate))
    b = bytearray(base); b[32:40] = struct.pack("<Q", struct.unpack_from("<Q", base, 32)[0] + 1)
    out.append(("member_lengths", "header", bytes(b), mate))
    return tuple(out)


def noncanonical():
    """(id, member, mate, text): well-formed kind-2 members the canonical encoder would not write; they decode"""
    out = []
    text, mate = b"r12\n\nr13\n\nab\n\n", b"r12\n+\nr12\nzz\nab\n\n"
    # TEXT for digits and DELTA of 1 and 0; NUM where MATCH applies; an empty text token in front of a MATCH of the second mate token
    s = dict(ops=bytes([0, 4, 5, 0, 2, 5, 4, 5]), delta=b"\x01", num=b"", tlen=bytes([2, 2]), text=b"12ab", plus=bytes(3), ptext=b"")
    out.append(("text_for_digits", _tiny(text, 3, mate, **s), mate, text))
    text, mate = b"x7\nx7\n", b"y7\n\n"
    s = dict(ops=bytes([4, 3, 5]), num=struct.pack("<I", 7), tlen=b"\x01", text=b"x", plus=b"\x02", ptext=b"\x02x7")
    out.append(("num_for_match_literal_for_name", _tiny(text, 1, mate, **s), mate, text))
    return out


def truncations():
    _, _, _, base = small()
    return [base[:k] for k in sorted(set(list(range(0, 200, 7)) + [95, 96, 97, len(base) // 2, len(base) - 1]))] + [base + b"\x00"]


def bit_flips(count: int = 200, seed: int = 78):
    _, _, _, base = small()
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        b = bytearray(base)
        at = int(rng.integers(0, len(b))); b[at] ^= 1 << int(rng.integers(0, 8))
        out.append(bytes(b))
    return out
