"""Inputs shared by tests/test_bwt.py (host twin) and tests/test_gpu_bwt.py (device): the synthetic members of the `.bwt` coder, the
members the independent reference (tests/bwt_reference.py) makes of them at block and anchor sizes no encoder writes, and one crafted
member per refusal rule of DESIGN.md section 3.8."""
import numpy as np

import bwt_reference as br
import entropy_cases as ec

BLK = 1 << br.BLK_LOG2
GEOMETRIES = ((8, 4), (8, 8), (12, 4), (12, 8))        # (blk_log2, anc_log2) the decoders are given


def text_member(golden_dir, size: int) -> bytes:
    m = ec.golden_members(golden_dir)
    name = max((k for k in m if "dif_char.txt" in k), key=lambda k: len(m[k]))
    assert len(m[name]) >= size, (name, len(m[name]))
    return m[name][:size]


def small_members(golden_dir):
    """the member list of the issue at sizes the reference can transform: with blocks of 2^8 and 2^12 bytes "one block", "one block + 1"
    and "a last block of 1 byte" are 256 / 4096 bytes and one more"""
    rng = np.random.default_rng(20261)
    unit = rng.integers(0, 256, size=1000, dtype=np.uint8).tobytes()
    return {
        "empty": b"",
        "one_byte": b"\x5a",
        "255_equal": b"\x07" * 255,
        "all_equal_5000": b"\x07" * 5000,
        "period_2_64k": b"ab" * (1 << 15),
        "period_1000_64k": (unit * 66)[:1 << 16],
        "uniform_random_10000": rng.integers(0, 256, size=10000, dtype=np.uint8).tobytes(),
        "one_block_2^8": rng.integers(0, 4, size=256, dtype=np.uint8).tobytes(),
        "one_block_2^8_plus_1": rng.integers(0, 4, size=257, dtype=np.uint8).tobytes(),
        "one_block_2^12": rng.integers(0, 4, size=4096, dtype=np.uint8).tobytes(),
        "one_block_2^12_plus_1": rng.integers(0, 4, size=4097, dtype=np.uint8).tobytes(),       # (the last block is 1 byte)
        "text_dif_char": text_member(golden_dir, 8000),
    }


def block_members(golden_dir):
    """members around the block size the encoders write (2^20): the reference cannot transform them, host twin and device are held
    against each other and against the round trip"""
    rng = np.random.default_rng(20262)
    text = text_member(golden_dir, 4096)
    big = np.frombuffer((text * (3 * BLK // len(text) + 1))[:2 * BLK + 300001], dtype=np.uint8).copy()
    big[::997] = rng.integers(0, 256, size=big[::997].size, dtype=np.uint8)
    return {
        "exactly_one_block": big[:BLK].tobytes(),
        "one_block_plus_1": big[:BLK + 1].tobytes(),                      # (the last block is 1 byte)
        "three_blocks_last_short": big.tobytes(),
        "all_equal_block_and_a_bit": b"\x00" * (BLK + 4097),
    }


def compression_member() -> bytes:
    """64 repeats of 1000 uniform random bytes, fixed seed: order-1 sees about 4 successors per context (about 2 bits per byte); after
    block sorting nearly every rank is 0"""
    return np.random.default_rng(64000).integers(0, 256, size=1000, dtype=np.uint8).tobytes() * 64


_REF = {}


def ref_member(raw: bytes, blk_log2: int, anc_log2: int, kind=None) -> bytes:
    """bwt_reference.ref_encode, kept: several tests want the same members"""
    key = (raw, blk_log2, anc_log2, kind)
    if key not in _REF:
        _REF[key] = br.ref_encode(raw, blk_log2, anc_log2, kind)
    return _REF[key]


def decoder_cases(golden_dir):
    """(label, raw, member): every small member block sorted (kind forced, so that members plain rANS would win are transformed too) at
    every geometry, and as the format's own choice at the first one"""
    for name, raw in small_members(golden_dir).items():
        for blk_log2, anc_log2 in GEOMETRIES:
            if raw:
                yield "%s/bwt/%d/%d" % (name, blk_log2, anc_log2), raw, ref_member(raw, blk_log2, anc_log2, br.BWT)
        yield "%s/choice/8/4" % name, raw, ref_member(raw, 8, 4)


# ---- one crafted member per refusal rule ------------------------------------------------------------------------------------------------
def split(member: bytes):
    h = br.parse_header(member)
    at = br.HEADER + h["index_bytes"]
    index = [int.from_bytes(member[br.HEADER + 4 * k:br.HEADER + 4 * k + 4], "little") for k in range(h["index_bytes"] // 4)]
    return h, index, member[at:]


def join(h, index, emb: bytes, **over) -> bytes:
    """the parts back into a member whose header describes it to the byte (index_bytes and member_bytes recomputed)"""
    f = dict(h, index_bytes=4 * len(index), member_bytes=len(emb))
    f.update(over)
    return (br.ref_header(f["kind"], f["blk_log2"], f["anc_log2"], f["raw_len"], f["crc"], f["index_bytes"], f["member_bytes"])
            + b"".join(r.to_bytes(4, "little") for r in index) + emb)


_CRAFTED = None


def crafted_refusals(golden_dir):
    """(raw, good member, {label: member}): made from the reference's block-sorted member of 600 text bytes at blocks of 2^8 and anchors
    every 2^4 bytes (3 blocks of 16, 16 and 6 index rows), each so that the named rule is the first thing wrong with it"""
    global _CRAFTED
    if _CRAFTED is not None:
        return _CRAFTED
    raw = text_member(golden_dir, 600)
    good = ref_member(raw, 8, 4, br.BWT)
    h, index, emb = split(good)
    assert h["blocks"] == [256, 256, 88] and len(index) == 38 and join(h, index, emb) == good
    out = {}
    out["bad_magic"] = b"MCBX" + good[4:]
    out["version_2"] = good[:4] + b"\x02" + good[5:]
    out["kind_2"] = good[:5] + b"\x02" + good[6:]
    out["blk_log2_7"] = join(h, index, emb, blk_log2=7)
    out["blk_log2_24"] = join(h, index, emb, blk_log2=24)
    out["anc_log2_3"] = join(h, index, emb, anc_log2=3)
    out["anc_log2_24"] = join(h, index, emb, anc_log2=24)
    out["byte_appended"] = good + b"\x00"
    out["last_byte_cut"] = good[:-1]
    out["index_one_row_short"] = join(h, index[:-1], emb)
    out["raw_len_plus_1"] = join(h, index, emb, raw_len=h["raw_len"] + 1)
    ix = list(index); ix[0] = 257
    out["primary_index_beyond_block"] = join(h, ix, emb)
    ix = list(index); ix[16] = 0
    out["primary_index_0"] = join(h, ix, emb)
    ix = list(index); ix[32 + 3] = 89
    out["anchor_beyond_last_block"] = join(h, ix, emb)
    ix = list(index); ix[5], ix[6] = ix[6], ix[5]
    out["anchors_do_not_chain"] = join(h, ix, emb)
    ix = list(index); ix[16 + 7] = ix[16]
    out["anchor_is_the_primary_row"] = join(h, ix, emb)
    e = bytearray(emb); e[-3] ^= 0x10
    out["embedded_member_corrupted"] = join(h, index, bytes(e))
    e = bytearray(emb); e[8] ^= 1                                              # its raw_len
    out["embedded_member_other_length"] = join(h, index, bytes(e))
    out["wrong_raw_crc"] = join(h, index, emb, crc=h["crc"] ^ 1)
    plain = ref_member(raw, 8, 4, br.PLAIN)
    ph, _, pemb = split(plain)
    out["plain_wrong_raw_crc"] = join(ph, [], pemb, crc=ph["crc"] ^ 1)
    out["plain_with_an_index"] = join(ph, [1], pemb)
    _CRAFTED = (raw, good, out)
    return _CRAFTED
