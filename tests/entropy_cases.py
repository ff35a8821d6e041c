"""Inputs shared by tests/test_entropy.py (host twin) and tests/test_gpu_entropy.py (device): the golden stream files as members, the
synthetic members, the hostile corpus, and a numpy reader of the `.rans` format that recomputes what a member's
own tables say its bytes cost."""
import glob
import gzip
import io
import math
import os
import tarfile

import numpy as np

SEG = 2048                     # what the encoders write (rans_model.hpp SEG)
HEADER = 32
RUN_OVERHEAD = 8               # bytes per segment run beyond its share of the model's bits (4 state + 2 length + rounding)
MODELS = ((0, 1), (1, 1), (1, 2), (1, 4), (2, 1), (2, 2), (2, 4))      # (model, stride), simpler first


def golden_members(golden_dir):
    """every stream file of every stream fixture: {"fixture/name": bytes}"""
    out = {}
    for p in sorted(glob.glob(os.path.join(golden_dir, "streams_*.tar.gz"))):
        tag = os.path.basename(p)[len("streams_"):-len(".tar.gz")]
        with gzip.open(p, "rb") as g:
            tf = tarfile.open(fileobj=io.BytesIO(g.read()))
            for m in tf.getmembers():
                if m.isfile():
                    out[tag + "/" + os.path.basename(m.name)] = tf.extractfile(m).read()
    return out


def synthetic_members():
    rng = np.random.default_rng(20260)
    skew = rng.choice(np.array([65, 67, 71, 84], dtype=np.uint8), size=50000, p=[0.7, 0.2, 0.07, 0.03])
    words = (rng.integers(0, 300, size=6000).astype("<u4") * 7).view(np.uint8)       # 32-bit little-endian words: stride 4 pays
    return {
        "empty": b"",
        "one_byte": b"\x5a",
        "all_equal": b"\x07" * 10000,
        "uniform_random": rng.integers(0, 256, size=20000, dtype=np.uint8).tobytes(),
        "skewed_4_symbols": skew.tobytes(),
        "segment_minus_1": skew[:SEG - 1].tobytes(),
        "segment_plus_1": skew[:SEG + 1].tobytes(),
        "three_segments_minus_1": rng.integers(0, 7, size=3 * SEG - 1, dtype=np.uint8).tobytes(),
        "words_u32": words.tobytes(),
    }


def hostile_corpus(member: bytes, flips: int, seed: int = 7, truncations=None):
    """(label, bytes): every truncation length (or the listed ones) and `flips` seeded single-bit flips"""
    for cut in (range(len(member)) if truncations is None else truncations):
        yield "cut@%d" % cut, member[:cut]
    rng = np.random.default_rng(seed)
    for bit in rng.integers(0, 8 * len(member), size=flips):
        b = bytearray(member)
        b[int(bit) >> 3] ^= 1 << (int(bit) & 7)
        yield "flip@%d" % int(bit), bytes(b)


def pick_hostile_member(golden_dir):
    """a golden stream file of at least 4 KB that the coder does not store: the largest dif_char.txt of the fixtures (ref.bin, 2-bit
    packed bases of a random genome, is the larger file, but it is stored and would exercise only the header checks and the CRC)"""
    m = golden_members(golden_dir)
    name = max((k for k in m if "dif_char.txt" in k), key=lambda k: len(m[k]))
    assert len(m[name]) >= 4096, (name, len(m[name]))
    return name, m[name]


def parse_member(member: bytes):
    """header fields and, for the rANS models, freq[plane, context, symbol] from the member's own tables"""
    assert member[:4] == b"MCRS" and member[4] == 1
    h = {"model": member[5], "stride": member[6], "seg_log2": member[7], "raw_len": int.from_bytes(member[8:16], "little"),
         "crc": int.from_bytes(member[16:20], "little"), "table_bytes": int.from_bytes(member[20:24], "little"),
         "payload_bytes": int.from_bytes(member[24:32], "little")}
    h["n_seg"] = -(-h["raw_len"] // (1 << h["seg_log2"]))
    if h["model"] == 0:
        return h, None
    n_ctx = 256 if h["model"] == 2 else 1
    freq = np.zeros((h["stride"], n_ctx, 256), dtype=np.int64)
    at = HEADER
    for pl in range(h["stride"]):
        for c in range(n_ctx):
            nsym = int.from_bytes(member[at:at + 2], "little"); at += 2
            for _ in range(nsym):
                freq[pl, c, member[at]] = int.from_bytes(member[at + 1:at + 3], "little"); at += 3
            assert nsym == 0 or freq[pl, c].sum() == 4096
    assert at == HEADER + h["table_bytes"]
    assert len(member) == HEADER + h["table_bytes"] + 2 * h["n_seg"] + h["payload_bytes"]
    return h, freq


def model_bits(raw: bytes, h, freq) -> float:
    """B = sum over the raw bytes of -log2(f / 4096) under the member's tables"""
    d = np.frombuffer(raw, dtype=np.uint8).astype(np.int64)
    if d.size == 0:
        return 0.0
    s = h["stride"]
    i = np.arange(d.size)
    ctx = np.zeros(d.size, dtype=np.int64)
    if h["model"] == 2:
        ctx[s:] = d[:-s]
        ctx[(i % (1 << h["seg_log2"])) < s] = 0
    f = freq[i % s, ctx, d]
    assert (f > 0).all()
    return float(-np.log2(f / 4096.0).sum())


def numpy_estimate(raw: bytes, h, freq) -> int:
    n_seg = -(-len(raw) // SEG)
    if h["model"] == 0:
        return HEADER + len(raw)
    return HEADER + h["table_bytes"] + math.ceil(model_bits(raw, h, freq) / 8.0) + RUN_OVERHEAD * n_seg


def big_member(golden_dir, size: int) -> np.ndarray:
    """~size bytes: a fixture's ref.bin and dif_char.txt tiled, with a seeded perturbation (one byte in 97 replaced)"""
    m = golden_members(golden_dir)
    unit = np.frombuffer(m["stages_L150/ref.bin.0"] + m["stages_L150/dif_char.txt.0"], dtype=np.uint8)
    out = np.tile(unit, size // unit.size + 1)[:size].copy()
    rng = np.random.default_rng(11)
    at = np.arange(0, size, 97)
    out[at] = rng.integers(0, 256, size=at.size, dtype=np.uint8)
    return out


# ---- members made with the independent reference (tests/rans_reference.py) --------------------------------------------------------------
CODED_MODELS = MODELS[1:]


def split_member(member: bytes):
    """a coded member -> (header dict, serialised tables, list of runs)"""
    import rans_reference as rr
    h = rr.parse_header(member)
    at = HEADER + h["table_bytes"]
    lens = [int.from_bytes(member[at + 2 * s:at + 2 * s + 2], "little") for s in range(h["n_seg"])]
    at += 2 * h["n_seg"]
    runs = []
    for l in lens:
        runs.append(member[at:at + l]); at += l
    assert at == len(member)
    return h, member[HEADER:HEADER + h["table_bytes"]], runs


def join_member(h, tables: bytes, runs, lens=None, **over) -> bytes:
    """the parts back into a member whose header describes it to the byte (table_bytes and payload_bytes recomputed); lens: the stored
    run lengths when they are to differ from the runs'; over: header fields to overwrite"""
    import rans_reference as rr
    f = dict(h, table_bytes=len(tables), payload_bytes=sum(len(r) for r in runs))
    f.update(over)
    lens = [len(r) for r in runs] if lens is None else lens
    return (rr.ref_header(f["model"], f["stride"], f["seg_log2"], f["raw_len"], f["crc"], f["table_bytes"], f["payload_bytes"])
            + tables + b"".join(l.to_bytes(2, "little") for l in lens) + b"".join(runs))


_CRAFTED = None


def crafted_refusals():
    """(raw, good member, {label: member}): one member per refusal rule of DESIGN 3.6, each made from the reference's order-1 stride-1
    member of three segments so that the named rule is the first thing wrong with it.  Everything but the "header" cases passes the
    header check: the sizes are recomputed."""
    global _CRAFTED
    if _CRAFTED is not None:
        return _CRAFTED
    import rans_reference as rr
    raw = synthetic_members()["three_segments_minus_1"]
    good = rr.ref_encode(raw, 2, 1)
    h, tables, runs = split_member(good)
    assert h["n_seg"] == 3 and join_member(h, tables, runs) == good
    state = lambda v: [runs[0], v.to_bytes(4, "little") + runs[1][4:], runs[2]]
    out = {}
    # run lengths: the runs as they are, the boundary between the first two moved by one byte
    out["length_moved_to_neighbour"] = join_member(h, tables, runs, lens=[len(runs[0]) - 1, len(runs[1]) + 1, len(runs[2])])
    out["run_of_length_3"] = join_member(h, tables, [runs[0], runs[1][:3], runs[2]])
    out["state_2^23-1"] = join_member(h, tables, state((1 << 23) - 1))
    out["state_2^31"] = join_member(h, tables, state(1 << 31))
    out["byte_appended_to_run"] = join_member(h, tables, [runs[0], runs[1] + b"\x00", runs[2]])
    # tables: rows are n u16, n x (symbol u8, freq u16); the row of context c
    rows, at = [], 0
    for c in range(256):
        n = int.from_bytes(tables[at:at + 2], "little")
        rows.append(tables[at:at + 2 + 3 * n]); at += 2 + 3 * n
    assert at == len(tables) and all(len(rows[c]) > 2 for c in range(1, 7))        # the contexts 1 .. 6 occur in every segment
    emptied = list(rows); emptied[3] = b"\x00\x00"
    out["table_row_emptied"] = join_member(h, b"".join(emptied), runs)
    r = bytearray(rows[3])
    k = next(k for k in range(2, len(r), 3) if int.from_bytes(r[k + 1:k + 3], "little") >= 2)
    r[k + 1:k + 3] = (int.from_bytes(r[k + 1:k + 3], "little") - 1).to_bytes(2, "little")
    short = list(rows); short[3] = bytes(r)
    out["table_row_sums_to_4095"] = join_member(h, b"".join(short), runs)
    out["header_seg_log2_7"] = join_member(h, tables, runs, seg_log2=7)
    out["header_seg_log2_16"] = join_member(h, tables, runs, seg_log2=16)
    # ... and with one segment at any segment size, so that the segment size alone is out of range
    tiny = rr.ref_encode(raw[:100], 2, 1, seg_log2=8)
    out["header_seg_log2_7_one_segment"] = tiny[:7] + b"\x07" + tiny[8:]
    out["header_seg_log2_16_one_segment"] = tiny[:7] + b"\x10" + tiny[8:]
    out["wrong_crc"] = join_member(h, tables, runs, crc=h["crc"] ^ 1)
    _CRAFTED = (raw, good, out)
    return _CRAFTED


def worst_case_raw() -> bytes:
    """100 segments of zeros, one segment that holds only the 255 other symbols, 3 segments of zeros: under order-0 stride 1 every symbol
    of that segment has frequency 1 (12 bits each), the longest run a segment of 2048 bytes can get"""
    z = np.zeros(SEG, dtype=np.uint8)
    rare = ((np.arange(SEG) % 255) + 1).astype(np.uint8)
    return np.concatenate([np.tile(z, 100), rare, np.tile(z, 3)]).tobytes()


def exact_segment(seg_log2: int) -> bytes:
    """exactly one segment of 2^seg_log2 bytes drawn from 7 symbols"""
    return np.random.default_rng(4400 + seg_log2).integers(0, 7, size=1 << seg_log2, dtype=np.uint8).tobytes()


def all_frequency_1_member(seg_log2: int = 15):
    """(raw, member): one segment of 2^seg_log2 bytes, every one a symbol of frequency 1 under the order-0 table the member carries
    (symbol 0, which does not occur, holds the rest): 12 bits per symbol, a run of 1.5 * 2^seg_log2 + 4 bytes"""
    import rans_reference as rr
    raw = ((np.arange(1 << seg_log2) % 255) + 1).astype(np.uint8).tobytes()
    freq = np.ones((1, 1, 256), dtype=np.int64)
    freq[0, 0, 0] = 4096 - 255
    return raw, rr.ref_encode(raw, 1, 1, seg_log2=seg_log2, freq=freq)


def words_bytes(n: int, seed: int = 31) -> bytes:
    """n bytes of 32-bit little-endian words like words_u32: the four byte positions have four different distributions"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 300, size=n // 4 + 1).astype("<u4") * 7).view(np.uint8)[:n].tobytes()


_REF_MEMBERS = {}


def ref_member(raw: bytes, model: int, stride: int, seg_log2: int = 11) -> bytes:
    """rans_reference.ref_encode, kept: the Python coder takes about a second per megabyte and several tests want the same members"""
    import rans_reference as rr
    key = (raw, model, stride, seg_log2)
    if key not in _REF_MEMBERS:
        _REF_MEMBERS[key] = rr.ref_encode(raw, model, stride, seg_log2=seg_log2)
    return _REF_MEMBERS[key]
