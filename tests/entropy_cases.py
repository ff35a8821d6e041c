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
