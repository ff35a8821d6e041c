"""An independent statement of the `.rans` member format, written from DESIGN.md section 3.6 alone: plain Python and numpy, zlib.crc32
for the checksum.  It shares no code with csrc/rans_model.hpp, csrc/entropy.hip or host/mcom_entropy.cpp, so that a mistake those three
have in common shows up as a difference.  Slow on purpose (about a microsecond-scale Python loop per symbol): tests keep what they code
with it near or below 2 MB."""
import zlib

import numpy as np

HEADER = 32
PROB_BITS = 12
M = 1 << PROB_BITS             # the frequencies of a row add up to this
STATE_L = 1 << 23              # the coder starts here; the state lives in [2^23, 2^31)
STATE_H = 1 << 31
SEG_LOG2 = 11                  # what the encoders write
STORED, ORDER0, ORDER1 = 0, 1, 2
PLANE_BASE = {1: 0, 2: 1, 4: 3}            # the order-1 planes of stride 1 | 2 | 4 side by side: 0 | 1 2 | 3 4 5 6


class RansRefused(ValueError):
    """ref_decode: the member is one that section 3.6 says is refused; .rule names the first rule it breaks"""
    def __init__(self, rule, detail=""):
        super().__init__(rule + (": " + detail if detail else ""))
        self.rule = rule


def run_cap(seg_bytes: int) -> int:
    """the room an encoder gives a run: 12 bits per symbol at most, + the state, + slack"""
    return seg_bytes * 3 // 2 + 8


# ---- histograms and tables ----------------------------------------------------------------------------------------------------------
def ref_hist(raw, seg_log2: int = SEG_LOG2):
    """o0[i mod 4, symbol] and o1[plane, context, symbol] (int64) of the planes 0 | 1 2 | 3 4 5 6: plane base(stride) + i mod stride, the
    context is byte i - stride, 0 for the first `stride` bytes of each segment"""
    d = np.frombuffer(bytes(raw), dtype=np.uint8).astype(np.int64) if not isinstance(raw, np.ndarray) else raw.astype(np.int64)
    i = np.arange(d.size, dtype=np.int64)
    at = i & ((1 << seg_log2) - 1)
    o0 = np.bincount((i & 3) * 256 + d, minlength=4 * 256).reshape(4, 256)
    o1 = np.zeros(7 * 65536, dtype=np.int64)
    for stride in (1, 2, 4):
        ctx = np.zeros(d.size, dtype=np.int64)
        ctx[stride:] = d[:-stride] if d.size > stride else 0
        ctx[at < stride] = 0
        plane = PLANE_BASE[stride] + (i & (stride - 1))
        o1 += np.bincount((plane * 256 + ctx) * 256 + d, minlength=7 * 65536)
    return o0, o1.reshape(7, 256, 256)


def ref_normalise(counts):
    """256 counts -> 256 frequencies that add up to 4096 (all 0 when nothing was counted): floor of the share, at least 1 for a symbol
    that occurs; a shortfall goes to the most frequent symbol (the lowest value among equals); an excess is taken one at a time from
    the symbol whose frequency is then the largest (the lowest value among equals)"""
    cnt = [int(c) for c in counts]
    tot = sum(cnt)
    if tot == 0:
        return [0] * 256
    f = [max(1, c * M // tot) if c else 0 for c in cnt]
    s = sum(f)
    if s < M:
        f[cnt.index(max(cnt))] += M - s
    while s > M:
        f[f.index(max(f))] -= 1
        s -= 1
    return f


def ref_tables(raw, model: int, stride: int, seg_log2: int = SEG_LOG2):
    """freq[plane, context, symbol] (int64; one context for order-0) of the bytes `raw` under (model, stride)"""
    o0, o1 = ref_hist(raw, seg_log2)
    n_ctx = 256 if model == ORDER1 else 1
    freq = np.zeros((stride, n_ctx, 256), dtype=np.int64)
    for pl in range(stride):
        if model == ORDER1:
            for c in range(256):
                row = o1[PLANE_BASE[stride] + pl, c]
                if row.any():
                    freq[pl, c] = ref_normalise(row)
        else:
            freq[pl, 0] = ref_normalise(o0[pl::stride].sum(axis=0))       # plane i mod stride gathers the positions i mod 4 it holds
    return freq


def _serialise(freq) -> bytes:
    out = bytearray()
    for pl in range(freq.shape[0]):
        for c in range(freq.shape[1]):
            syms = np.flatnonzero(freq[pl, c])
            out += len(syms).to_bytes(2, "little")
            for s in syms:
                out += bytes([int(s)]) + int(freq[pl, c, s]).to_bytes(2, "little")
    return bytes(out)


def _rows(freq):
    """per plane and context: (frequencies, cumulative starts) as Python lists"""
    cum = np.cumsum(freq, axis=2) - freq
    return freq.tolist(), cum.tolist()


# ---- the coder ----------------------------------------------------------------------------------------------------------------------
def _encode_run(seg, stride, o1, F, Cm) -> bytes:
    """one segment -> its run: symbols are coded last to first from the state 2^23; the bytes shifted out are read back by the decoder
    in the opposite order, so the run is the final state (u32, little endian) followed by them, last one first"""
    x = STATE_L
    emitted = bytearray()
    for i in range(len(seg) - 1, -1, -1):
        s = seg[i]
        ctx = seg[i - stride] if (o1 and i >= stride) else 0
        f = F[i % stride][ctx][s]
        if f == 0:
            raise ValueError("symbol %d has no frequency in plane %d, context %d" % (s, i % stride, ctx))
        c = Cm[i % stride][ctx][s]
        x_max = f << (23 - PROB_BITS + 8)                  # above this the step would leave [2^23, 2^31)
        while x >= x_max:
            emitted.append(x & 0xFF)
            x >>= 8
        x = ((x // f) << PROB_BITS) + (x % f) + c
    emitted.reverse()
    return x.to_bytes(4, "little") + bytes(emitted)


def ref_header(model, stride, seg_log2, raw_len, crc, table_bytes, payload_bytes) -> bytes:
    return (b"MCRS" + bytes([1, model, stride, seg_log2]) + raw_len.to_bytes(8, "little") + crc.to_bytes(4, "little")
            + table_bytes.to_bytes(4, "little") + payload_bytes.to_bytes(8, "little"))


def ref_encode(raw, model: int, stride: int, seg_log2: int = SEG_LOG2, freq=None) -> bytes:
    """raw bytes -> the member.  freq None: ref_tables of the bytes (counted with contexts cut at the given segment size); otherwise any
    valid freq[plane, context, symbol] that gives every (context, symbol) of the bytes a frequency"""
    raw = bytes(raw)
    crc = zlib.crc32(raw) if raw else 0
    if model == STORED:
        return ref_header(STORED, 1, seg_log2, len(raw), crc, 0, len(raw)) + raw
    if freq is None:
        freq = ref_tables(raw, model, stride, seg_log2)
    freq = np.asarray(freq, dtype=np.int64)
    assert freq.shape == (stride, 256 if model == ORDER1 else 1, 256)
    tables = _serialise(freq)
    F, Cm = _rows(freq)
    seg_bytes = 1 << seg_log2
    runs = [_encode_run(list(raw[a:a + seg_bytes]), stride, model == ORDER1, F, Cm) for a in range(0, len(raw), seg_bytes)]
    assert all(len(r) < 1 << 16 for r in runs)
    lens = b"".join(len(r).to_bytes(2, "little") for r in runs)
    payload = b"".join(runs)
    return ref_header(model, stride, seg_log2, len(raw), crc, len(tables), len(payload)) + tables + lens + payload


def parse_header(member: bytes):
    """the header as a dict, or RansRefused("header") when it does not describe the member to the byte"""
    bad = lambda why: RansRefused("header", why)
    if len(member) < HEADER or member[:4] != b"MCRS" or member[4] != 1:
        raise bad("magic / version / shorter than a header")
    h = {"model": member[5], "stride": member[6], "seg_log2": member[7], "raw_len": int.from_bytes(member[8:16], "little"),
         "crc": int.from_bytes(member[16:20], "little"), "table_bytes": int.from_bytes(member[20:24], "little"),
         "payload_bytes": int.from_bytes(member[24:32], "little")}
    if h["model"] > ORDER1 or h["stride"] not in (1, 2, 4):
        raise bad("model / stride")
    if not 8 <= h["seg_log2"] <= 15:
        raise bad("segment size")
    h["n_seg"] = -(-h["raw_len"] // (1 << h["seg_log2"]))
    rest = len(member) - HEADER
    if h["model"] == STORED:
        if not (h["stride"] == 1 and h["table_bytes"] == 0 and h["payload_bytes"] == h["raw_len"] == rest):
            raise bad("stored sizes")
    else:
        if rest != h["table_bytes"] + 2 * h["n_seg"] + h["payload_bytes"]:
            raise bad("length != 32 + tables + 2 n_seg + payload")
        if h["payload_bytes"] < 4 * h["n_seg"]:
            raise bad("fewer than 4 bytes per run")
    return h


def parse_tables(ser: bytes, model: int, stride: int):
    """serialised tables -> freq[plane, context, symbol], or RansRefused("tables")"""
    n_ctx = 256 if model == ORDER1 else 1
    freq = np.zeros((stride, n_ctx, 256), dtype=np.int64)
    at = 0
    for pl in range(stride):
        for c in range(n_ctx):
            if len(ser) - at < 2:
                raise RansRefused("tables", "cut short")
            n = int.from_bytes(ser[at:at + 2], "little"); at += 2
            if n > 256 or len(ser) - at < 3 * n:
                raise RansRefused("tables", "row length")
            last = -1
            for _ in range(n):
                s, f = ser[at], int.from_bytes(ser[at + 1:at + 3], "little"); at += 3
                if s <= last or not 1 <= f <= M:
                    raise RansRefused("tables", "symbols not ascending or a frequency outside 1 .. 4096")
                freq[pl, c, s] = f; last = s
            if n and int(freq[pl, c].sum()) != M:
                raise RansRefused("tables", "a row's sum is not 4096")
    if at != len(ser):
        raise RansRefused("tables", "bytes left over")
    return freq


def ref_decode(member) -> bytes:
    """the member -> its raw bytes; RansRefused for everything section 3.6 refuses"""
    member = bytes(member)
    h = parse_header(member)
    if h["model"] == STORED:
        raw = member[HEADER:]
    else:
        stride, o1, seg_bytes, n_seg = h["stride"], h["model"] == ORDER1, 1 << h["seg_log2"], h["n_seg"]
        at = HEADER + h["table_bytes"]
        freq = parse_tables(member[HEADER:at], h["model"], stride)
        lens = [int.from_bytes(member[at + 2 * s:at + 2 * s + 2], "little") for s in range(n_seg)]
        if sum(lens) != h["payload_bytes"]:
            raise RansRefused("lengths", "the run lengths do not add up to the payload")
        at += 2 * n_seg
        F, Cm = _rows(freq)
        slot_sym = {}                                      # (plane, context) -> slot table, made when the data first reaches the row
        out = bytearray()
        for seg in range(n_seg):
            run = member[at:at + lens[seg]]; at += lens[seg]
            if len(run) < 4:
                raise RansRefused("run<4", "segment %d" % seg)
            x = int.from_bytes(run[:4], "little"); p = 4
            if not STATE_L <= x < STATE_H:
                raise RansRefused("state", "segment %d starts with %#x" % (seg, x))
            n = min(seg_bytes, h["raw_len"] - seg * seg_bytes)
            d = [0] * n
            for i in range(n):
                pl = i % stride
                ctx = d[i - stride] if (o1 and i >= stride) else 0
                slot = x & (M - 1)
                table = slot_sym.get((pl, ctx))
                if table is None:
                    table = slot_sym[(pl, ctx)] = _slot_table(F[pl][ctx], Cm[pl][ctx])
                if table is False:
                    raise RansRefused("slot", "segment %d byte %d: context %d is empty" % (seg, i, ctx))
                s = table[slot]
                f, c = F[pl][ctx][s], Cm[pl][ctx][s]
                x = f * (x >> PROB_BITS) + slot - c
                while x < STATE_L:
                    if p >= len(run):
                        raise RansRefused("exhausted", "segment %d byte %d" % (seg, i))
                    x = (x << 8) | run[p]; p += 1
                d[i] = s
            if p != len(run) or x != STATE_L:
                raise RansRefused("end", "segment %d: %d of %d bytes taken, state %#x" % (seg, p, len(run), x))
            out += bytes(d)
        raw = bytes(out)
    if (zlib.crc32(raw) if raw else 0) != h["crc"]:
        raise RansRefused("crc")
    return raw


def _slot_table(f_row, c_row):
    """slot -> the symbol that owns it (a well-formed row of sum 4096 leaves no slot without an owner); False for an empty row, where
    no slot has one"""
    if not any(f_row):
        return False
    t = [0] * M
    for s in range(256):
        if f_row[s]:
            t[c_row[s]:c_row[s] + f_row[s]] = [s] * f_row[s]
    return t
