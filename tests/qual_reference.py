"""An independent statement of the `.mcq` member format, written from DESIGN.md section 3.9 alone: plain Python and numpy, zlib.crc32
for the checksum.  It shares no code with csrc/qual_model.hpp, csrc/rans_model.hpp, csrc/qual.hip or host/mcom_qual.cpp, so that a
mistake those have in common shows up as a difference.  Slow on purpose (a Python loop per symbol, about a second per megabyte):
tests keep what they code with it at or below 1 MB.  The embedded `.rans` member of kind 1 is section 3.6's: this file takes it from
the caller (ref_encode(..., rans_member=)) and hands it back (ref_decode(..., rans_decode=)) instead of stating that format again."""
import math
import zlib

import numpy as np

HEADER = 64
M = 4096
STATE_L = 1 << 23
STATE_H = 1 << 31
STORED, ORDER0, P, PP, PMP = 0, 1, 2, 3, 4
KIND_MODEL, KIND_RANS = 0, 1


class QualRefused(ValueError):
    """ref_decode: the member is one that section 3.9 says is refused; .rule names the first rule it breaks"""
    def __init__(self, rule, detail=""):
        super().__init__(rule + (": " + detail if detail else ""))
        self.rule = rule


def default_rps(L: int) -> int:
    return max(1, 2048 // L)


def n_ctx(model: int, A: int) -> int:
    Q = min(A, 8)
    return {ORDER0: 1, P: A, PP: 8 * A, PMP: 8 * A * Q}[model]


# ---- alphabet, contexts, tables -------------------------------------------------------------------------------------------------------
def ref_alphabet(q):
    """(the 32-byte map, the byte values that occur in ascending order)"""
    vals = np.unique(np.asarray(q, dtype=np.uint8)).tolist()
    m = bytearray(32)
    for v in vals:
        m[v >> 3] |= 1 << (v & 7)
    return bytes(m), vals


def map_values(m: bytes):
    return [v for v in range(256) if (m[v >> 3] >> (v & 7)) & 1]


def ref_symbols_contexts(q, vals, model):
    """dense symbols [n, L] and the context index of every cell under `model` (int64)"""
    q = np.asarray(q, dtype=np.uint8)
    n, L = q.shape
    A = len(vals); Q = min(A, 8)
    rank = np.zeros(256, dtype=np.int64); rank[np.array(vals, dtype=np.int64)] = np.arange(A)
    s = rank[q]
    prev = lambda k: np.concatenate([np.zeros((n, min(k, L)), np.int64), s[:, :max(L - k, 0)]], axis=1)
    p1, p2, p3 = prev(1), prev(2), prev(3)
    pos = (8 * np.arange(L, dtype=np.int64) // L)[None, :] + np.zeros((n, 1), np.int64)
    mb = Q * np.maximum(p2, p3) // A
    if model == ORDER0:
        c = np.zeros((n, L), np.int64)
    elif model == P:
        c = p1
    elif model == PP:
        c = p1 * 8 + pos
    else:
        c = (p1 * Q + mb) * 8 + pos
    return s, c


def ref_hist(q, vals=None):
    """the counts of model 4, int64 [A, Q, 8, A]: [s[j-1]][floor(Q max(s[j-2], s[j-3]) / A)][floor(8 j / L)][symbol]"""
    if vals is None:
        vals = ref_alphabet(q)[1]
    A = len(vals); Q = min(A, 8)
    s, c = ref_symbols_contexts(q, vals, PMP)
    return np.bincount((c * A + s).ravel(), minlength=A * Q * 8 * A).reshape(A, Q, 8, A)


def counts_of(h4, model):
    """[context, symbol] counts of `model` as sums of model 4's"""
    A, Q = h4.shape[0], h4.shape[1]
    if model == PMP:
        return h4.reshape(A * Q * 8, A)
    if model == PP:
        return h4.sum(axis=1).reshape(A * 8, A)
    if model == P:
        return h4.sum(axis=(1, 2))
    return h4.sum(axis=(0, 1, 2)).reshape(1, A)


def ref_normalise(counts):
    """counts of one context -> frequencies that add up to 4096 (all 0 when nothing was counted): floor of the share, at least 1 for a
    symbol that occurs; a shortfall goes to the most frequent symbol (the lowest among equals); an excess is taken one at a time from
    the symbol whose frequency is then the largest (the lowest among equals)"""
    cnt = [int(c) for c in counts]
    tot = sum(cnt)
    if tot == 0:
        return [0] * len(cnt)
    f = [max(1, c * M // tot) if c else 0 for c in cnt]
    s = sum(f)
    if s < M:
        f[cnt.index(max(cnt))] += M - s
    while s > M:
        f[f.index(max(f))] -= 1
        s -= 1
    return f


def ref_tables(h4, model):
    """(freq as a list of rows, the bits the model spends: sum count * log2(4096 / freq) in context then symbol order)"""
    cnt = counts_of(h4, model)
    freq, bits = [], 0.0
    for c in range(cnt.shape[0]):
        row = ref_normalise(cnt[c])
        freq.append(row)
        for s, f in enumerate(row):
            if f:
                bits += float(int(cnt[c, s])) * math.log2(M / f)
    return freq, bits


def _serialise(freq) -> bytes:
    out = bytearray()
    for row in freq:
        syms = [s for s, f in enumerate(row) if f]
        out += len(syms).to_bytes(2, "little")
        for s in syms:
            out += bytes([s]) + row[s].to_bytes(2, "little")
    return bytes(out)


def _starts(freq):
    out = []
    for row in freq:
        c, acc = [], 0
        for f in row:
            c.append(acc); acc += f
        out.append(c)
    return out


def ref_estimates(q, rows_per_seg=None):
    """the estimated member size by model id (what the choice compares)"""
    q = np.asarray(q, dtype=np.uint8)
    n, L = q.shape
    est = [HEADER + n * L, 0, 0, 0, 0]
    if n == 0:
        return est
    rps = rows_per_seg or default_rps(L)
    n_seg = -(-n // rps)
    h4 = ref_hist(q)
    for model in (ORDER0, P, PP, PMP):
        freq, bits = ref_tables(h4, model)
        est[model] = HEADER + len(_serialise(freq)) + math.ceil(bits / 8.0) + 8 * n_seg
    return est


def ref_choose(q, rows_per_seg=None) -> int:
    est = ref_estimates(q, rows_per_seg)
    if np.asarray(q).shape[0] == 0:
        return STORED
    best = STORED
    for model in (ORDER0, P, PP, PMP):
        if est[model] < est[best]:
            best = model
    return best


# ---- the coder -----------------------------------------------------------------------------------------------------------------------
def ref_header(kind, model, payload_bytes, crc, n_rows, L, rps, table_bytes, amap) -> bytes:
    return (b"MCQV" + bytes([1, kind, model]) + payload_bytes.to_bytes(5, "little") + crc.to_bytes(4, "little") + n_rows.to_bytes(8, "little")
            + L.to_bytes(2, "little") + rps.to_bytes(2, "little") + table_bytes.to_bytes(4, "little") + bytes(amap))


def _encode_run(syms, ctxs, F, Cm) -> bytes:
    x = STATE_L
    emitted = bytearray()
    for i in range(len(syms) - 1, -1, -1):
        f = F[ctxs[i]][syms[i]]
        if f == 0:
            raise ValueError("symbol %d has no frequency in context %d" % (syms[i], ctxs[i]))
        c = Cm[ctxs[i]][syms[i]]
        x_max = f << 19
        while x >= x_max:
            emitted.append(x & 0xFF)
            x >>= 8
        x = ((x // f) << 12) + (x % f) + c
    emitted.reverse()
    return x.to_bytes(4, "little") + bytes(emitted)


def ref_encode(q, model=None, rows_per_seg=None, rans_member=None, freq=None) -> bytes:
    """the matrix -> the member.  model None: the choice of section 3.9 among the ids, then kind 1 around `rans_member` (the `.rans`
    member of the flat bytes, made by the caller) when 64 + its length is smaller; model 0 .. 4: that id, kind 0; model "rans": kind 1.
    freq: rows to use instead of the counted ones (any valid rows that give every (context, symbol) of the matrix a frequency)."""
    q = np.ascontiguousarray(q, dtype=np.uint8)
    n, L = q.shape
    rps = rows_per_seg or default_rps(L)
    raw = q.tobytes()
    crc = zlib.crc32(raw) if raw else 0
    wrap = lambda: ref_header(KIND_RANS, 0, len(rans_member), crc, n, L, rps, 0, bytes(32)) + bytes(rans_member)
    if model == "rans":
        return wrap()
    auto = model is None
    if auto:
        model = ref_choose(q, rps)
    amap, vals = ref_alphabet(q)
    if n == 0 or model == STORED:
        member = ref_header(KIND_MODEL, STORED, len(raw), crc, n, L, rps, 0, amap) + raw
    else:
        if freq is None:
            freq, _ = ref_tables(ref_hist(q, vals), model)
        tables = _serialise(freq)
        Cm = _starts(freq)
        s, c = ref_symbols_contexts(q, vals, model)
        runs = [_encode_run(s[a:a + rps].ravel().tolist(), c[a:a + rps].ravel().tolist(), freq, Cm) for a in range(0, n, rps)]
        assert all(len(r) < 1 << 16 for r in runs)
        lens = b"".join(len(r).to_bytes(2, "little") for r in runs)
        payload = b"".join(runs)
        member = ref_header(KIND_MODEL, model, len(payload), crc, n, L, rps, len(tables), amap) + tables + lens + payload
    if auto and rans_member is not None and HEADER + len(rans_member) < len(member):
        return wrap()
    return member


def parse_header(member: bytes):
    bad = lambda why: QualRefused("header", why)
    if len(member) < HEADER or member[:4] != b"MCQV" or member[4] != 1:
        raise bad("magic / version / shorter than a header")
    h = {"kind": member[5], "model": member[6], "payload_bytes": int.from_bytes(member[7:12], "little"), "crc": int.from_bytes(member[12:16], "little"),
         "n_rows": int.from_bytes(member[16:24], "little"), "L": int.from_bytes(member[24:26], "little"), "rps": int.from_bytes(member[26:28], "little"),
         "table_bytes": int.from_bytes(member[28:32], "little"), "map": member[32:64]}
    if h["kind"] > 1 or h["model"] > 4:
        raise bad("kind / model")
    if not 1 <= h["L"] <= 256 or not 1 <= h["rps"] <= 4096 or h["rps"] * h["L"] > 32768:
        raise bad("L / rows_per_seg")
    if h["n_rows"] >= 1 << 32 or h["n_rows"] * h["L"] > 1 << 34:
        raise bad("n_rows")
    rest, raw = len(member) - HEADER, h["n_rows"] * h["L"]
    h["n_seg"] = -(-h["n_rows"] // h["rps"])
    if h["kind"] == KIND_RANS:
        if h["model"] != 0 or h["table_bytes"] != 0 or h["payload_bytes"] != rest or any(h["map"]):
            raise bad("kind 1 fields")
        e = member[HEADER:]
        if len(e) < 32 or int.from_bytes(e[8:16], "little") != raw or int.from_bytes(e[16:20], "little") != h["crc"]:
            raise QualRefused("embedded", "length or CRC of the embedded member")
    elif h["model"] == STORED:
        if not (h["table_bytes"] == 0 and h["payload_bytes"] == raw == rest):
            raise bad("stored sizes")
    else:
        if h["n_rows"] == 0 or not any(h["map"]):
            raise bad("a coded member without rows or without an alphabet")
        if rest != h["table_bytes"] + 2 * h["n_seg"] + h["payload_bytes"]:
            raise bad("length != 64 + tables + 2 n_seg + payload")
        if h["payload_bytes"] < 4 * h["n_seg"]:
            raise bad("fewer than 4 bytes per run")
    return h


def parse_tables(ser: bytes, model: int, A: int):
    freq, at = [], 0
    for _ in range(n_ctx(model, A)):
        if len(ser) - at < 2:
            raise QualRefused("tables", "cut short")
        n = int.from_bytes(ser[at:at + 2], "little"); at += 2
        if n > A or len(ser) - at < 3 * n:
            raise QualRefused("tables", "row length")
        row, last = [0] * A, -1
        for _ in range(n):
            s, f = ser[at], int.from_bytes(ser[at + 1:at + 3], "little"); at += 3
            if s <= last or s >= A or not 1 <= f <= M:
                raise QualRefused("tables", "symbols not ascending, a symbol >= A or a frequency outside 1 .. 4096")
            row[s] = f; last = s
        if n and sum(row) != M:
            raise QualRefused("tables", "a row's sum is not 4096")
        freq.append(row)
    if at != len(ser):
        raise QualRefused("tables", "bytes left over")
    return freq


def ref_decode(member, rans_decode=None):
    """the member -> the uint8 matrix [n_rows, L]; QualRefused for everything section 3.9 refuses.  rans_decode: the decoder of the
    embedded member of kind 1 (bytes -> bytes, raising for what section 3.6 refuses)."""
    member = bytes(member)
    h = parse_header(member)
    n, L = h["n_rows"], h["L"]
    if h["kind"] == KIND_RANS:
        try:
            raw = rans_decode(member[HEADER:])
        except Exception as e:                                 # noqa: BLE001
            raise QualRefused("embedded", str(e))
    elif h["model"] == STORED:
        raw = member[HEADER:]
    else:
        vals = map_values(h["map"])
        A = len(vals); Q = min(A, 8)
        model, rps, n_seg = h["model"], h["rps"], h["n_seg"]
        at = HEADER + h["table_bytes"]
        freq = parse_tables(member[HEADER:at], model, A)
        lens = [int.from_bytes(member[at + 2 * s:at + 2 * s + 2], "little") for s in range(n_seg)]
        if sum(lens) != h["payload_bytes"]:
            raise QualRefused("lengths", "the run lengths do not add up to the payload")
        at += 2 * n_seg
        Cm = _starts(freq)
        slot_tabs = {}
        out = bytearray()
        for seg in range(n_seg):
            run = member[at:at + lens[seg]]; at += lens[seg]
            if len(run) < 4:
                raise QualRefused("run<4", "segment %d" % seg)
            x = int.from_bytes(run[:4], "little"); p = 4
            if not STATE_L <= x < STATE_H:
                raise QualRefused("state", "segment %d starts with %#x" % (seg, x))
            for _ in range(min(rps, n - seg * rps)):
                p1 = p2 = p3 = 0
                for j in range(L):
                    pos = 8 * j // L
                    ctx = 0 if model == ORDER0 else p1 if model == P else p1 * 8 + pos if model == PP else (p1 * Q + Q * max(p2, p3) // A) * 8 + pos
                    tab = slot_tabs.get(ctx)
                    if tab is None:
                        tab = slot_tabs[ctx] = _slot_table(freq[ctx], Cm[ctx])
                    if tab is False:
                        raise QualRefused("slot", "segment %d: context %d is empty" % (seg, ctx))
                    slot = x & (M - 1)
                    s = tab[slot]
                    x = freq[ctx][s] * (x >> 12) + slot - Cm[ctx][s]
                    while x < STATE_L:
                        if p >= len(run):
                            raise QualRefused("exhausted", "segment %d" % seg)
                        x = (x << 8) | run[p]; p += 1
                    out.append(vals[s])
                    p3, p2, p1 = p2, p1, s
            if p != len(run) or x != STATE_L:
                raise QualRefused("end", "segment %d: %d of %d bytes taken, state %#x" % (seg, p, len(run), x))
        raw = bytes(out)
    if len(raw) != n * L:
        raise QualRefused("embedded", "length")
    if (zlib.crc32(raw) if raw else 0) != h["crc"]:
        raise QualRefused("crc")
    return np.frombuffer(raw, dtype=np.uint8).reshape(n, L)


def _slot_table(f_row, c_row):
    if not any(f_row):
        return False
    t = [0] * M
    for s, f in enumerate(f_row):
        if f:
            t[c_row[s]:c_row[s] + f] = [s] * f
    return t
