"""The lossy quality transforms of DESIGN.md section 3.13 and their report, written from that text in numpy / plain Python.  It shares
no code with csrc/qual_lossy.hpp: the spec parser is a regular expression, the maps are written out range by range, the P-block is the
plain nested loop of the text.  The host twin (tests/test_qual_lossy.py) and the kernels (tests/test_gpu_qual_lossy.py) are held
against it, bytes and report both."""
import re

import numpy as np


class LossyRefused(ValueError):
    pass


_NUM = r"(0|[1-9][0-9]{0,2})"
_SPEC = re.compile(r"\A(?:(ill8)|thr:%s:%s:%s|pblock:%s)\Z" % (_NUM, _NUM, _NUM, _NUM))


def parse(text: str):
    """("ill8",) | ("thr", T, LO, HI) | ("pblock", P); LossyRefused for anything that is not the canonical text of an accepted spec"""
    m = _SPEC.match(text)
    if not m:
        raise LossyRefused(text)
    if m.group(1):
        return ("ill8",)
    if m.group(2) is not None:
        T, LO, HI = int(m.group(2)), int(m.group(3)), int(m.group(4))
        if max(T, LO, HI) > 93 or LO >= T or HI < T:
            raise LossyRefused(text)
        return ("thr", T, LO, HI)
    P = int(m.group(5))
    if not 1 <= P <= 47:
        raise LossyRefused(text)
    return ("pblock", P)


def canonical(spec) -> str:
    return spec[0] if spec[0] == "ill8" else ":".join(str(v) for v in spec)


def ill8_lut() -> np.ndarray:
    lut = np.arange(256, dtype=np.int64)
    for lo, hi, to in ((2, 9, 6), (10, 19, 15), (20, 24, 22), (25, 29, 27), (30, 34, 33), (35, 39, 37), (40, 93, 40)):
        lut[33 + lo:33 + hi + 1] = 33 + to
    return lut.astype(np.uint8)


def thr_lut(T: int, LO: int, HI: int) -> np.ndarray:
    lut = np.arange(256, dtype=np.int64)
    phred = np.arange(0, 94)
    lut[33:127] = np.where(phred < T, LO, HI) + 33
    return lut.astype(np.uint8)


def is_idempotent(lut) -> bool:
    lut = np.asarray(lut, dtype=np.uint8)
    return bool(np.array_equal(lut[lut], lut))


def pblock_row(row, P: int) -> list:
    q = [int(v) for v in row]
    out = list(q)
    s = 0
    while s < len(q):
        lo = hi = q[s]
        j = s + 1
        while j < len(q):
            nlo, nhi = min(lo, q[j]), max(hi, q[j])
            if nhi - nlo > 2 * P:
                break
            lo, hi = nlo, nhi
            j += 1
        for i in range(s, j):
            out[i] = lo + (hi - lo) // 2
        s = j
    return out


def report(before, after) -> dict:
    d = np.abs(np.asarray(before, dtype=np.int64) - np.asarray(after, dtype=np.int64))
    return {"changed": int(np.count_nonzero(d)), "sum_abs": int(d.sum()), "sum_sq": int((d * d).sum()), "max_abs": int(d.max()) if d.size else 0}


def transform(rows, spec):
    """rows: uint8 matrix [n, L]; spec: the text or a parsed spec or ("lut", map).  Returns (matrix, report)."""
    if isinstance(spec, str):
        spec = parse(spec)
    rows = np.asarray(rows, dtype=np.uint8)
    if spec[0] == "pblock":
        out = np.array([pblock_row(r, spec[1]) for r in rows], dtype=np.uint8).reshape(rows.shape)
    else:
        lut = ill8_lut() if spec[0] == "ill8" else thr_lut(*spec[1:]) if spec[0] == "thr" else np.asarray(spec[1], dtype=np.uint8)
        if not is_idempotent(lut):
            raise LossyRefused("a map that is not idempotent")
        out = lut[rows]
    return out, report(rows, out)


# ---- the P-block rows every test walks (section "How to check"): name -> row of L bytes for a given P ------------------------------------
def pblock_rows(P: int, L: int):
    """constant; 33 / 126 alternating (every block one column); rising by 1 per column (blocks of 2 P + 1; wrapped into 33 .. 126 by a
    sawtooth so that it stays a quality line); a range of exactly 2 P (one block); a range of exactly 2 P + 1"""
    j = np.arange(L)
    rising = 33 + j % 94
    two_p = np.where(j % 2 == 0, 40, 40 + 2 * P)
    two_p1 = np.where(j % 2 == 0, 34, 34 + 2 * P + 1)
    if L >= 3:
        two_p[1] = 40 + P; two_p1[1] = 34 + P
    return {"constant": np.full(L, 70, np.uint8), "alternating": np.where(j % 2 == 0, 33, 126).astype(np.uint8), "rising": rising.astype(np.uint8),
            "range 2P": two_p.astype(np.uint8), "range 2P+1": two_p1.astype(np.uint8)}
