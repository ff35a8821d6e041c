"""Shared inputs of the range-decode tests (tests/test_range.py on the host, tests/test_gpu_range.py on the device; DESIGN.md section
3.19): the golden -p folders, the grid of `.mcq` members and of (first, count) ranges, and the members with one flipped payload byte.
Everything is made once per process and handed out unchanged."""
import functools
import gzip
import io
import os
import tarfile

import numpy as np

import qual_cases as qc
import qual_reference as QR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TAGS = {"stages_L100": 3015, "stages_L150": 2015}          # golden -p stream files: tag -> reads


@functools.lru_cache(maxsize=None)
def golden_reads(tag):
    with gzip.open(os.path.join(GOLDEN, tag + ".reads.gz"), "rb") as f:
        rows = f.read().split(b"\n")[:-1]
    assert len(rows) == TAGS[tag]
    return tuple(rows)


def write_golden_folder(tag, folder):
    """the reference's -p stream files of `tag` into the (existing, empty) folder"""
    with gzip.open(os.path.join(GOLDEN, "streams_order_" + tag + ".tar.gz"), "rb") as g:
        tf = tarfile.open(fileobj=io.BytesIO(g.read()))
        for m in tf.getmembers():
            with open(os.path.join(str(folder), m.name), "wb") as f:
                f.write(tf.extractfile(m).read())


def read_ranges(n, seed):
    """the (first, count) of the issue: both ends, the clip, sixteen-lane group boundaries, and a seeded dozen"""
    fixed = [(0, 0), (0, 1), (n - 1, 1), (n, 5), (0, n), (0, n + 7), (15, 2), (16, 16), (17, n - 17)]
    rng = np.random.default_rng(seed)
    rand = []
    for _ in range(12):
        first = int(rng.integers(0, n + 1))
        rand.append((first, int(rng.integers(0, n - first + 20))))
    return fixed + rand


def tilings(n, seed):
    """three tilings of [0, n): lists of (first, count) whose outputs concatenate to the whole"""
    rng = np.random.default_rng(seed)
    out = [[(0, n // 3), (n // 3, n // 3), (2 * (n // 3), n)],              # thirds, the last one clipped
           [(0, 16), (16, 1), (17, n - 17)]]                                  # a sixteen-lane group, one row, the rest
    cuts = sorted(set(int(v) for v in rng.integers(1, n, 6)))
    edges = [0] + cuts + [n]
    out.append([(a, b - a) for a, b in zip(edges[:-1], edges[1:])])
    return out


# ---- quality members ----------------------------------------------------------------------------------------------------------------
QUAL_L = (1, 100, 150, 256)                                   # rows_per_seg 2048, 20, 13, 8
QUAL_A = (1, 4, 41, 94)
QUAL_MODELS = (0, 1, 2, 3, 4, "rans")                        # every forced model id, and kind 1


def _matrix(L, A, n):
    values = {1: [70], 4: [35, 45, 56, 70], 41: list(range(33, 74)), 94: list(range(33, 127))}[A]
    return qc._alphabet(1000 * L + A, n, L, values)


@functools.lru_cache(maxsize=None)
def qual_matrix(L, A):
    """2 rps + 3 rows: two whole segments and a short one"""
    q = _matrix(L, A, 2 * QR.default_rps(L) + 3)
    q.setflags(write=False)
    return q


def qual_ranges(L, n):
    rps = QR.default_rps(L)
    out = []
    for first in (0, 1, rps - 1, rps, rps + 1):
        for count in (0, 1, rps, rps + 1, n - first):
            out.append((first, count))
    return out


@functools.lru_cache(maxsize=None)
def qual_member(L, A, model):
    """the host encoder's member of qual_matrix(L, A) under a forced model"""
    from minicom_amd import pipeline
    return pipeline.qual_encode(qual_matrix(L, A), model)


def qual_grid():
    return [(L, A, model) for L in QUAL_L for A in QUAL_A for model in QUAL_MODELS]


def flip_in_segment(member: bytes, seg: int) -> bytes:
    """a coded member (kind 0, models 1 to 4) with one byte of segment `seg`'s run flipped: the header, the tables and the run lengths stay"""
    h = QR.parse_header(member)
    at = QR.HEADER + h["table_bytes"]
    lens = [int.from_bytes(member[at + 2 * s:at + 2 * s + 2], "little") for s in range(h["n_seg"])]
    run0 = at + 2 * h["n_seg"] + sum(lens[:seg])
    b = bytearray(member)
    b[run0 + lens[seg] // 2] ^= 0x5A
    return bytes(b)
