"""The one-launch prefix sums (csrc/scan.hip: mcom_scan_u32, mcom_scan64) and the read-back of their totals (csrc/api.hip: mcom_d2h_async,
mcom_stream_sync, the ring of pinned words and the table that tracks it) at their edges, through the test hooks of include/mcom_test.h.

The reference of every test is numpy in uint32 / uint64 arithmetic, which wraps like the kernels': the expected output of a scan of x is
concatenate([[0], cumsum(x)[:-1]]) modulo 2^32 or 2^64, and every comparison is exact.  Sizes come from the library's own constants
(threads of a workgroup, elements per thread) and from the compute units of the card, not from numbers written down here.

NOT covered: the poison path.  A bounded wait that runs out needs a workgroup that never publishes its sum, which no input brings about;
tests/test_gpu_claim.py covers the host side of the flag.  Every script here has to come back with MCOM_OK, i.e. with the flag down."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MCOM_OK = 0
PAD = 16                                                 # guard elements in front of an output region (keeps its start 16-byte aligned)
DT = {4: np.uint32, 8: np.uint64}
GUARD = {4: 0xA5A5A5A5, 8: 0xA5A5A5A5A5A5A5A5}          # what untouched output memory holds; the host arrays of a script start out the same


def _signed(v, width):
    return int(np.array([v], dtype=DT[width]).view({4: np.int32, 8: np.int64}[width])[0])


def _dev(a):
    """numpy uint32 / uint64 -> device int32 / int64 tensor (torch has no arithmetic-free unsigned types to speak of)"""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])).cuda()


def _exclusive(x):
    """E[i] = sum of x[:i] in x's own arithmetic, i = 0 .. len(x): E[:n] is the exclusive scan of x[:n] for every n"""
    return np.concatenate([np.zeros(1, x.dtype), np.cumsum(x, dtype=x.dtype)])


class _Env:
    def __init__(self):
        import minicom_amd
        self.ctx = minicom_amd.Context(0)
        k = minicom_amd.Context.scan_constants()
        self.threads, self.ring, self.tracked = k["threads"], k["ring_words"], k["tracked"]
        self.per = {4: k["per_u32"], 8: k["per_u64"]}
        self.tile = {w: self.threads * p for w, p in self.per.items()}
        self.m = min(2 * self.ctx.n_cu(), 2048)          # workgroups of a scan at the most
        assert self.m >= 2 and self.ring >= 8 and self.tracked >= 2
        # the shared input of the scripts: random words, read as uint32 or (two at a time) as uint64 at any element offset
        self.n32 = (max(max(self.sizes(4)), 2 * max(self.sizes(8))) + 8192) & ~1
        rng = np.random.default_rng(20250)
        self.x = {4: rng.integers(0, 1 << 32, self.n32, dtype=np.uint64).astype(np.uint32)}
        self.x[8] = self.x[4].view(np.uint64)
        self.e = {w: _exclusive(self.x[w]) for w in (4, 8)}
        self.d_x = _dev(self.x[4])

    def sizes(self, w):
        """the boundary sizes of a scan of w-byte elements; the last per[w] entries are one size for every residue n mod PER"""
        per, tile, m = self.per[w], self.tile[w], self.m
        s = [1, per - 1, per, per + 1, tile - 1, tile, tile + 1, 2 * tile, 64 * tile, 64 * tile + 1, 65 * tile + 1,
             m * tile - 1, m * tile, m * tile + 1, 2 * m * tile + 1, 3 * m * tile + per + 3]
        return s + [2 * tile + 1 + r for r in range(per)]

    def total(self, w, a, n):
        """the last element of the exclusive scan of the n elements of width w at element a of the shared input"""
        return (int(self.e[w][a + n - 1]) - int(self.e[w][a])) % 2 ** (8 * w)


@pytest.fixture(scope="module")
def env():
    e = _Env()
    yield e
    e.ctx.close()


def _values(kind, w, n, tile, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":                                 # full range: the sums wrap
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) if w == 4 else rng.integers(0, 1 << 64, n, dtype=np.uint64)
    if kind == "flags":                                  # what most callers scan; ~ tile / 32 ones per tile, so no chunk's sum is zero
        return (rng.integers(0, 32, n) == 0).astype(DT[w])
    # "carry": one large value per tile -- its low 32 bits just below 2^32, for uint64 a non-zero high half on top -- and a few small ones
    # that push some sums over the edge: both published halves of a chunk's sum matter, and the carry from the low one into the high one
    x = np.zeros(n, dtype=DT[w])
    x[rng.integers(0, n, max(n // 97, 1))] = rng.integers(1, 8, max(n // 97, 1)).astype(DT[w])
    at = np.minimum(np.arange(0, n, tile) + rng.integers(0, tile, (n + tile - 1) // tile), n - 1)
    big = np.uint64(0xFFFFFFFF) - rng.integers(0, 4, at.size).astype(np.uint64)
    if w == 8:
        big |= rng.integers(1, 1 << 20, at.size).astype(np.uint64) << np.uint64(32)
    x[at] = big.astype(DT[w])
    return x


def _check_region(buf, lo, n, want, w, what):
    """buf[lo : lo + n] == want[:n] and every other element of buf is the guard (device tensors)"""
    import torch
    g = _signed(GUARD[w], w)
    got = buf[lo:lo + n]
    if not torch.equal(got, want[:n]):
        bad = int(torch.nonzero(got != want[:n])[0])
        raise AssertionError(f"{what}: element {bad} of {n} is {int(got[bad]) & (2 ** (8 * w) - 1):#x}, expected {int(want[bad]) & (2 ** (8 * w) - 1):#x}")
    assert bool((buf[:lo] == g).all()), f"{what}: wrote in front of the output"
    if not bool((buf[lo + n:] == g).all()):
        bad = int(torch.nonzero(buf[lo + n:] != g)[0])
        raise AssertionError(f"{what}: wrote {bad} elements past the end of the output")


def _scan_checked(env, w, d_src, in_off, n, out_off, want, what, in_place=False):
    """one scan of d_src[in_off : in_off + n] to element PAD + out_off of a guarded buffer of its own, or in place in a guarded copy"""
    import torch
    tail = 2 * env.tile[w] + PAD                         # room behind the output: a store past the end stays inside the buffer and is seen
    buf = torch.full((PAD + out_off + n + tail,), _signed(GUARD[w], w), dtype=d_src.dtype, device=d_src.device)
    dst = buf[PAD + out_off:]
    if in_place:
        dst[:n] = d_src[in_off:in_off + n]
        env.ctx.scan_async(dst, dst, n)
    else:
        env.ctx.scan_async(d_src[in_off:], dst, n)
    _check_region(buf, PAD + out_off, n, want, w, what)


@pytest.mark.parametrize("kind", ["random", "carry", "flags"])
@pytest.mark.parametrize("w", [4, 8])
def test_scan_at_every_boundary_size(env, w, kind):
    """1 and PER +- 1 (the scalar tail of so_load / so_store), TILE +- 1 (one workgroup against the ticket protocol), workgroups 64 and
    65 (the look-back's second trip), M * TILE +- 1 (one tile per workgroup against two: `base += all`), three and four tiles per chunk
    with a short last chunk, and every n mod PER (the lane that stores the total)."""
    sizes = env.sizes(w)
    x = _values(kind, w, max(sizes), env.tile[w], 7 * w + len(kind))
    d_x, d_want = _dev(x), _dev(_exclusive(x))
    for n in sizes:
        _scan_checked(env, w, d_x, 0, n, 0, d_want, f"u{8 * w} {kind} n={n}")


@pytest.mark.parametrize("w", [4, 8])
def test_scan_at_every_alignment_and_in_place(env, w):
    """input and output at every element offset inside 16 bytes, independently: the vector and the scalar branch of so_load and of
    so_store in all four combinations; and in place (in == out, as mcom_contig_layout scans) at every offset.  One workgroup pair
    (TILE + 1) and two tiles per workgroup (M * TILE + 1).  The guard around the output catches a store past `last`."""
    offs = range(16 // w)
    top = env.m * env.tile[w] + 1
    x = _values("random", w, top + 16 // w, env.tile[w], 99 + w)
    d_x = _dev(x)
    want = {a: _dev(_exclusive(x[a:a + top])) for a in offs}
    for n in (env.tile[w] + 1, top):
        for a, b in itertools.product(offs, offs):
            _scan_checked(env, w, d_x, a, n, b, want[a], f"u{8 * w} n={n} in+{a} out+{b}")
        for a in offs:
            _scan_checked(env, w, d_x, a, n, a, want[a], f"u{8 * w} n={n} in place +{a}", in_place=True)


# ---- scripted sequences ------------------------------------------------------------------------------------------------------------
class _Script:
    """Steps for mcom_test_scan_script over the shared input (env.d_x) and a guarded output buffer, with what numpy expects of them."""

    def __init__(self, env):
        from minicom_amd import hip
        self.env, self.hip = env, hip
        self.steps, self.scans, self.reads, self.copies = [], {}, [], []
        self.out_bytes, self.copy_bytes = 16 * PAD, 0

    def _add(self, op, width=0, a=0, b=0, n=0):
        self.steps.append((op, width, a, b, n))
        return len(self.steps) - 1

    def region(self, w, n):
        """a fresh output region for n elements of width w: its element offset (16-byte aligned, a guard gap in front)"""
        off = self.out_bytes // w
        self.out_bytes = (self.out_bytes + n * w + 64 + 15) & ~15
        return off

    def scan(self, w, n, a=0, b=None):
        """scan n elements at element a of the input to element b of the output (None: a fresh region); -> the step's index"""
        b = self.region(w, n) if b is None else b
        i = self._add(self.hip.SCAN_STEP_SCAN, w, a, b, n)
        self.scans[i] = (w, a, b, n)
        return i

    def readback(self, i, expect=None):
        """the last output element of scan step i; expect: the value if it is not that scan's own total"""
        w, a, _, n = self.scans[i]
        self.reads.append((w, self.env.total(w, a, n) if expect is None else expect, f"read-back {len(self.reads)} of step {i} (u{8 * w}, n={n})"))
        self._add(self.hip.SCAN_STEP_READBACK, 0, i, len(self.reads) - 1)

    def last_byte_offset(self, i):
        w, _, b, n = self.scans[i]
        return (b + n - 1) * w

    def launch(self, poke_at=None, value=0):
        self._add(self.hip.SCAN_STEP_LAUNCH, 0, poke_at or 0, value, 0 if poke_at is None else 1)

    def copy(self, src, at, nbytes, expect, what):
        """nbytes from byte `at` of the output (src 0) or the input (src 1); expect: the bytes"""
        self._add(self.hip.SCAN_STEP_COPY, src, at, self.copy_bytes, nbytes)
        self.copies.append((self.copy_bytes, nbytes, bytes(expect), what))
        self.copy_bytes += nbytes + 3                     # (host destinations at odd addresses, a gap of fill bytes between them)

    def sync(self):
        self._add(self.hip.SCAN_STEP_SYNC)

    def run(self, check_outputs=True):
        import torch
        env = self.env
        tail = 2 * env.tile[4] * 8 + 64
        d_out = torch.full(((self.out_bytes + tail) // 8,), _signed(GUARD[8], 8), dtype=torch.int64, device=env.d_x.device)
        steps = np.array(self.steps, dtype=self.hip.SCAN_STEP_DTYPE)
        rc, tot, cp = env.ctx.scan_script(steps, env.d_x, d_out, len(self.reads), self.copy_bytes)
        assert rc == MCOM_OK, f"script failed with {rc}: {env.ctx.lib.mcom_last_error(env.ctx._h).decode()}"
        for j, (w, want, what) in enumerate(self.reads):
            got = int(tot[j])
            assert got & (2 ** (8 * w) - 1) == want, f"{what}: {got & (2 ** (8 * w) - 1):#x}, expected {want:#x}"
            assert w == 8 or got >> 32 == GUARD[4], f"{what}: wrote more than {w} bytes"
        for at, nb, want, what in self.copies:
            assert cp[at:at + nb].tobytes() == want, f"{what}: {cp[at:at + nb].tobytes().hex()}, expected {want.hex()}"
            assert np.all(cp[at + nb:at + nb + 3] == 0xA5), f"{what}: wrote past its {nb} bytes"
        if check_outputs:
            self.check_outputs(d_out)
        return d_out

    def check_outputs(self, d_out):
        """every scan's region holds its scan (regions written once), and whatever lies between the regions is untouched"""
        import torch
        env = self.env
        want = {4: _dev(env.e[4]), 8: _dev(env.e[8])}
        view = {4: d_out.view(torch.int32), 8: d_out}
        seen = torch.zeros(d_out.numel() * 2, dtype=torch.bool, device=d_out.device)       # per 32-bit word: inside a region
        for i, (w, a, b, n) in self.scans.items():
            got = view[w][b:b + n]
            ref = want[w][a:a + n] - want[w][a]
            if not torch.equal(got, ref):
                bad = int(torch.nonzero(got != ref)[0])
                raise AssertionError(f"step {i} (u{8 * w}, n={n}): element {bad} is {int(got[bad]) & (2 ** (8 * w) - 1):#x}, expected {int(ref[bad]) & (2 ** (8 * w) - 1):#x}")
            seen[b * w // 4:(b + n) * w // 4] = True
        assert bool((view[4][~seen] == _signed(GUARD[4], 4)).all()), "a scan wrote outside its region"


def _mixed_sizes(env):
    """(width, n) pairs for the scripts about totals: one workgroup and several, both widths in turn, no two alike"""
    out = []
    for q in range(200):
        w = 4 if q % 2 == 0 else 8
        n = (1, env.per[w] + 1, env.tile[w] - 1, env.tile[w] + 1, 3 * env.tile[w] + 5, 65 * env.tile[w] + 1, env.m * env.tile[w] + 1)[q % 7]
        out.append((w, n + q))
    return out


def test_200_scans_back_to_back(env):
    """no synchronisation between the launches: the ticket counter has to be back at zero and no published word of an earlier launch may
    pass for this one's.  Sizes cycle through the boundary list of each width, the widths alternate, every scan has a region of its own."""
    s = _Script(env)
    sz = {w: env.sizes(w) for w in (4, 8)}
    for q in range(200):
        w = 4 if q % 2 == 0 else 8
        s.scan(w, sz[w][(q // 2) % len(sz[w])])
    s.run()


def test_ticket_counter_is_back_at_zero_for_the_next_launch(env):
    """the smallest case of the above: three launches of two workgroups each.  With a counter left at 2 the second launch's workgroups
    would take chunks 2 and 3, which do not exist, and wait for sums nobody publishes."""
    s = _Script(env)
    for w in (4, 8, 4):
        s.scan(w, env.tile[w] + 1)
    s.run()


def test_two_contexts_in_turn(env):
    """a scan on each of two contexts in turn, unsynchronised: their published sums, tickets and rings are separate"""
    import minicom_amd
    import torch
    other = minicom_amd.Context(0)
    try:
        jobs = []
        for q in range(24):
            w = 4 if (q // 2) % 2 == 0 else 8
            n = (env.tile[w] + 1, 65 * env.tile[w] + 1, env.m * env.tile[w] + 1)[(q // 4) % 3] + q
            src = env.d_x if w == 4 else env.d_x.view(torch.int64)
            buf = torch.full((PAD + n + 2 * env.tile[w],), _signed(GUARD[w], w), dtype=src.dtype, device=src.device)
            (env.ctx if q % 2 == 0 else other).scan_async(src, buf[PAD:], n)
            jobs.append((w, n, buf))
        env.ctx.sync(); other.sync()
        want = {w: _dev(env.e[w]) for w in (4, 8)}
        for q, (w, n, buf) in enumerate(jobs):
            _check_region(buf, PAD, n, want[w], w, f"scan {q} (context {q % 2}, u{8 * w}, n={n})")
    finally:
        other.close()


def test_totals_read_back_at_once(env):
    """1 .. 8 scans, each followed at once by its read-back, then one synchronisation: every total is in the ring.  Both widths: a uint32
    total is the low half of the ring's 8-byte word, and only 4 bytes of the destination may change."""
    pairs = _mixed_sizes(env)
    for k in range(1, env.tracked + 1):
        s = _Script(env)
        for w, n in pairs[k:2 * k]:
            s.readback(s.scan(w, n))
        s.run()


@pytest.mark.parametrize("w", [4, 8])
def test_total_at_every_boundary_size(env, w):
    """the word the kernel stores for the host, whichever lane and workgroup holds element n - 1: every boundary size, every n mod PER"""
    s = _Script(env)
    assert len(env.sizes(w)) < env.ring
    for n in env.sizes(w):
        s.readback(s.scan(w, n))
    s.run()


@pytest.mark.parametrize("k", [9, 63, 64, 65, 130])
def test_totals_read_back_after_many_scans(env, k):
    """k scans in a row, then all the read-backs, then one synchronisation: only the newest scans are tracked (the others' totals come by
    copy), and past 64 scans the ring's words have been handed out again"""
    assert env.tracked < 9 and env.ring == 64
    s = _Script(env)
    ids = [s.scan(w, n) for w, n in _mixed_sizes(env)[:k]]
    for i in ids:
        s.readback(i)
    s.run()


def test_ring_word_comes_round_while_its_read_back_waits(env):
    """70 times scan + read-back, one synchronisation at the end: scan 65 gets the ring word of scan 1, whose value is still waiting there.
    This FAILED before: scan_one launched the new scan first and served the waiting read-backs afterwards (mcom_ring_flush_slot
    behind MCOM_LAUNCH), so a read-back 64 scans old received the NEW scan's total.  They are served before the launch now."""
    s = _Script(env)
    for w, n in _mixed_sizes(env)[:env.ring + 6]:
        s.readback(s.scan(w, n))
    s.run()


def test_totals_after_another_launch(env):
    """scan, another kernel, read-back: the tracked entry no longer counts and the value comes by copy -- seen because the other kernel
    CHANGES the word; and a kernel that changes nothing in between; and a synchronisation in between"""
    for w in (4, 8):
        n = 3 * env.tile[w] + 7
        s = _Script(env)
        i = s.scan(w, n)
        s.launch(s.last_byte_offset(i), 0x12345678)
        s.readback(i, expect=(s.env.total(w, 0, n) & ~0xFFFFFFFF) | 0x12345678)
        j = s.scan(w, n + 1)
        s.launch()
        s.readback(j)
        k = s.scan(w, n + 2)
        s.sync()
        s.readback(k)
        d_out = s.run(check_outputs=False)
        del d_out


def test_totals_of_earlier_scans_in_a_row(env):
    """scan, scan, then the FIRST scan's read-back (scans in a row keep the earlier totals valid), the same three scans deep, both widths"""
    s = _Script(env)
    a = s.scan(4, env.tile[4] + 3)
    b = s.scan(8, 2 * env.tile[8] + 1)
    s.readback(a)
    c = s.scan(4, 5)
    s.readback(b); s.readback(a); s.readback(c)
    s.run()


def test_total_of_an_overwritten_output(env):
    """a scan into region A, a second scan of other data over A, then the read-back of A's last element: the second scan's value.  Once
    with the same length (the second scan's own total) and once with a longer second scan, where A's last element lies INSIDE the
    second output and only the copy can be right."""
    for w in (4, 8):
        n = env.tile[w] + 9
        s = _Script(env)
        ra, rb = s.region(w, n), s.region(w, 2 * n)
        a = s.scan(w, n, a=0, b=ra)
        s.scan(w, n, a=1000, b=ra)
        s.readback(a, expect=env.total(w, 1000, n))
        b = s.scan(w, n, a=0, b=rb)
        s.scan(w, 2 * n, a=2000, b=rb)
        s.readback(b, expect=env.total(w, 2000, n))
        assert env.total(w, 0, n) not in (env.total(w, 1000, n), env.total(w, 2000, n))
        s.run(check_outputs=False)


def test_read_back_of_another_width(env):
    """4 bytes of a uint64 scan's last element: its low word.  8 bytes at a uint32 scan's last element: that element and the word behind
    it (the guard) -- the ring's word would have zeros there, so a ring hit of the wrong size shows."""
    s = _Script(env)
    n8, n4 = env.tile[8] + 5, env.tile[4] + 5
    a = s.scan(8, n8)
    s.copy(0, s.last_byte_offset(a), 4, (env.total(8, 0, n8) & 0xFFFFFFFF).to_bytes(4, "little"), "4 bytes of a uint64 total")
    b = s.scan(4, n4)
    s.copy(0, s.last_byte_offset(b), 8, (env.total(4, 0, n4) | GUARD[4] << 32).to_bytes(8, "little"), "8 bytes at a uint32 total")
    s.run()


def test_small_copies_past_the_pinned_page(env):
    """600 copies of 8 bytes and a few of 256 before one synchronisation: the 4096-byte page fills up and the later ones go straight to
    their destinations; scans and their read-backs among them"""
    s = _Script(env)
    raw = env.x[4].view(np.uint8)
    pairs = _mixed_sizes(env)
    for q in range(600):
        at = 3 + 11 * q
        s.copy(1, at, 8, raw[at:at + 8], f"copy {q} of 8 bytes")
        if q % 40 == 7:
            s.readback(s.scan(*pairs[q // 40]))
        if q in (100, 300, 599):
            at = 5 + 100 * q
            s.copy(1, at, 256, raw[at:at + 256], f"copy of 256 bytes after {q}")
    s.run()


@pytest.mark.parametrize("n", ["0", "1", "tile-1", "tile"])
def test_contig_layout_at_the_scan_edges(env, n):
    """mcom_contig_layout: an in-place uint64 scan of n + 1 words and its total.  No contig, one, and n + 1 = TILE and TILE + 1; contigs of
    length 0 among the others."""
    n = {"0": 0, "1": 1, "tile-1": env.tile[8] - 1, "tile": env.tile[8]}[n]
    rng = np.random.default_rng(n)
    lens = rng.integers(0, 5000, n)
    lens[rng.integers(0, 4, n) == 0] = 0
    soff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    coff, clen, tw = env.ctx.contig_layout(_dev(soff.view(np.uint64)))
    words = (2 * lens + 63) // 64 + 1
    assert np.array_equal(coff.cpu().numpy(), np.concatenate([[0], np.cumsum(words)]).astype(np.int64))
    assert tw == int(words.sum())
    assert np.array_equal(clen.cpu().numpy(), lens)
