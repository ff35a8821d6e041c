"""The kernels that are compiled once per word count W = ceil(L / 32), at the first, an interior and the last read length of every W
(read_length_cases.SWEEP), bit for bit against the sequential oracle.  No tolerance anywhere.

Which (L, k, route) launches which instantiation:

  k_sketch_reads<W, WIDE, ODDK> (csrc/reads.hip; WIDE: k >= 17, ODDK: k odd) -- test_sketch_instantiations, every L of the row, every k
  of ks(L), over the whole array and through a row selector:

    W   L              <W,wide,odd>   <W,wide,even>   <W,narrow,odd>   <W,narrow,even>
    1   1, 19, 32      k = 31, 19, 17 k = 30 (L = 32) k = 15, 1        k = 16, 8
    2   33, 51, 64     k = 31, 17     k = 30          k = 15           k = 16, 8
    3   65, 83, 96     k = 31, 17     k = 30          k = 15           k = 16, 8
    4   97, 115, 128   k = 31, 17     k = 30          k = 15           k = 16, 8
    5   129, 147, 160  k = 31, 17     k = 30          k = 15           k = 16, 8
    6   161, 179, 192  k = 31, 17     k = 30          k = 15           k = 16, 8
    7   193, 211, 224  k = 31, 17     k = 30          k = 15           k = 16, 8
    8   225, 243, 256  k = 31, 17     k = 30          k = 15           k = 16, 8
  (L = 1 has k = 1 alone, L = 19 has k = 19, 17, 16, 15, 8: its only wide k are odd.)  Eight rows of four: all 32.

  The four copies of the classification rules (kthread_reads.c:84-224) -- test_classification_routes, every L of the row, e = 1 and 4,
  k = ks(L)[0]:

    W      L           route (a) pitch == L, aligned   routes (b) pitch > L and (c) pitch == L, unaligned base   route (d) packed input
    1 - 4  1 ... 128   k_classify_flat<W>              k_classify_pack<16>                                       k_classify_packed<W>
    5 - 8  129 ... 256 k_classify_flat<W>              k_classify_pack16                                         k_classify_packed<W>

  k_encode_byte<W>: test_encode_byte, W = 1 (L = 32) ... 8.  k_st_len<W> / k_st_emit<W> (csrc/streams.hip): test_stream_encoder at
  L = 32, 96, 161, 192, 224 (W = 1, 3, 6, 6, 7).  The realign, consensus, merge, decoder and whole-pipeline kernels get their missing
  word counts as parameters of their own tests (test_gpu_realign.py, test_gpu_consensus_edges.py, test_gpu_merge.py, test_gpu_decode.py,
  test_gpu_edges.py)."""
import os

import numpy as np
import pytest

import read_length_cases as rlc

pytestmark = pytest.mark.gpu

U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
N_READS = 2051                       # n % 64 = 3 (neither 0 nor 1); odd, so n L is no multiple of 16 unless L is
RID0 = 7


@pytest.fixture(scope="module")
def ctx():
    import minicom_amd
    c = minicom_amd.Context(0)
    yield c
    c.close()


def _pack_codes(reads):
    """Packed rows (A0 C1 G2 T3, anything else 0) and N flags of include/mcom.h, in numpy."""
    n, L = reads.shape
    code = np.zeros(256, dtype=np.uint64); code[ord("C")] = 1; code[ord("G")] = 2; code[ord("T")] = 3
    W, NW = (L + 31) // 32, (L + 63) // 64
    packed = np.zeros((n, W), dtype=np.uint64); nmask = np.zeros((n, NW), dtype=np.uint64)
    c = code[reads]; isn = (reads == ord("N")).astype(np.uint64)
    for i in range(L):
        packed[:, i // 32] |= c[:, i] << np.uint64(2 * (i % 32))
        nmask[:, i // 64] |= isn[:, i] << np.uint64(i % 64)
    return packed, nmask


def _classification_reads(L, e):
    from minicom_amd import synth
    directed, _ = rlc.class_matrix(L, e)
    reads = np.concatenate([directed, synth.synth_reads(500 + L + e, N_READS, L, plumbing=True)])[:N_READS]
    assert len(reads) == N_READS and N_READS % 64 not in (0, 1) and (L % 16 == 0 or (N_READS * L) % 16 != 0)
    return np.ascontiguousarray(reads), len(directed)


class _Want:
    """The oracle's answer for one batch: computed once, compared with every route."""

    def __init__(self, reads, k, e):
        import oracle
        self.reads, self.k, self.e = reads, k, e
        self.sub, self.cls, self.rec, self.ncnt = oracle.process_reads_batch(reads, k, e=e, rid0=RID0)
        self.keep = self.cls == 0
        self.packed = _pack_codes(self.sub[self.keep])[0]              # the N-substituted sequence of the kept reads, 2-bit packed
        self.nmask = _pack_codes(reads)[1]

    def check(self, out, route):
        """out: packed, cls, ncnt, nmask, rec as numpy arrays (the comparison of test_gpu_reads.py::_check_process, records in full)."""
        assert np.array_equal(out["cls"], self.cls), (route, np.flatnonzero(out["cls"] != self.cls)[:8].tolist())
        assert np.array_equal(out["ncnt"].view(np.uint16), self.ncnt), route
        assert np.array_equal(out["nmask"].view(np.uint64), self.nmask), route
        assert np.array_equal(out["packed"].view(np.uint64)[self.keep], self.packed), route
        rec = out["rec"].view(np.uint64)
        assert np.array_equal(rec[:, 0], self.rec["x"]) and np.array_equal(rec[:, 1], self.rec["y"]), route
        assert np.all(rec[~self.keep] == U64MAX), route


def _host(out):
    return {name: t.cpu().numpy() for name, t in out.items()}


@pytest.mark.parametrize("e", [1, 4])
@pytest.mark.parametrize("L", rlc.SWEEP)
def test_classification_routes(ctx, L, e):
    """Every directed row of read_length_cases.class_rows plus reads with the synthetic extras through every route of
    mcom_process_reads / mcom_process_reads_packed: packed rows, classes, N counts, N masks and records equal the oracle's."""
    import torch
    k = rlc.ks(L)[0]
    reads, n_directed = _classification_reads(L, e)
    n = len(reads)
    want = _Want(reads, k, e)
    if L >= 16:
        assert set(want.cls[:n_directed].tolist()) == set(range(8))

    # (a) rows back to back in a tensor of their own: the byte-stream kernel
    d = torch.from_numpy(reads).cuda()
    assert d.data_ptr() % 16 == 0
    first = ctx.process_reads(d, L, k, e=e, rid0=RID0, want_nmask=True)
    ctx.sync()
    want.check(_host(first), "flat")

    # (b) pitched rows; what lies between the rows would count if a lane took it for bases
    for pitch in (L + 1, L + 3, (L // 16 + 1) * 16 + 16):
        buf = np.empty((n, pitch), dtype=np.uint8)
        buf[:, 0::2] = ord("N"); buf[:, 1::2] = ord("T"); buf[:, :L] = reads
        out = ctx.process_reads(torch.from_numpy(buf).cuda(), L, k, e=e, rid0=RID0, want_nmask=True)
        ctx.sync()
        want.check(_host(out), "pitch %d" % pitch)

    # (c) rows back to back at a base address that is not 16-byte aligned: the call leaves the byte-stream kernel.  Input inside a
    # buffer of N, outputs inside filled arrays: nothing outside the rows may be read as a base, nothing outside the outputs written
    W, NW, G = (L + 31) // 32, (L + 63) // 64, 64
    for shift in (1, 7):
        host = np.full(G + n * L + G, ord("N"), dtype=np.uint8)
        host[shift:shift + n * L] = reads.ravel()
        big = torch.from_numpy(host).cuda()
        assert big.data_ptr() % 16 == 0
        rows = big[shift:shift + n * L].view(n, L)
        assert rows.data_ptr() % 16 == shift and rows.is_contiguous()
        packed = torch.full((G + n * W + G,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        nmask = torch.full((G + n * NW + G,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        rec = torch.full((G + 2 * n + G,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        cls = torch.full((G + n + G,), 0xEE, dtype=torch.uint8, device="cuda")
        ncnt = torch.full((G + n + G,), 0x5A5A, dtype=torch.int16, device="cuda")
        inner = {"packed": packed[G:G + n * W].view(n, W), "nmask": nmask[G:G + n * NW].view(n, NW), "rec": rec[G:G + 2 * n].view(n, 2),
                 "cls": cls[G:G + n], "ncnt": ncnt[G:G + n]}
        ctx._check(ctx.lib.mcom_process_reads(ctx._h, ctx._p(rows, torch.uint8), L, n, L, k, e, RID0, ctx._p(inner["packed"]), ctx._p(inner["cls"]),
                                              ctx._p(inner["ncnt"]), ctx._p(inner["nmask"]), ctx._p(inner["rec"])))
        ctx.sync()
        want.check(_host(inner), "shift %d" % shift)
        assert np.array_equal(big.cpu().numpy(), host)
        for name, t, fill, m in (("packed", packed, 0x5A5A5A5A5A5A5A5A, n * W), ("nmask", nmask, 0x5A5A5A5A5A5A5A5A, n * NW),
                                 ("rec", rec, 0x5A5A5A5A5A5A5A5A, 2 * n), ("cls", cls, 0xEE, n), ("ncnt", ncnt, 0x5A5A, n)):
            assert bool((t[:G] == fill).all()) and bool((t[G + m:] == fill).all()), (name, shift)

    # (d) packed input, out of place and in place
    hp, hn = _pack_codes(reads)
    dp, dn = torch.from_numpy(hp.view(np.int64)).cuda(), torch.from_numpy(hn.view(np.int64)).cuda()
    for in_place in (False, True):
        a, b = dp.clone(), dn.clone()
        out = ctx.process_reads_packed(a, b, L, k, e=e, rid0=RID0, in_place=in_place)
        ctx.sync()
        want.check(_host(out), "packed, in place" if in_place else "packed")
        assert (out["packed"].data_ptr() == a.data_ptr()) == in_place
        for name in ("packed", "cls", "ncnt", "nmask", "rec"):                 # rows of the other classes too: what the characters give
            assert torch.equal(out[name], first[name]), (name, in_place)
        if not in_place:
            assert torch.equal(a, dp) and torch.equal(b, dn)


@pytest.mark.parametrize("L", rlc.SWEEP)
def test_sketch_instantiations(ctx, L):
    """mcom_sketch_reads at every k of ks(L): the 4000 reads whose records reach both ends of the read on both strands
    (test_read_length_cases.py shows it on the oracle; asserted here on the batch) and the palindromic and homopolymer rows."""
    import torch
    import oracle
    from minicom_amd.hip import pack_nt4, records_to_numpy
    reads = np.concatenate([rlc.sketch_reads_for(L), rlc.directed_sketch_rows(L)])
    n, n_dir = len(reads), 6
    packed = torch.from_numpy(pack_nt4(reads).view(np.int64)).cuda()
    rng = np.random.default_rng(L)
    rids = rng.permutation(n)[: n // 3].astype(np.int32)
    rids[:n_dir] = np.arange(n - n_dir, n)                                     # the directed rows through the selector as well
    d_rids = torch.from_numpy(rids).cuda()
    for k in rlc.ks(L):
        want = oracle.sketch_two_batch(reads, k, rid0=11)
        got = records_to_numpy(ctx.sketch_reads(packed, L, k, rid0=11)); ctx.sync()
        assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["y"], want["y"]), (L, k)
        for i in range(n - n_dir, n):
            assert (int(got["x"][i]), int(got["y"][i])) == oracle.sketch_two(reads[i].tobytes(), k, 11 + i), (L, k, i)
        # what the batch held: both extreme positions on both strands, and (an even k has palindromes) a row without a minimizer
        y = want["y"][want["x"] != U64MAX]
        assert len(rlc.position_coverage(y, k, L)) == (4 if k < L else 2), (L, k)
        if k % 2 == 0:
            assert int((want["x"][n - n_dir:] == U64MAX).sum()) >= 1, (L, k)
        else:
            assert not (want["x"] == U64MAX).any()                             # an odd k-mer never equals its reverse complement
        # a shuffled third of the rows: the record carries the row's own id, rid0 plays no part
        base = oracle.sketch_two_batch(reads, k, rid0=0)
        sel = records_to_numpy(ctx.sketch_reads(packed, L, k, rids=d_rids, rid0=11)); ctx.sync()
        assert np.array_equal(sel["x"], base["x"][rids]) and np.array_equal(sel["y"], base["y"][rids]), (L, k, "rids")


@pytest.mark.parametrize("L", [L for L in rlc.SWEEP if L >= 32])
def test_encode_byte(ctx, L):
    """mcom_encode_byte against the oracle's encode_byte (kthread_hash_realign.c:283-314): both strands, windows at the first and the
    last position of a contig, both answers."""
    import torch
    import oracle
    from minicom_amd.hip import pack_nt4
    reads, contigs, cid, pos, dirs = rlc.encode_byte_cases(L)
    want = [oracle.encode_byte(reads[i].tobytes(), contigs[cid[i]] + b"\0", int(pos[i]), int(dirs[i]), L) for i in range(len(reads))]
    cg = ctx.upload_contigs(contigs)
    rows = torch.from_numpy(pack_nt4(reads).view(np.int64)).cuda()
    got = ctx.encode_byte(rows, cg, torch.from_numpy(cid).cuda(), torch.from_numpy(pos).cuda(), torch.from_numpy(dirs).cuda(), L)
    ctx.sync()
    assert got.cpu().numpy().tolist() == want, L
    assert set(want) == {0, 1}


@pytest.mark.parametrize("L", [32, 96, 161, 192, 224])
def test_stream_encoder(tmp_path, L):
    """The device encoder of cluster_dump (csrc/streams.hip, k_st_len<W> and k_st_emit<W>) writes the files of the host loop, byte for
    byte: the comparison of test_streams.py::test_device_stream_encoder_equals_the_host_loop at the other word counts."""
    from minicom_amd import synth
    from minicom_amd.pipeline import Pipeline
    reads = np.concatenate([synth.synth_reads(3030 + L, 6000, L), synth.synth_reads(3031 + L, 600, L, plumbing=True)])
    files = {}
    for how in (0, 1):
        p = Pipeline(reads, host_threads=2, host_dump=how)
        p.pre_process()
        d = tmp_path / f"streams{how}"; d.mkdir()
        p.cluster_dump(str(d))
        if how == 0:
            assert p.stat("dump_bytes") > 0                              # the device encoder ran
        p.close()
        files[how] = {f: (d / f).read_bytes() for f in sorted(os.listdir(d))}
    assert sorted(files[0]) == sorted(files[1])
    for name in files[1]:
        assert files[0][name] == files[1][name], name
    assert b"N" in files[0]["dif_char.txt.0"]
