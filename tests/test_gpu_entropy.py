"""The built-in entropy stage on the GPU (csrc/entropy.hip) against its host twin: identical bytes, cross
decoding, the same hostile members refused, and the command line end to end with -G.  Then against the independent reference of
tests/rans_reference.py: the exact histogram counts and per-segment CRCs (test hooks of include/mcom_test.h), the encoder's bytes, the
decoder at the segment sizes no encoder writes, pointers that are not 16-byte aligned, the longest possible run and one crafted member
per refusal rule."""
import gzip
import os
import subprocess
import tarfile

import numpy as np
import pytest

import entropy_cases as ec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")


@pytest.fixture(scope="module")
def ctx():
    import minicom_amd
    return minicom_amd.Context(0)


def _dev(b):
    import torch
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda() if len(b) else torch.empty(0, dtype=torch.uint8, device="cuda")


def _host(t) -> bytes:
    return t.cpu().numpy().tobytes()


def test_device_bytes_equal_host_bytes_and_cross_decode(ctx, golden_dir):
    """every golden member and every synthetic case, default choice and every forced (model, stride): device encode == host encode,
    device decode of the host's member and host decode of the device's member give the original"""
    from minicom_amd import pipeline
    members = {"synthetic/" + k: v for k, v in ec.synthetic_members().items()}
    members.update(ec.golden_members(golden_dir))
    for name, raw in members.items():
        d_raw = _dev(raw)
        forced = ec.MODELS if (name.startswith("synthetic/") or name.startswith("order_stages_L100/") or name.startswith("pe_stages_L150/")) else ()
        for hint in (None,) + tuple(forced):
            kw = {} if hint is None else {"model": hint[0], "stride": hint[1]}
            host = pipeline.rans_encode(raw, **kw)
            dev = _host(ctx.rans_encode(d_raw, **kw))
            assert dev == host, (name, hint, len(dev), len(host))
            assert _host(ctx.rans_decode(_dev(host))) == raw, (name, hint)
            assert pipeline.rans_decode(dev) == raw, (name, hint)


def test_a_member_of_300_mb(ctx, golden_dir):
    """~300 MB (2.4 G bits: a 32-bit bit offset would wrap; 146 k segments, 572 workgroups): the same bytes as the host twin, and back"""
    from minicom_amd import pipeline
    import torch
    raw = ec.big_member(golden_dir, 300 * 1000 * 1000 + 1234)
    d_raw = torch.from_numpy(raw).cuda()
    for kw in ({}, {"model": 2, "stride": 1}):
        dev = ctx.rans_encode(d_raw, **kw)
        host = pipeline.rans_encode(raw.tobytes(), **kw)
        assert int(dev.shape[0]) == len(host)
        assert torch.equal(dev.cpu(), torch.from_numpy(np.frombuffer(host, dtype=np.uint8).copy())), kw
        back = ctx.rans_decode(dev)
        assert torch.equal(back, d_raw), kw
        del dev, back


def test_hostile_members_device_refuses_what_the_host_refuses(ctx, golden_dir):
    """a reduced, seeded sample of the CPU test's corpus (every 7th truncation, 300 flips) for the order-0 / order-1 members of one
    stream file: the device accepts exactly what the host accepts, and what it accepts is the original"""
    from minicom_amd import pipeline
    from minicom_amd.hip import McomError
    name, raw = ec.pick_hostile_member(golden_dir)
    for kw in ({}, {"model": 2, "stride": 2}):
        member = pipeline.rans_encode(raw, **kw)
        assert ec.parse_member(member)[0]["model"] != 0
        for label, bad in ec.hostile_corpus(member, flips=300, truncations=range(0, len(member), 7)):
            try:
                want = pipeline.rans_decode(bad, cap=len(raw))
            except McomError:
                want = None
            try:
                got = _host(ctx.rans_decode(_dev(bad), cap=len(raw)))
            except McomError:
                got = None
            assert got == want, (label, kw)
            assert want is None or want == raw, label


def _run(cmd, cwd):
    p = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-3000:]
    return p.stdout.decode(errors="replace")


@pytest.mark.parametrize("mode,tag,suffix", [("r", "stages_L100", "_comp"), ("p", "order_stages_L100", "_comp_order"), ("pe", "pe_stages_L100", "_comp_pe")])
def test_minicom_G_end_to_end(golden_dir, tmp_path, mode, tag, suffix):
    """minicom -r / -p / -1 -2 with -G at -t 1: every member ends in .rans, the archive holds the reference's stream files byte for byte,
    and both `minicom -d -G` and `minicom -d` (host twin) give the reads back"""
    from minicom_amd import container
    with gzip.open(os.path.join(golden_dir, "stages_L100.reads.gz"), "rb") as f:
        rows = f.read().split(b"\n")[:-1]
    half = len(rows) // 2

    def fastq(path, rs):
        with open(path, "wb") as f:
            for i, r in enumerate(rs):
                f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))
    if mode == "pe":
        fastq(tmp_path / "s_1.fastq", rows[:half]); fastq(tmp_path / "s_2.fastq", rows[half:2 * half])
        _run(["bash", os.path.join(BIN, "minicom"), "-1", "s_1.fastq", "-2", "s_2.fastq", "-t", "1", "-G"], tmp_path)
    else:
        fastq(tmp_path / "s.fastq", rows)
        _run(["bash", os.path.join(BIN, "minicom"), "-r", "s.fastq", "-t", "1", "-G"] + (["-p"] if mode == "p" else []), tmp_path)
    arch = tmp_path / ("s" + suffix + ".minicom")
    with tarfile.open(arch) as t:
        names = [os.path.basename(m.name) for m in t.getmembers() if m.isfile()]
    assert len(names) > 5 and all(n == "info.txt" or n.endswith(".rans") for n in names), names
    d = tmp_path / "unpacked"
    container.unpack(str(arch), str(d), device=0)
    want = {k.split("/")[1]: v for k, v in ec.golden_members(golden_dir).items() if k.split("/")[0] == tag}
    want.pop("ids.txt.0", None)
    assert sorted(os.listdir(d)) == sorted(want)
    for name, data in want.items():
        assert (d / name).read_bytes() == data, name
    base = arch.name[: -len(".minicom")]
    for flags in (["-G"], []):
        _run(["bash", os.path.join(BIN, "minicom"), "-d", arch.name] + flags, tmp_path)
        if mode == "pe":
            a = (tmp_path / (base + "_dec_1.reads")).read_bytes().split(b"\n")[:-1]
            b = (tmp_path / (base + "_dec_2.reads")).read_bytes().split(b"\n")[:-1]
            assert sorted(zip(a, b)) == sorted(zip(rows[:half], rows[half:2 * half])), flags
        else:
            got = (tmp_path / (base + "_dec.reads")).read_bytes().split(b"\n")[:-1]
            assert (got == rows if mode == "p" else sorted(got) == sorted(rows)), flags


# ---- the device against the independent reference (tests/rans_reference.py) --------------------------------------------------------------
SMALL_LENGTHS = (1, 15, 16, 17, 2047, 2048, 2049, 2063, 2064, 2065, 3 * 2048 - 1)


def _dev_at(b, off):
    """the bytes on the device, `off` bytes behind a 16-byte aligned address: a slice of a larger tensor, as the container passes"""
    import torch
    a = b if isinstance(b, np.ndarray) else np.frombuffer(b, dtype=np.uint8)
    buf = torch.empty(off + a.size + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + a.size]
    t.copy_(torch.from_numpy(a.copy()))
    assert t.data_ptr() % 16 == off % 16 and t.is_contiguous()
    return t


def _room_at(n, off):
    import torch
    buf = torch.empty(off + n + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf[off:off + n]


def _seven(n, seed=5):
    return np.random.default_rng(seed).integers(0, 7, size=n, dtype=np.uint8)


def _check_hist(ctx, raw, offsets, label):
    import torch
    import rans_reference as rr
    o0, o1 = (torch.from_numpy(a).cuda() for a in rr.ref_hist(raw))
    for off in offsets:
        g0, g1 = ctx.rans_test_hist(_dev_at(raw, off))
        assert torch.equal(g0, o0), (label, off, "order-0", int((g0 != o0).sum()))
        assert torch.equal(g1, o1), (label, off, "order-1", int((g1 != o1).sum()))


def test_histogram_counts_equal_the_reference(ctx):
    """k_rans_hist, launched as the encoder launches it, against numpy: every one of the 4 x 256 + 7 x 65536 counts, at lengths around a
    16-byte chunk and a segment, bytes of 7 symbols (contexts collide) and 32-bit words, the member 0, 1, 4 and 15 bytes behind an
    aligned address.  (A count above 2^32 -- the reason the counters are 64-bit -- takes a member of more than 4 GB of one
    (context, symbol): out of reach of a test of seconds.)"""
    for n in SMALL_LENGTHS:
        for label, raw in (("seven", _seven(n)), ("words", np.frombuffer(ec.words_bytes(n), dtype=np.uint8))):
            _check_hist(ctx, raw, (0, 1, 4, 15), (label, n))


@pytest.mark.parametrize("content", ["seven", "words", "one_value"])
def test_histogram_counts_beyond_the_grid_cap(ctx, content):
    """more 16-byte chunks than 8 workgroups per CU hold at once, so that the grid-stride loop goes round more than once (~9 MB); also
    all one value: one cell per plane takes every increment"""
    import torch
    n = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 4096 + 4096 + 5
    raw = _seven(n) if content == "seven" else np.frombuffer(ec.words_bytes(n), dtype=np.uint8) if content == "words" else np.full(n, 0xA5, dtype=np.uint8)
    _check_hist(ctx, raw, (0, 1), (content, n))


@pytest.mark.parametrize("seg_log2", [8, 11, 15])
def test_segment_crcs_equal_zlib(ctx, seg_log2):
    """k_rans_crc, launched as the codec launches it: the CRC-32 of every segment (the last one short) is zlib's"""
    import zlib
    for n in SMALL_LENGTHS + ((257 << 8) + 3,):
        raw = ec.words_bytes(n, seed=n)
        want = [zlib.crc32(raw[a:a + (1 << seg_log2)]) for a in range(0, n, 1 << seg_log2)]
        for off in (0, 1):
            got = ctx.rans_test_seg_crc(_dev_at(raw, off), seg_log2).cpu().tolist()
            assert got == want, (n, off)


def test_device_encode_equals_reference_encode(ctx):
    """every synthetic member x the six coded models: the device's bytes are the reference's -- the first comparison of the device with
    something that is not its twin.  Then with the input 1 and 15 bytes behind an aligned address and the member written 1 byte behind
    one (the byte-wise loads of the histogram, the CRC and the coder)"""
    syn = ec.synthetic_members()
    for name, raw in syn.items():
        d_raw = _dev(raw)
        for model, stride in ec.CODED_MODELS:
            assert _host(ctx.rans_encode(d_raw, model=model, stride=stride)) == ec.ref_member(raw, model, stride), (name, model, stride)
    bound = ctx.lib.mcom_rans_bound
    for name in ("skewed_4_symbols", "three_segments_minus_1", "words_u32"):
        raw = syn[name]
        for off in (1, 15):
            d_raw = _dev_at(raw, off)
            for model, stride in ec.CODED_MODELS:
                got = ctx.rans_encode(d_raw, model=model, stride=stride, out=_room_at(int(bound(len(raw))), 1))
                assert _host(got) == ec.ref_member(raw, model, stride), (name, off, model, stride)


OTHER_SEG_LENGTHS = {8: [(s << 8) + d for s in (63, 64, 65, 256, 257) for d in (-1, 0, 1)],          # a wave and a workgroup of segments, +- a byte
                     9: [(64 << 9) - 1, 64 << 9, (64 << 9) + 1, (65 << 9) + 17],
                     12: [1 << 12, (2 << 12) - 1, (5 << 12) + 33],
                     15: [1 << 15, (2 << 15) - 1]}


def _decode_both_ways(ctx, member, raw, label):
    assert _host(ctx.rans_decode(_dev(member))) == raw, (label, "aligned")
    got = ctx.rans_decode(_dev_at(member, 3), out=_room_at(len(raw), 5))
    assert got.data_ptr() % 16 == 5 and _host(got) == raw, (label, "member + 3, output + 5")


@pytest.mark.parametrize("model,stride", ec.CODED_MODELS)
@pytest.mark.parametrize("seg_log2", [8, 9, 12, 15])
def test_device_decodes_reference_members_at_other_segment_sizes(ctx, seg_log2, model, stride):
    """no encoder writes segments other than 2^11 bytes, so the decoder's rounds, lengths and store offsets for 2^8 .. 2^15 are only
    reached by members of the reference: lengths that cross a wave (64) and a workgroup (256) of segments, each decoded with member and
    output aligned and with the member 3, the output 5 bytes behind an aligned address (the byte-wise stores)"""
    for n in OTHER_SEG_LENGTHS[seg_log2]:
        raw = ec.words_bytes(n, seed=seg_log2)
        _decode_both_ways(ctx, ec.ref_member(raw, model, stride, seg_log2), raw, (seg_log2, model, stride, n))


def test_device_decodes_the_longest_run_a_u16_length_holds(ctx):
    """one segment of 2^15 symbols of frequency 1: a run of 49156 bytes, close to the top of the u16 length"""
    raw, member = ec.all_frequency_1_member(15)
    _, _, runs = ec.split_member(member)
    assert len(runs) == 1 and len(runs[0]) == 49156
    _decode_both_ways(ctx, member, raw, "frequency 1")


def test_worst_case_run_room_on_the_device(ctx):
    """the member of test_entropy.test_worst_case_run_room: the encoder's scratch run is filled to 3076 of 3080 bytes without raising its
    flag, the bytes are the host twin's, and the member decodes on the device"""
    from minicom_amd import pipeline
    raw = ec.worst_case_raw()
    host = pipeline.rans_encode(raw, model=1, stride=1)
    dev = ctx.rans_encode(_dev(raw), model=1, stride=1)
    assert _host(dev) == host
    assert _host(ctx.rans_decode(dev)) == raw


def test_crafted_refusals_on_the_device(ctx):
    """one member per refusal rule (entropy_cases.crafted_refusals; the host twin and the reference refuse them in test_entropy.py): the
    device raises for each and decodes the member they were made from"""
    from minicom_amd.hip import McomError
    raw, good, crafted = ec.crafted_refusals()
    assert _host(ctx.rans_decode(_dev(good))) == raw
    for label, bad in crafted.items():
        with pytest.raises(McomError):
            ctx.rans_decode(_dev(bad), cap=len(raw))
            pytest.fail("accepted: " + label)
