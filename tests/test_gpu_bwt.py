"""The block-sorting coder on the GPU (csrc/bwt.hip) against its host twin and the independent reference of
tests/bwt_reference.py: identical bytes, the decoder at block and anchor sizes no encoder writes, pointers that are not 16-byte aligned,
one crafted member per refusal rule, the stages through the hooks of include/mcom_test.h, and the container's route."""
import os

import numpy as np
import pytest

import bwt_cases as bc
import bwt_reference as br

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import minicom_amd
    return minicom_amd.Context(0)


def _dev(b):
    import torch
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda() if len(b) else torch.empty(0, dtype=torch.uint8, device="cuda")


def _host(t) -> bytes:
    return t.cpu().numpy().tobytes()


def test_device_bytes_equal_host_twin_and_reference(ctx, golden_dir):
    """every small member: device encode == host encode (== the reference's member where one block of the encoder's size is within the
    reference's reach), device decode of it gives the original"""
    from minicom_amd import pipeline
    for name, raw in bc.small_members(golden_dir).items():
        host = pipeline.bwt_encode(raw)
        dev = _host(ctx.bwt_encode(_dev(raw)))
        assert dev == host, (name, len(dev), len(host))
        if len(raw) <= 4096:
            assert dev == bc.ref_member(raw, br.BLK_LOG2, br.ANC_LOG2), name
        assert _host(ctx.bwt_decode(_dev(host))) == raw, name


def test_members_around_the_block_size(ctx, golden_dir):
    """one block, one block + 1 byte, three blocks with a short last one (about 3 MiB) and an all-equal block: device == host twin, both
    ways.  The text members come out block sorted; the all-equal one does not (plain rANS codes it as small: a tie goes to plain), so
    its transform is held against the host twin's stage by stage in test_all_equal_block_takes_every_round"""
    from minicom_amd import pipeline
    for name, raw in bc.block_members(golden_dir).items():
        host = pipeline.bwt_encode(raw)
        dev = _host(ctx.bwt_encode(_dev(raw)))
        assert dev == host, (name, len(dev), len(host))
        assert host[5] == (br.PLAIN if name.startswith("all_equal") else br.BWT), name
        assert _host(ctx.bwt_decode(_dev(host))) == raw, name


def test_all_equal_block_takes_every_round(ctx, golden_dir):
    """2^20 + 4097 equal bytes: two suffixes of an all-equal block tie until the compared prefix (2^(r+1) bytes after round r) is as long
    as the shorter one, so the first block settles in round 19, the 20th -- the longest the doubling loop can run at this block size but
    for its last round.  Transformed bytes, index and ranks equal the host twin's, and the ranks decode back"""
    from minicom_amd import pipeline
    raw = bc.block_members(golden_dir)["all_equal_block_and_a_bit"]
    want_tr, want_ix, want_ranks = pipeline.bwt_stages(raw)
    tr, ix, rounds = ctx.bwt_test_forward(_dev(raw))
    assert ix.tolist() == want_ix and _host(tr) == want_tr
    assert br.BLK_LOG2 <= rounds <= br.BLK_LOG2 + 1, rounds
    ranks = ctx.bwt_test_mtf(tr)
    assert _host(ranks) == want_ranks
    assert _host(ctx.bwt_test_mtf(ranks, decode=True)) == want_tr


def test_decoder_at_the_geometries_no_encoder_writes(ctx, golden_dir):
    """the reference's members at blocks of 2^8 / 2^12 bytes and anchors every 2^4 / 2^8: the device decodes each to the original"""
    for label, raw, member in bc.decoder_cases(golden_dir):
        assert _host(ctx.bwt_decode(_dev(member))) == raw, label


@pytest.mark.parametrize("offset", [1, 7, 13])
def test_addresses_that_are_not_16_byte_aligned(ctx, golden_dir, offset):
    """input, member and output at `offset` bytes into larger buffers: the same bytes, and nothing written outside"""
    import torch
    from minicom_amd import pipeline
    raw = bc.text_member(golden_dir, 8000) * 7 + b"x"
    host = pipeline.bwt_encode(raw)
    assert host[5] == br.BWT
    src = torch.full((len(raw) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    src[offset:offset + len(raw)] = _dev(raw)
    room = torch.full((len(host) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    got = ctx.bwt_encode(src[offset:offset + len(raw)], out=room[offset:offset + len(host)])
    assert _host(got) == host
    assert bool((room[:offset] == 0xEE).all()) and bool((room[offset + len(host):] == 0xEE).all())
    back = torch.full((len(raw) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    out = ctx.bwt_decode(room[offset:offset + len(host)], out=back[offset:offset + len(raw)])
    assert _host(out) == raw
    assert bool((back[:offset] == 0xEE).all()) and bool((back[offset + len(raw):] == 0xEE).all())


def test_crafted_refusals_on_the_device(ctx, golden_dir):
    """one member per refusal rule (the host twin and the reference refuse them in test_bwt.py): the device raises for each and decodes
    the member they were made from.  What a refused call leaves behind: the room offered may hold part of the text -- a
    walk writes its bytes before it finds that it does not chain, and the CRC is judged last -- but nothing outside that room is
    written, and the members refused on the host (header, embedded header, index rows) leave the room itself untouched"""
    import torch
    from minicom_amd import pipeline
    from minicom_amd.hip import McomError
    raw, good, crafted = bc.crafted_refusals(golden_dir)
    assert _host(ctx.bwt_decode(_dev(good))) == raw
    for label, bad in crafted.items():
        with pytest.raises(McomError):
            pipeline.bwt_decode(bad)
        back = torch.full((len(raw) + 1 + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        with pytest.raises(McomError):
            ctx.bwt_decode(_dev(bad), out=back[32:32 + len(raw) + 1])
            pytest.fail("the device accepted " + label)
        assert bool((back[:32] == 0xEE).all()) and bool((back[32 + len(raw) + 1:] == 0xEE).all()), label
        if br_rule(bad) in ("header", "embedded-header", "index"):
            assert bool((back == 0xEE).all()), label
    assert _host(ctx.bwt_decode(_dev(good))) == raw


def br_rule(member: bytes) -> str:
    """which of the reference's rules refuses the member; "embedded-header" when it is the embedded member's header, judged before a launch"""
    import rans_reference as rr
    try:
        br.ref_decode(member)
    except br.BwtRefused as e:
        if e.rule != "embedded":
            return e.rule
        try:
            h = br.parse_header(member)
            eh = rr.parse_header(member[br.HEADER + h["index_bytes"]:])
        except rr.RansRefused:
            return "embedded-header"
        return "embedded-header" if eh["raw_len"] != h["raw_len"] or (h["kind"] == br.PLAIN and eh["crc"] != h["crc"]) else "embedded"
    return "accepted"


def test_file_route_on_the_device_leaves_no_output_for_a_refused_member(golden_dir, tmp_path):
    """mcomz e --bwt --gpu / mcomz d --gpu give the file back (the member equals the host twin's); a member refused by a walk, by the CRC
    and by the header each end with status 1, the member's kind in the message, and no output file"""
    import subprocess
    from minicom_amd import pipeline
    mcomz = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "mcomz")
    raw = bc.text_member(golden_dir, 8000) * 3
    (tmp_path / "in").write_bytes(raw)
    subprocess.run([mcomz, "e", "--bwt", "--gpu", str(tmp_path / "in"), str(tmp_path / "m.bwt")], check=True)
    assert (tmp_path / "m.bwt").read_bytes() == pipeline.bwt_encode(raw)
    subprocess.run([mcomz, "d", "--gpu", str(tmp_path / "m.bwt"), str(tmp_path / "back")], check=True)
    assert (tmp_path / "back").read_bytes() == raw
    _, _, crafted = bc.crafted_refusals(golden_dir)
    for label in ("anchors_do_not_chain", "wrong_raw_crc", "blk_log2_7"):
        (tmp_path / "bad").write_bytes(crafted[label])
        p = subprocess.run([mcomz, "d", "--gpu", str(tmp_path / "bad"), str(tmp_path / "out")], capture_output=True, text=True)
        assert p.returncode == 1 and not (tmp_path / "out").exists(), label
        if label != "blk_log2_7":
            assert ".bwt member" in p.stderr, (label, p.stderr)


def test_forward_stage_against_the_reference(ctx, golden_dir):
    """the transformed bytes and the index (mcom_test_bwt_forward) of members of one block of at most 2^12 bytes against the reference's,
    and of the 3 MiB member against the host twin's"""
    from minicom_amd import pipeline
    for name, raw in bc.small_members(golden_dir).items():
        if not 0 < len(raw) <= 4096:
            continue
        want_tr, want_ix, _ = br.ref_stages(raw, br.BLK_LOG2, br.ANC_LOG2)
        tr, ix, rounds = ctx.bwt_test_forward(_dev(raw))
        assert _host(tr) == want_tr and ix.tolist() == want_ix, name
        assert 1 <= rounds <= br.BLK_LOG2 + 1, (name, rounds)
    raw = bc.block_members(golden_dir)["three_blocks_last_short"]
    want_tr, want_ix, _ = pipeline.bwt_stages(raw)
    tr, ix, rounds = ctx.bwt_test_forward(_dev(raw))
    assert ix.tolist() == want_ix and _host(tr) == want_tr
    assert rounds < br.BLK_LOG2 + 1, rounds                                  # text with noise every 997 bytes settles early


def test_mtf_stage_against_the_reference(ctx, golden_dir):
    """the move-to-front ranks (mcom_test_bwt_mtf), both directions, against the reference's sequential coder over blocks of 2^20 bytes:
    a short member, then one block + 2053 bytes of a few symbols and of all 256 (every stretch changes the whole list)"""
    rng = np.random.default_rng(3)
    members = [bc.text_member(golden_dir, 5000)] + [rng.integers(0, hi, size=bc.BLK + 2053, dtype=np.uint8).tobytes() for hi in (5, 256)]
    for data in members:
        want = b"".join(br.mtf(data[a:a + bc.BLK]) for a in range(0, len(data), bc.BLK))
        ranks = ctx.bwt_test_mtf(_dev(data))
        assert _host(ranks) == want, len(data)
        assert _host(ctx.bwt_test_mtf(ranks, decode=True)) == data, len(data)


def test_container_route_on_the_device(ctx, golden_dir, tmp_path):
    """compress_fastq(codec="bwt", device=0) on the smallest golden read set (L = 40) as a FASTQ, decompress_file(device=0) and verify_file: the reads come
    back, and the archive's `.bwt` members equal the host twin's"""
    import gzip
    import tarfile
    from minicom_amd import container, pipeline
    with gzip.open(os.path.join(golden_dir, "stages_L40.reads.gz"), "rb") as f:
        rows = f.read().split(b"\n")[:-1]
    fq = str(tmp_path / "r.fastq")
    with open(fq, "wb") as f:
        for i, r in enumerate(rows):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))
    arc = str(tmp_path / "a.minicom")
    sizes = container.compress_fastq(fq, arc, codec="bwt", device=0)
    assert sizes["n_reads"] == len(rows)
    out = str(tmp_path / "reads.txt")
    assert container.decompress_file(arc, out, device=0) == len(rows)
    rep = container.verify_file(arc, fq, device=0)
    assert rep["identical"], rep
    with open(out, "rb") as f:
        assert sorted(f.read().split(b"\n")[:-1]) == sorted(rows)
    with tarfile.open(arc) as t:
        members = [(m.name, t.extractfile(m).read()) for m in t.getmembers() if m.name.endswith(".bwt")]
    assert members
    for name, data in members:
        assert data == pipeline.bwt_encode(pipeline.bwt_decode(data)), name
