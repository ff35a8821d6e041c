"""The block-sorting coder's host twin (host/mcom_bwt.cpp) against the independent reference of
tests/bwt_reference.py: the same bytes, the decoder at block and anchor sizes no encoder writes, the bound that holds by construction,
the compression the transform is there for, one crafted member per refusal rule, the container and the command line, and once under
AddressSanitizer + UBSan as a stand-alone program."""
import os
import subprocess
import tarfile

import pytest

import bwt_cases as bc
import bwt_reference as br
import entropy_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
HEADER = 40


@pytest.fixture(scope="module")
def pipeline():
    from minicom_amd import pipeline
    return pipeline


def _all_members(golden_dir):
    m = {"small/" + k: v for k, v in bc.small_members(golden_dir).items()}
    m.update({"block/" + k: v for k, v in bc.block_members(golden_dir).items()})
    m.update(ec.golden_members(golden_dir))
    return m


def test_encoder_bytes_equal_the_reference(pipeline, golden_dir):
    """members of one block the reference can sort (at most 2^12 bytes; the encoders write blocks of 2^20): the same member; for the
    longer ones their first 4096 bytes; and the stages of each against the reference's"""
    for name, raw in bc.small_members(golden_dir).items():
        cut = raw[:4096]
        assert pipeline.bwt_encode(cut) == bc.ref_member(cut, br.BLK_LOG2, br.ANC_LOG2), name
        if cut:
            tr, ix, ranks = pipeline.bwt_stages(cut)
            assert (tr, ix, ranks) == br.ref_stages(cut, br.BLK_LOG2, br.ANC_LOG2), name


def test_decoder_at_the_geometries_no_encoder_writes(pipeline, golden_dir):
    """the reference's members at blocks of 2^8 / 2^12 bytes and anchors every 2^4 / 2^8 bytes, block sorted and as the format's own
    choice: the host twin decodes each to the original, and so does the reference"""
    n = 0
    for label, raw, member in bc.decoder_cases(golden_dir):
        assert pipeline.bwt_decode(member) == raw, label
        n += 1
    assert n == 12 * 5 - 4                                  # (the empty member has no block-sorted form)
    raw = bc.small_members(golden_dir)["text_dif_char"]
    assert br.ref_decode(bc.ref_member(raw, 8, 4, br.BWT)) == raw


def test_round_trip_and_bound_on_every_member(pipeline, golden_dir):
    """every golden stream file and every synthetic member: back to the original, and never larger than the `.rans` member of the same
    bytes plus the `.bwt` header -- the fallback makes that hold by construction"""
    for name, raw in _all_members(golden_dir).items():
        member = pipeline.bwt_encode(raw)
        assert pipeline.bwt_decode(member) == raw, name
        assert len(member) <= len(pipeline.rans_encode(raw)) + HEADER, name
        assert len(member) <= pipeline.load_host_library().mcomh_bwt_bound(len(raw)), name


def test_block_sorting_halves_a_repetitive_member(pipeline):
    """64 repeats of 1000 uniform random bytes: the order-1 model sees about 4 successors per context (about 2 bits per byte), after block
    sorting nearly every rank is 0: the `.bwt` member must be smaller than half the `.rans` member"""
    raw = bc.compression_member()
    bwt, rans = pipeline.bwt_encode(raw), pipeline.rans_encode(raw)
    print("bwt %d bytes, rans %d bytes" % (len(bwt), len(rans)))
    assert bwt[5] == br.BWT
    assert 2 * len(bwt) < len(rans), (len(bwt), len(rans))


def test_crafted_refusals(pipeline, golden_dir):
    """one member per refusal rule: the host twin raises for each, as the reference does, and both decode the member they were made from"""
    from minicom_amd.hip import McomError
    raw, good, crafted = bc.crafted_refusals(golden_dir)
    assert pipeline.bwt_decode(good) == raw and br.ref_decode(good) == raw
    rules = set()
    for label, bad in crafted.items():
        with pytest.raises(McomError):
            pipeline.bwt_decode(bad)
            pytest.fail("the host twin accepted " + label)
        with pytest.raises(br.BwtRefused) as e:
            br.ref_decode(bad)
        rules.add(e.value.rule)
    assert rules == {"header", "embedded", "index", "walk", "chain", "crc"}


def test_container_pack_and_unpack(golden_dir, tmp_path):
    """container.pack(codec="bwt") / unpack on a fixture stream folder gives the files back; members carry .bwt"""
    import gzip
    import io
    from minicom_amd import container
    src, dst = tmp_path / "s", tmp_path / "d"
    src.mkdir()
    with gzip.open(os.path.join(golden_dir, "streams_order_stages_L100.tar.gz"), "rb") as g:
        tf = tarfile.open(fileobj=io.BytesIO(g.read()))
        for m in tf.getmembers():
            if m.isfile():
                (src / os.path.basename(m.name)).write_bytes(tf.extractfile(m).read())
    assert "bwt" in container.CODECS
    arc = str(tmp_path / "a.minicom")
    sizes = container.pack(str(src), arc, codec="bwt")
    assert all(n == "info.txt" or n.endswith(".bwt") for n in sizes) and len(sizes) > 4
    kinds = container.unpack(arc, str(dst))
    assert kinds["order"] and not kinds["paired"]
    names = sorted(os.listdir(src))
    assert sorted(os.listdir(dst)) == names
    for n in names:
        assert (dst / n).read_bytes() == (src / n).read_bytes(), n


def test_mcomz_both_kinds(pipeline, golden_dir, tmp_path):
    """mcomz e --bwt then mcomz d gives the file back; mcomz d still decodes a .rans file; a refused member leaves no output"""
    mcomz = os.path.join(BIN, "mcomz")
    raw = bc.text_member(golden_dir, 8000) * 3
    a = tmp_path / "in"; a.write_bytes(raw)
    subprocess.run([mcomz, "e", "--bwt", str(a), str(tmp_path / "m.bwt")], check=True)
    assert (tmp_path / "m.bwt").read_bytes() == pipeline.bwt_encode(raw)
    subprocess.run([mcomz, "d", str(tmp_path / "m.bwt"), str(tmp_path / "back")], check=True)
    assert (tmp_path / "back").read_bytes() == raw
    subprocess.run([mcomz, "e", str(a), str(tmp_path / "m.rans")], check=True)
    assert (tmp_path / "m.rans").read_bytes() == pipeline.rans_encode(raw)
    subprocess.run([mcomz, "d", str(tmp_path / "m.rans"), str(tmp_path / "back2")], check=True)
    assert (tmp_path / "back2").read_bytes() == raw
    _, _, crafted = bc.crafted_refusals(golden_dir)
    for label in ("anchors_do_not_chain", "wrong_raw_crc", "blk_log2_7"):
        (tmp_path / "bad").write_bytes(crafted[label])
        p = subprocess.run([mcomz, "d", str(tmp_path / "bad"), str(tmp_path / "out")], capture_output=True)
        assert p.returncode == 1 and not (tmp_path / "out").exists(), label
        assert b".bwt member" in p.stderr, label


def test_surface(pipeline):
    import minicom_amd
    assert {"mcom_bwt_bound", "mcom_bwt_encode", "mcom_bwt_decode", "mcom_test_bwt_forward", "mcom_test_bwt_mtf"} <= set(minicom_amd.ABI_SYMBOLS)
    assert {"mcomh_bwt_bound", "mcomh_bwt_encode", "mcomh_bwt_decode", "mcomh_bwt_pack_file", "mcomh_bwt_unpack_file"} <= set(pipeline.HOST_ABI_SYMBOLS)


def test_host_twin_under_the_sanitizers(golden_dir, tmp_path):
    """host/mcom_bwt.cpp as a stand-alone program built with AddressSanitizer + UBSan (`make -C minicom_amd/host fuzz_bwt`): the round
    trips of the small members, every crafted member refused, the reference's members decoded, then every truncation and 2000 bit flips
    of one of them"""
    exe = str(tmp_path / "fuzz_bwt")
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "minicom_amd", "host"), "fuzz_bwt", "FUZZ_BWT_OUT=" + exe], capture_output=True, text=True)
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    d = tmp_path / "corpus"
    d.mkdir()
    for k, (name, raw) in enumerate(bc.small_members(golden_dir).items()):
        (d / ("m%02d.raw" % k)).write_bytes(raw)
    (d / "block.raw").write_bytes(bc.block_members(golden_dir)["one_block_plus_1"])
    _, good, crafted = bc.crafted_refusals(golden_dir)
    (d / "a.good").write_bytes(good)
    for k, (label, raw, member) in enumerate(bc.decoder_cases(golden_dir)):
        (d / ("c%02d.good" % k)).write_bytes(member)
    for k, bad in enumerate(crafted.values()):
        (d / ("r%02d.bad" % k)).write_bytes(bad)
    p = subprocess.run([exe, str(d)], capture_output=True, text=True)
    assert p.returncode == 0 and "fuzz_bwt ok" in p.stdout, (p.stdout + p.stderr)[-3000:]
