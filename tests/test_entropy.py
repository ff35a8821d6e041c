"""The built-in entropy stage on the host: the plain C++ twin of the GPU coder (host/mcom_entropy.cpp), the
`rans` codec of the container, bin/mcomz and `minicom -d` of a rans archive.  No GPU anywhere in this file; the device side and the
byte-for-byte comparison of the two are tests/test_gpu_entropy.py."""
import math
import os
import struct
import subprocess
import tarfile

import numpy as np
import pytest

import entropy_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")


def _all_members(golden_dir):
    m = {"synthetic/" + k: v for k, v in ec.synthetic_members().items()}
    m.update(ec.golden_members(golden_dir))
    return m


def test_fixture_coverage(golden_dir):
    """the members cover every kind of stream fixture: default, -p, paired end, L 40 / 100 / 150"""
    tags = {k.split("/")[0] for k in ec.golden_members(golden_dir)}
    assert {"stages_L40", "stages_L100", "stages_L150", "order_stages_L100", "order_stages_L150", "pe_stages_L100", "pe_stages_L150"} <= tags


def test_host_round_trip_and_stored_bound(golden_dir):
    """every stream file of every fixture and every synthetic member: decode(encode(x)) == x, and the member never grows by more than
    its header (stored mode)"""
    from minicom_amd import pipeline
    for name, raw in _all_members(golden_dir).items():
        member = pipeline.rans_encode(raw)
        assert pipeline.rans_decode(member) == raw, name
        assert len(member) <= len(raw) + ec.HEADER, (name, len(raw), len(member))
        assert pipeline.rans_encode(raw) == member, name                      # deterministic
    small = [v for k, v in ec.synthetic_members().items() if k in ("skewed_4_symbols", "all_equal")]
    assert all(len(pipeline.rans_encode(v)) < len(v) // 3 for v in small)     # ... and it does compress what can be compressed


def test_every_forced_model_round_trips_within_its_model_bound(golden_dir):
    """each (model, stride) through the hint; coded size <= ceil(B / 8) + 8 bytes per segment run + header + tables, B recomputed with
    numpy from the member's OWN tables.  8 = 4 bytes of final state + 2 of stored length + the rounding of the renormalisation bytes
    (the coder loses < 0.0007 bit per symbol, < 1.5 bits over a segment of 2048 bytes)."""
    from minicom_amd import pipeline
    for name, raw in _all_members(golden_dir).items():
        for model, stride in ec.MODELS:
            member = pipeline.rans_encode(raw, model=model, stride=stride)
            h, freq = ec.parse_member(member)
            assert (h["model"], h["stride"], h["raw_len"]) == (model, stride, len(raw)), name
            assert pipeline.rans_decode(member) == raw, (name, model, stride)
            if model == 0:
                assert len(member) == ec.HEADER + len(raw)
                continue
            bits = ec.model_bits(raw, h, freq)
            bound = math.ceil(bits / 8.0) + ec.RUN_OVERHEAD * h["n_seg"] + ec.HEADER + h["table_bytes"]
            assert len(member) <= bound, (name, model, stride, len(member), bound)


def test_model_choice_is_the_minimum_estimate(golden_dir):
    """the default choice is the candidate with the smallest estimated size, ties to the simpler model; the estimates are recomputed with
    numpy from each candidate's stored tables"""
    from minicom_amd import pipeline
    for name, raw in _all_members(golden_dir).items():
        est = []
        for model, stride in ec.MODELS:
            h, freq = ec.parse_member(pipeline.rans_encode(raw, model=model, stride=stride))
            est.append(ec.numpy_estimate(raw, h, freq))
        lib = pipeline.rans_estimate(raw)
        assert all(abs(a - b) <= 1 for a, b in zip(est, lib)), (name, est, lib)          # (float summation order: a byte at most)
        h, _ = ec.parse_member(pipeline.rans_encode(raw))
        chosen = ec.MODELS.index((h["model"], h["stride"]))
        assert chosen == int(np.argmin(lib)), (name, lib, chosen)
        order = np.argsort(est, kind="stable")
        if est[order[1]] - est[order[0]] > 1:
            assert chosen == int(order[0]), (name, est, chosen)
    # the members were made so that the choice is not always the same
    pick = lambda raw: ec.parse_member(pipeline.rans_encode(raw))[0]
    syn = ec.synthetic_members()
    assert pick(syn["uniform_random"])["model"] == 0 and pick(syn["one_byte"])["model"] == 0 and pick(syn["empty"])["model"] == 0
    assert pick(syn["skewed_4_symbols"])["model"] == 1 and pick(syn["words_u32"])["stride"] == 4


def test_hostile_members_are_refused_or_exact(golden_dir):
    """every truncation and 2000 seeded single-bit flips of a golden member of >= 4 KB: an error or the exact original, never a crash,
    never a wrong output with success"""
    from minicom_amd import pipeline
    from minicom_amd.hip import McomError
    name, raw = ec.pick_hostile_member(golden_dir)
    member = pipeline.rans_encode(raw)
    assert ec.parse_member(member)[0]["model"] != 0, "the hostile member should exercise the coder, not stored mode"
    refused = harmless = 0
    for label, bad in ec.hostile_corpus(member, flips=2000):
        try:
            out = pipeline.rans_decode(bad, cap=len(raw))
        except McomError:
            refused += 1
            continue
        assert out == raw, label
        harmless += 1
        assert label.startswith("flip"), label                         # a truncated member is never accepted
    assert refused >= len(member) + 1900, (refused, harmless)           # (the CRC-32 catches what the structure checks let through)


def test_hostile_corpus_under_the_sanitizers(golden_dir, tmp_path):
    """the same corpus once against the host twin built with AddressSanitizer + UBSan (`make -C minicom_amd/host fuzz_entropy`), every
    member and every output in a heap block of exactly its size.  CPU build: the GPU pool has no sanitizer runs."""
    from minicom_amd import pipeline
    exe = str(tmp_path / "fuzz_entropy")
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "minicom_amd", "host"), "fuzz_entropy", "FUZZ_OUT=" + exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    name, raw = ec.pick_hostile_member(golden_dir)
    member = pipeline.rans_encode(raw)
    (tmp_path / "raw.bin").write_bytes(raw)
    with open(tmp_path / "corpus.bin", "wb") as f:
        for _, bad in ec.hostile_corpus(member, flips=2000):
            f.write(struct.pack("<I", len(bad)) + bad)
    p = subprocess.run([exe, str(tmp_path / "raw.bin"), str(tmp_path / "corpus.bin")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "fuzz_entropy ok" in p.stdout, (p.stdout + p.stderr)[-3000:]


def _unpack_golden(golden_dir, tag, dst):
    os.makedirs(dst, exist_ok=True)
    for k, v in ec.golden_members(golden_dir).items():
        if k.split("/")[0] == tag:
            with open(os.path.join(dst, k.split("/")[1]), "wb") as f:
                f.write(v)


@pytest.mark.parametrize("tag,extra", [("stages_L100", ()), ("order_stages_L100", ("idsbin.tar",)), ("pe_stages_L100", ("peidsbin.tar", "filebin.tar")),
                                       ("stages_L40", ()), ("stages_L150", ())])
def test_container_rans_codec_restores_the_stream_files(golden_dir, tmp_path, tag, extra):
    from minicom_amd import container
    src = str(tmp_path / "src")
    _unpack_golden(golden_dir, tag, src)
    before = {n: open(os.path.join(src, n), "rb").read() for n in os.listdir(src)}
    arc = str(tmp_path / "x.minicom")
    sizes = container.pack(src, arc, codec="rans", threads=3)
    with tarfile.open(arc) as t:
        names = [m.name for m in t.getmembers()]
    want = {"info.txt"} | {g + ".rans" for g in ("refbin.tar", "dirbin.tar", "begposbin.tar", "dif_char.tar") + tuple(extra)}
    want |= {s + ".rans" for s in container.SINGLES if s in before}
    assert names[0] == "info.txt" and set(names) == want == set(sizes)
    dst = str(tmp_path / "dst")
    kinds = container.unpack(arc, dst)
    assert kinds == {"order": "idsbin.tar" in extra, "paired": "filebin.tar" in extra}
    after = {n: open(os.path.join(dst, n), "rb").read() for n in os.listdir(dst)}
    assert after == {k: v for k, v in before.items() if not k.startswith("ids.txt.")} or after == before
    with pytest.raises(ValueError):
        container.pack(src, arc, codec="zip")


def test_mcomz_round_trip_and_corrupt_member(golden_dir, tmp_path):
    name, raw = ec.pick_hostile_member(golden_dir)
    (tmp_path / "a.bin").write_bytes(raw)
    mcomz = os.path.join(BIN, "mcomz")
    p = subprocess.run([mcomz, "e", "a.bin", "a.bin.rans"], cwd=tmp_path, capture_output=True)
    assert p.returncode == 0, p.stderr
    from minicom_amd import pipeline
    assert (tmp_path / "a.bin.rans").read_bytes() == pipeline.rans_encode(raw)
    p = subprocess.run([mcomz, "d", "a.bin.rans", "back.bin"], cwd=tmp_path, capture_output=True)
    assert p.returncode == 0 and (tmp_path / "back.bin").read_bytes() == raw
    member = bytearray((tmp_path / "a.bin.rans").read_bytes())
    member[len(member) // 2] ^= 0x10
    (tmp_path / "bad.rans").write_bytes(bytes(member))
    (tmp_path / "cut.rans").write_bytes(bytes(member[:-3]))
    for bad in ("bad.rans", "cut.rans", "missing.rans"):
        p = subprocess.run([mcomz, "d", bad, "out.bin"], cwd=tmp_path, capture_output=True)
        assert p.returncode == 1 and b"mcomz:" in p.stderr, bad
        assert not (tmp_path / "out.bin").exists(), bad
    p = subprocess.run([mcomz, "x", "a", "b"], cwd=tmp_path, capture_output=True)
    assert p.returncode == 1 and b"usage" in p.stderr


def test_minicom_d_reads_a_rans_archive_without_a_gpu(golden_dir, tmp_path):
    """`minicom -d` of an archive whose members are .rans: decoded by mcomz d on the host, the fixture's reads come back"""
    import gzip
    from minicom_amd import container
    src = str(tmp_path / "streams")
    _unpack_golden(golden_dir, "stages_L100", src)
    container.pack(src, str(tmp_path / "sample_comp.minicom"), codec="rans")
    p = subprocess.run(["bash", os.path.join(BIN, "minicom"), "-d", "sample_comp.minicom", "-t", "2"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-3000:]
    with gzip.open(os.path.join(golden_dir, "stages_L100.reads.gz"), "rb") as f:
        rows = f.read().split(b"\n")[:-1]
    got = (tmp_path / "sample_comp_dec.reads").read_bytes().split(b"\n")[:-1]
    assert sorted(got) == sorted(rows)
    assert not (tmp_path / "sample_comp").exists()


def test_the_symbols_are_exported():
    import minicom_amd
    from minicom_amd import pipeline
    assert {"mcom_rans_bound", "mcom_rans_encode", "mcom_rans_decode"} <= set(minicom_amd.ABI_SYMBOLS)
    assert {"mcomh_rans_encode", "mcomh_rans_decode", "mcomh_entropy_pack_file", "mcomh_entropy_unpack_file"} <= set(pipeline.HOST_ABI_SYMBOLS)
    assert "rans" in __import__("minicom_amd.container", fromlist=["CODECS"]).CODECS


# ---- the host twin against the independent reference (tests/rans_reference.py, written from DESIGN 3.6) --------------------------------
def test_host_encode_equals_reference_encode():
    """every synthetic member x every forced (model, stride), and the default choice under the (model, stride) its header names: the
    host twin's bytes are the reference's, whose tables come from its own counts and its own normalisation"""
    from minicom_amd import pipeline
    for name, raw in ec.synthetic_members().items():
        for model, stride in ec.MODELS:
            assert pipeline.rans_encode(raw, model=model, stride=stride) == ec.ref_member(raw, model, stride), (name, model, stride)
        member = pipeline.rans_encode(raw)
        assert member == ec.ref_member(raw, member[5], member[6]), (name, "default", member[5], member[6])


@pytest.mark.parametrize("seg_log2", [8, 9, 10, 12, 15])
def test_host_decodes_reference_members_at_other_segment_sizes(seg_log2):
    """the encoders write segments of 2^11 bytes only; the decoder takes 2^8 .. 2^15.  Reference members of the six coded models at the
    other sizes (contexts cut at THAT segment size) decode on the host, and with the reference's own decoder"""
    from minicom_amd import pipeline
    import rans_reference as rr
    syn = ec.synthetic_members()
    inputs = {k: syn[k] for k in ("one_byte", "segment_plus_1", "three_segments_minus_1", "words_u32", "skewed_4_symbols")}
    inputs["exact_segment"] = ec.exact_segment(seg_log2)
    for name, raw in inputs.items():
        for model, stride in ec.CODED_MODELS:
            member = rr.ref_encode(raw, model, stride, seg_log2=seg_log2)
            assert member[7] == seg_log2
            assert pipeline.rans_decode(member) == raw, (name, model, stride)
            assert rr.ref_decode(member) == raw, (name, model, stride)


def test_one_crafted_member_per_refusal_rule():
    """a valid three-segment member of the reference, then one member per rule of DESIGN 3.6 with that rule the first thing wrong: the
    host twin and the reference's decoder accept the first and refuse every other one"""
    from minicom_amd import pipeline
    from minicom_amd.hip import McomError
    import rans_reference as rr
    raw, good, crafted = ec.crafted_refusals()
    assert pipeline.rans_decode(good) == raw and rr.ref_decode(good) == raw
    assert len(crafted) == 12
    want_rule = {"length_moved_to_neighbour": ("exhausted", "end"), "run_of_length_3": ("run<4",), "state_2^23-1": ("state",), "state_2^31": ("state",),
                 "byte_appended_to_run": ("end",), "table_row_emptied": ("slot",), "table_row_sums_to_4095": ("tables",), "wrong_crc": ("crc",)}
    for label, bad in crafted.items():
        with pytest.raises(rr.RansRefused) as e:
            rr.ref_decode(bad)
        assert e.value.rule in want_rule.get(label, ("header",)), (label, e.value.rule)         # refused for the reason it was made for
        if not label.startswith("header"):
            rr.parse_header(bad)
        with pytest.raises(McomError):
            pipeline.rans_decode(bad, cap=len(raw))


def test_worst_case_run_room():
    """a segment made only of symbols of frequency 1 (12 bits each) costs the longest run a 2048-byte segment can have: it stays within
    the room the encoders give a run, run_cap(2048) = 3080 bytes less the 4 the state takes at the end, and the member decodes"""
    from minicom_amd import pipeline
    import rans_reference as rr
    raw = ec.worst_case_raw()
    member = pipeline.rans_encode(raw, model=1, stride=1)
    h, freq = ec.parse_member(member)
    assert (h["model"], h["stride"], h["n_seg"]) == (1, 1, 104)
    assert (freq[0, 0, 1:] == 1).all() and freq[0, 0, 0] == 4096 - 255
    _, _, runs = ec.split_member(member)
    longest = max(len(r) for r in runs)
    assert longest == len(runs[100]) and longest > 2048 * 12 // 8, longest          # the rare segment, and it does cost 12 bits a symbol
    assert longest <= rr.run_cap(2048) - 4 and rr.run_cap(2048) == 3080, longest
    assert pipeline.rans_decode(member) == raw
    assert rr.ref_decode(member) == raw
