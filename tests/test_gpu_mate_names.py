"""`.mcn` kind 2 on the GPU (csrc/names.hip): mcom_name_encode_mate / mcom_name_decode_mate against the independent
reference (tests/mate_name_reference.py) and the host twin -- identical bytes, texts and mates at odd addresses, a mate whose buffer ends at
its last byte, canaries around the output, the same hostile members refused with the flag of their rule."""
import re

import numpy as np
import pytest

import mate_name_cases as mc
import mate_name_reference as MR

pytestmark = pytest.mark.gpu
CANARY = 0xA5
# the flag word's bits (csrc/name_model.hpp) by the rule the reference names, for the rules that a kernel or the mate check raises
FLAG_OF_RULE = {"no mate token": 2, "value": 4, "25th token": 8, "name above 255": 16, "mate": 256}


@pytest.fixture(scope="module")
def ctx():
    import minicom_amd
    return minicom_amd.Context(0)


def _dev(b, offset=0):
    """the bytes on the device, `offset` bytes into a fresh buffer (an odd address for offset 1 or 3)"""
    import torch
    buf = torch.full((offset + len(b) + 16,), CANARY, dtype=torch.uint8, device="cuda")
    if len(b):
        buf[offset:offset + len(b)] = torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()
    return buf[offset:offset + len(b)]


def _exact(b):
    """the bytes in an allocation of exactly their length: the buffer ends at the last byte"""
    import torch
    if not len(b):
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()


def _host(t) -> bytes:
    return t.cpu().numpy().tobytes()


def _decode_in_canary(ctx, member, mate_dev, text_len, offset=3, room=None):
    """(text or None when refused, the refusal's message, canary intact?): the member decoded `offset` bytes into a buffer of canary bytes"""
    import torch
    from minicom_amd import McomError
    room = max(text_len, 1) if room is None else room
    buf = torch.full((offset + room + 64,), CANARY, dtype=torch.uint8, device="cuda")
    try:
        got, why = _host(ctx.name_decode_mate(_dev(member, 1), mate_dev, out=buf[offset:offset + room])), ""
    except McomError as e:
        got, why = None, str(e)
    b = buf.cpu().numpy()
    intact = bool((b[:offset] == CANARY).all() and (b[offset + room:] == CANARY).all())
    if got is not None:
        intact = intact and bool((b[offset + len(got):offset + room] == CANARY).all())
    return got, why, intact


def _check_case(ctx, names, plus, mnames, mplus, tag):
    from minicom_amd import McomError, pipeline
    text, mate, n = mc.text_of(names, plus), mc.text_of(mnames, mplus), len(names)
    want = MR.ref_encode_mate(text, n, mate, pipeline.bwt_encode, pipeline.rans_encode)
    assert pipeline.name_encode(text, n, mate=mate) == want, tag
    for offset, mate_dev in ((1, _dev(mate, 3)), (3, _exact(mate)), (0, _dev(mate, 0))):
        got = _host(ctx.name_encode_mate(_dev(text, offset), n, mate_dev))
        assert got == want, (tag, offset, len(got), len(want), got[5], want[5])
    forced = MR.ref_encode_mate(text, n, mate, pipeline.bwt_encode, pipeline.rans_encode, kind=2)
    for m in (want, forced):
        for mate_dev in (_exact(mate), _dev(mate, 1)):
            back, why, intact = _decode_in_canary(ctx, m, mate_dev, len(text))
            assert back == text and intact, (tag, m[5], why)
    with pytest.raises(McomError):
        ctx.name_decode(_dev(forced, 1))                                     # no mate: kind 2 is refused, as before


@pytest.mark.parametrize("name,names,plus,mnames,mplus", mc.cases(), ids=[c[0] for c in mc.cases()])
def test_device_emits_the_reference_and_the_host_bytes(ctx, name, names, plus, mnames, mplus):
    """every case of the CPU file from odd addresses and with a mate that ends at its last byte: the reference's bytes and the host
    twin's; the device decodes the chosen member and the kind-2 member into a buffer of canary bytes without touching a byte around"""
    _check_case(ctx, names, plus, mnames, mplus, name)


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_record_counts_around_the_launch_shapes(ctx, n):
    """one wave and one workgroup of records, one less and one more; '/1' -> '/2' names, so that kind 2 is what is made"""
    from minicom_amd import pipeline
    a, b = mc.slash_pair(n, n)
    plus = mc.nc.mixed_plus(b, n)
    _check_case(ctx, b, plus, a, None, "n%d" % n)
    forced = MR.ref_encode_mate(mc.text_of(b, plus), n, mc.text_of(a), pipeline.bwt_encode, pipeline.rans_encode, kind=2)
    assert pipeline.name_decode(forced, device=0, mate=mc.text_of(a)) == mc.text_of(b, plus)


def test_five_thousand_records_all_plus_kinds(ctx):
    """5 000 records over twenty workgroups, every kind of third line with literals, names that differ from the mate in every way the op
    rule knows; pipeline.name_encode / name_decode on device 0 give the host twin's bytes and the text"""
    from minicom_amd import pipeline
    a, b = mc.illumina_pair(21, 5000)
    rng = np.random.default_rng(3)
    for i in rng.integers(0, 5000, 400):
        i = int(i)
        how = i % 5
        b[i] = [b[i].replace(b":45:", b":%d:" % (45 + i % 300)), b[i] + b"x", b[i][:20], b"other%d" % i, b""][how]
    plus = mc.nc.mixed_plus(b, 8)
    text, mate = mc.text_of(b, plus), mc.text_of(a, mc.nc.mixed_plus(a, 2))
    want = pipeline.name_encode(text, 5000, mate=mate)
    assert want[5] == 2 and want == MR.ref_encode_mate(text, 5000, mate, pipeline.bwt_encode, pipeline.rans_encode)
    assert pipeline.name_encode(text, 5000, device=0, mate=mate) == want
    assert _host(ctx.name_encode_mate(_dev(text, 1), 5000, _exact(mate))) == want
    back, why, intact = _decode_in_canary(ctx, want, _exact(mate), len(text))
    assert back == text and intact, why
    assert pipeline.name_decode(want, device=0, mate=mate) == text


def test_a_plus_text_as_long_as_the_name_keeps_its_bytes(ctx):
    """a '+' text that has the name's length without being the name is a literal: its bytes reach `ptext` on the device as on the host,
    with and without a mate (the device's count of literal bytes once came out as 0 for exactly these records)"""
    from minicom_amd import pipeline
    rng = np.random.default_rng(2)
    names = [b"r%d" % int(v) + b"r" * 40 for v in rng.integers(0, 10 ** 6, 300)]
    plus = [b"p" * len(x) if i % 3 else x if i % 2 else b"" for i, x in enumerate(names)]
    text, mate = mc.text_of(names, plus), mc.text_of(names)
    alone = pipeline.name_encode(text, 300)
    assert alone[5] == 0 and _host(ctx.name_encode(_dev(text, 1), 300)) == alone
    want = pipeline.name_encode(text, 300, mate=mate)
    assert want[5] == 2 and _host(ctx.name_encode_mate(_dev(text, 1), 300, _exact(mate))) == want
    back, why, intact = _decode_in_canary(ctx, want, _exact(mate), len(text))
    assert back == text and intact, why
    assert _host(ctx.name_decode(_dev(alone, 1))[0]) == text


def test_noncanonical_members_decode(ctx):
    for name, member, mate, text in mc.noncanonical():
        back, why, intact = _decode_in_canary(ctx, member, _exact(mate), len(text))
        assert back == text and intact, (name, why)


def test_hostile_members_are_refused_on_the_device(ctx):
    """one crafted member per refusal rule, truncations, bit flips of the member and of the mate: the device takes the host twin's
    decision for every one, names the flag of the rule, and leaves the bytes around the output alone"""
    from minicom_amd import McomError, pipeline
    text, n, mate, base = mc.small()
    rng = np.random.default_rng(5)
    mate_flips = []
    for _ in range(30):
        b = bytearray(mate); at = int(rng.integers(0, len(b))); b[at] ^= 1 << int(rng.integers(0, 8))
        mate_flips.append(bytes(b))
    members = [(name, m, mt, rule) for name, rule, m, mt in mc.crafted()] + [("cut%d" % i, m, mate, None) for i, m in enumerate(mc.truncations())] + \
              [("flip%d" % i, m, mate, None) for i, m in enumerate(mc.bit_flips(60))] + [("mate_flip%d" % i, base, mt, "mate") for i, mt in enumerate(mate_flips)]
    for name, m, mt, rule in members:
        try:
            want = pipeline.name_decode(m, mate=mt)
        except McomError:
            want = None
        assert not (rule and want is not None), name
        if len(m) < 96:
            with pytest.raises(McomError):
                ctx.name_decode_mate(_dev(m, 1), _exact(mt))
            continue
        got, why, intact = _decode_in_canary(ctx, m, _exact(mt), len(text), room=len(text) + 600)
        assert got == want and intact, (name, why)
        if rule in FLAG_OF_RULE:
            f = re.search(r"flag 0x([0-9a-f]+)", why)
            assert f and int(f.group(1), 16) == FLAG_OF_RULE[rule], (name, rule, why)


def test_refused_inputs(ctx):
    """a text the coder without a mate refuses names its record here too; a mate that is not two lines of at most 255 bytes per record
    is refused"""
    from minicom_amd import McomError
    for name, text, n, rec in mc.nc.refused_inputs():
        with pytest.raises(McomError) as e:
            ctx.name_encode_mate(_dev(text, 1), n, _exact(b"m\n\n" * n))
        if rec is not None:
            assert "record %d " % (rec + 1) in str(e.value), (name, str(e.value))
    for mate in (b"", b"a\n\n", b"a\n\nb\n\nc\n\n", b"a\n\nb\n", b"a\n\nb\n\nc", b"a\n\n" + b"n" * 256 + b"\n\n"):
        with pytest.raises(McomError):
            ctx.name_encode_mate(_dev(b"x\n\ny\n\n", 1), 2, _exact(mate))


def test_fastq_name_member_mate_on_the_device(tmp_path):
    """mcomh_fastq_name_member_mate on GPU 0 and by the host twin on two files of 2 000 records (`mcomz e --fastq-names --mate ... --gpu`):
    the same member either way, the coder's for the two name texts; files that differ in records are an error and leave no member"""
    import os
    import subprocess
    from minicom_amd import McomError, pipeline
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    a, b = mc.illumina_pair(3, 2000)
    p1, p2 = mc.nc.mixed_plus(a, 5), mc.nc.mixed_plus(b, 6)
    f1, f2 = tmp_path / "A_1.fastq", tmp_path / "A_2.fastq"
    f1.write_bytes(b"".join(b"@" + x + b"\nACGT\n+" + p + b"\nIIII\n" for x, p in zip(a, p1)))
    f2.write_bytes(b"".join(b"@" + x + b"\nACGT\n+" + p + b"\nIIII\n" for x, p in zip(b, p2)))
    assert pipeline.fastq_name_member(str(f2), str(tmp_path / "host.mcn"), mate_path=str(f1)) == 2000
    assert pipeline.fastq_name_member(str(f2), str(tmp_path / "gpu.mcn"), device=0, mate_path=str(f1)) == 2000
    want = pipeline.name_encode(mc.text_of(b, p2), 2000, mate=mc.text_of(a, p1))
    assert want[5] == 2 and (tmp_path / "gpu.mcn").read_bytes() == (tmp_path / "host.mcn").read_bytes() == want
    mcomz = os.path.join(root, "bin", "mcomz")
    p = subprocess.run([mcomz, "e", "--fastq-names", "--mate", str(f1), "--gpu", str(f2), str(tmp_path / "z.mcn")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.split() == ["2000"] and (tmp_path / "z.mcn").read_bytes() == want, p.stderr
    # the file forms on the device
    (tmp_path / "t2.txt").write_bytes(mc.text_of(b, p2)); (tmp_path / "t1.txt").write_bytes(mc.text_of(a, p1))
    assert subprocess.run([mcomz, "e", "--names", "--mate", str(tmp_path / "t1.txt"), "--gpu", str(tmp_path / "t2.txt"), str(tmp_path / "y.mcn")]).returncode == 0
    assert (tmp_path / "y.mcn").read_bytes() == want
    assert subprocess.run([mcomz, "d", "--mate", str(tmp_path / "t1.txt"), "--gpu", str(tmp_path / "y.mcn"), str(tmp_path / "back.txt")]).returncode == 0
    assert (tmp_path / "back.txt").read_bytes() == mc.text_of(b, p2)
    out = tmp_path / "never.mcn"
    (tmp_path / "short.fastq").write_bytes(b"".join(b"@" + x + b"\nACGT\n+\nIIII\n" for x in a[:1999]))
    with pytest.raises(McomError) as e:
        pipeline.fastq_name_member(str(f2), str(out), device=0, mate_path=str(tmp_path / "short.fastq"))
    assert "1999" in str(e.value) and not out.exists()
