"""`minicom -p -V -A` on the GPU (csrc/odd_align.hip): each device call against the rule in plain Python
(tests/odd_align_reference.py) -- hits and member bytes equal, canaries around every output --, the refusals of the device decoder in the
host twin's words, the folder call with --gpu against the host twin's bytes, and `bin/minicom -p -V -A` end to end."""
import gzip
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

import odd_align_reference as ref
import ragged_cases as rc
import test_odd_align as cpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ref.cases()
CANARY = 64


@pytest.fixture(scope="module")
def ctx():
    import minicom_amd
    return minicom_amd.Context(0)


def _dev(b):
    import torch
    a = np.frombuffer(bytes(b), dtype=np.uint8).copy()
    return torch.from_numpy(a).cuda() if a.size else torch.zeros(0, dtype=torch.uint8, device="cuda")


def _off(off):
    import torch
    return torch.tensor(off, dtype=torch.int64, device="cuda")


def _text(ctx, refs):
    return ctx.odd_text([(_dev(img), n) for img, n in refs], canary=CANARY)


def _u64(t):
    return [int(v) for v in t.cpu().numpy().view(np.uint64)]


@pytest.mark.parametrize("name,refs,reads,want", CASES, ids=ref.case_ids())
def test_device_calls_give_the_reference(ctx, name, refs, reads, want):
    from minicom_amd import pipeline
    T = ref.text_of(refs)
    t, t_bases = _text(ctx, refs)
    host_t, _ = pipeline.odd_text_host(refs)
    assert t_bases == len(T) and _u64(t) == [int(v) for v in host_t]
    idx = ctx.odd_index_build(t, t_bases)
    try:
        grid = ctx.odd_index_entries(idx, canary=CANARY).cpu().numpy().view(np.uint64)
        keys = [int(k) for k in grid[:, 0]]
        assert keys == sorted(keys)
        want_grid = sorted((sum("ACGT".index(c) << (2 * j) for j, c in enumerate(T[q:q + ref.K])), q) for q in range(0, len(T) - ref.K + 1, ref.G))
        assert sorted((int(k), int(q)) for k, q in grid) == want_grid
        off, text = ref.offsets(reads), "".join(reads).encode()
        d_text, d_off = _dev(text), _off(off)
        want_hits = ref.align_all(T, reads)
        hits = ctx.odd_align(idx, t, t_bases, d_text, d_off, canary=CANARY)
        assert _u64(hits) == want_hits
    finally:
        ctx.odd_index_free(idx)
    want_member, want_res = ref.encode(T, reads, want_hits)
    member, res = ctx.odd_align_encode(hits, t, t_bases, d_text, d_off, canary=CANARY)
    assert member.cpu().numpy().tobytes() == want_member and res.cpu().numpy().tobytes() == want_res
    if not want_member:
        return
    back, flags, why = ctx.odd_align_decode(member, t, t_bases, res, d_off, canary=CANARY)
    assert flags == 0 and why is None and back.cpu().numpy().tobytes() == text


@pytest.mark.parametrize("what", cpu.DAMAGE)
def test_device_decoder_refuses_in_the_twins_words(ctx, what):
    from minicom_amd import pipeline
    name, refs, reads, _ = next(c for c in CASES if c[0] == "mixed_301")
    T = ref.text_of(refs)
    hits = ref.align_all(T, reads)
    member, res = ref.encode(T, reads, hits)
    host_t, t_bases = pipeline.odd_text_host(refs)
    good = dict(T=T, t=host_t, t_bases=t_bases, reads=reads, hits=hits, member=member, res=res, layout=cpu.layout_of(member))
    member, res, lengths, flag = cpu.damaged(good, what)
    off = [0]
    for l in lengths:
        off.append(off[-1] + l)
    _, host_flags, host_why = pipeline.odd_align_decode_host(bytes(member), host_t, t_bases, bytes(res), off)
    t, _ = _text(ctx, refs)
    back, flags, why = ctx.odd_align_decode(_dev(member), t, t_bases, _dev(res), _off(off), canary=CANARY)
    assert back is None and flags == host_flags and flags & flag and why == host_why


def test_folder_call_on_the_gpu_gives_the_host_twins_bytes(golden_dir, tmp_path):
    from minicom_amd import pipeline
    got = {}
    for tag, device in (("host", None), ("gpu", 0)):
        d = tmp_path / tag
        cpu.odd_folder(golden_dir, d)
        got[tag] = (pipeline.odd_align_folder(str(d), device=device), {f: (d / f).read_bytes() for f in sorted(os.listdir(d))})
    assert got["gpu"] == got["host"] and got["gpu"][0][1] > 0
    e = tmp_path / "exe"
    cpu.odd_folder(golden_dir, e)
    p = subprocess.run([os.path.join(ROOT, "bin", "decompress"), "--odd-align", "--gpu", str(e)], capture_output=True, text=True)
    assert p.returncode == 0 and tuple(int(v) for v in p.stdout.split()) == got["host"][0], p.stdout + p.stderr
    assert {f: (e / f).read_bytes() for f in sorted(os.listdir(e))} == got["host"][1]
    # the GPU decoder rebuilds the odd text on the card: the records of the folder come back, and a damaged member is refused in the twin's words
    recs = cpu.odd_folder(golden_dir, tmp_path / "plain")
    out = tmp_path / "out.fastq"
    assert pipeline.decompress_fastq(str(e), str(out), device=0) == len(recs) and out.read_bytes() == rc.text_of(recs)
    cpu.folder_damage(e, recs, "same")
    p = subprocess.run([os.path.join(ROOT, "bin", "decompress"), "--fastq", "--gpu", str(e), str(tmp_path / "never.fastq")], capture_output=True, text=True)
    assert p.returncode != 0 and cpu.WORDS["same"] in p.stderr and not (tmp_path / "never.fastq").exists(), p.stdout + p.stderr


# ---- through bin/minicom --------------------------------------------------------------------------------------------------------------------
MINICOM = os.path.join(ROOT, "bin", "minicom")


def _run(args, cwd):
    return subprocess.run([MINICOM] + [str(a) for a in args], cwd=str(cwd), capture_output=True, text=True)


def _records(seed=61, n=2000, L=100):
    """2 000 reads of 100 bases from one genome at coverage 20, 30 % of them trimmed to 31 .. 99 bases"""
    from minicom_amd import synth
    reads = synth.synth_reads(seed, n, L, coverage=20)
    rng = random.Random(seed)
    lengths = [L if rng.random() >= 0.3 else rng.randrange(31, L) for _ in range(n)]
    recs = rc.make_records(seed, lengths, n_rate=0.0)
    return [(nm, reads[i].tobytes()[:len(s)], p, q) for i, (nm, s, p, q) in enumerate(recs)]


@pytest.fixture(scope="module")
def archives(tmp_path_factory):
    """X.fastq and its archives made with -p -V -Q -N -K -G, with -A (in a/) and without (in v/), every member opened"""
    import test_gpu_ragged as tgr
    d = tmp_path_factory.mktemp("odd_align_cli")
    recs = _records()
    members = {}
    for tag, flags in (("a", ["-A"]), ("v", [])):
        w = d / tag
        w.mkdir()
        (w / "X.fastq").write_bytes(rc.text_of(recs))
        p = _run(["-r", "X.fastq", "-p", "-V", "-Q", "-N", "-K", "-G"] + flags, w)
        assert p.returncode == 0 and (w / "X_comp_order.minicom").exists(), p.stdout + p.stderr
        (w / "open").mkdir()
        members[tag] = tgr._members(w / "X_comp_order.minicom", w / "open")
    return d, recs, members


def _packed_sizes(archive_path):
    import tarfile
    with tarfile.open(archive_path) as t:
        return {os.path.basename(m.name): m.size for m in t.getmembers() if m.isfile()}


def test_archive_differs_from_the_V_archive_in_the_odd_reads_only(archives):
    d, recs, members = archives
    a, v = members["a"], members["v"]
    assert "odd.aln" in a and "odd.aln" not in v
    assert sorted(set(a) - {"odd.aln", "odd.seq"}) == sorted(set(v) - {"odd.seq"})
    for name in v:
        if name != "odd.seq":
            assert a[name] == v[name], name
    odd = [s.decode() for _, s, _, _ in recs if len(s) != 100]
    assert v["odd.seq"] == "".join(odd).encode()
    # what the member says, against the rule over the archive's own contigs: T from the unpacked ref.bin.* and beg_pos.bin.* of every set
    L, nth = (int(x) for x in a["info.txt"].split()[:2])
    refs = []
    for th in range(nth):
        pos, at, bases = a["begposbin.tar/beg_pos.bin.%d" % th], 0, 0
        while at + 4 <= len(pos):
            num, = struct.unpack_from("<I", pos, at); at += 4
            if num:
                bases += sum(struct.unpack_from("<%dH" % num, pos, at)) + L
            at += 2 * num
        refs.append((a["refbin.tar/ref.bin.%d" % th], bases))
    T = ref.text_of(refs)
    member, res = ref.encode(T, odd, ref.align_all(T, odd))
    assert a["odd.aln"] == member and a.get("odd.seq", b"") == res
    sa, sv = _packed_sizes(d / "a" / "X_comp_order.minicom"), _packed_sizes(d / "v" / "X_comp_order.minicom")
    new = sa["odd.aln.rans"] + sa.get("odd.seq.rans", 0)
    print("packed odd.seq of -V: %d bytes; packed odd.aln + residual odd.seq of -V -A: %d bytes" % (sv["odd.seq.rans"], new))
    assert new < sv["odd.seq.rans"]


@pytest.mark.parametrize("flags", [[], ["-G"], ["-G", "-z"]], ids=["host", "gpu", "gpu_gz"])
def test_round_trip_gives_the_input_file_back(archives, tmp_path, flags):
    d, recs, _ = archives
    p = _run(["-d", d / "a" / "X_comp_order.minicom"] + flags, tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    out = tmp_path / ("X_comp_order_dec.fastq" + (".gz" if "-z" in flags else ""))
    got = gzip.decompress(out.read_bytes()) if "-z" in flags else out.read_bytes()
    assert got == (d / "a" / "X.fastq").read_bytes()


@pytest.mark.parametrize("mode", ["check_input", "check_changed_base", "test"])
def test_check_and_test_modes(archives, tmp_path, mode):
    """-d -c on the input: 0; on a file with one base changed in an aligned odd read: 2; -d -T: 0; nothing is left behind"""
    d, recs, members = archives
    arc = d / "a" / "X_comp_order.minicom"
    if mode == "check_input":
        p = _run(["-d", arc, "-c", d / "a" / "X.fastq"], tmp_path)
        assert p.returncode == 0 and "DIFFERENT" not in p.stdout, p.stdout + p.stderr
    elif mode == "check_changed_base":
        member = members["a"]["odd.aln"]
        odd_at = [i for i, r in enumerate(recs) if len(r[1]) != 100]
        j = next(j for j in range(len(odd_at)) if (member[64 + (j >> 3)] >> (j & 7)) & 1)      # the first aligned odd record
        nm, s, pl, q = recs[odd_at[j]]
        v = list(recs)
        v[odd_at[j]] = (nm, s[:3] + (b"A" if s[3:4] != b"A" else b"C") + s[4:], pl, q)
        (tmp_path / "check.fastq").write_bytes(rc.text_of(v))
        p = _run(["-d", arc, "-c", tmp_path / "check.fastq"], tmp_path)
        assert p.returncode == 2 and "DIFFERENT" in p.stdout, p.stdout + p.stderr
        (tmp_path / "check.fastq").unlink()
    else:
        p = _run(["-d", arc, "-T", "-G"], tmp_path)
        assert p.returncode == 0, p.stdout + p.stderr
    assert list(tmp_path.iterdir()) == []


def test_A_without_V_is_refused(tmp_path):
    (tmp_path / "X.fastq").write_bytes(rc.text_of(rc.make_records(5, [100, 100, 37, 100])))
    p = _run(["-r", "X.fastq", "-p", "-A", "-G"], tmp_path)
    assert p.returncode == 1 and "without -V" in p.stdout, p.stdout + p.stderr
    assert sorted(f.name for f in tmp_path.iterdir()) == ["X.fastq"]


def test_python_container_round_trip(tmp_path):
    from minicom_amd import container
    recs = _records(seed=67, n=600)
    fq = tmp_path / "X.fastq"
    fq.write_bytes(rc.text_of(recs))
    arc = str(tmp_path / "X.minicom")
    sizes = container.compress_fastq(str(fq), arc, order=True, ragged=True, ragged_align=True, quality=True, names=True, codec="rans")
    assert "odd.aln.rans" in sizes
    for k, device in enumerate((0, None)):
        out = tmp_path / ("out%d.fastq" % k)
        assert container.decompress_file(arc, str(out), device=device) == len(recs)
        assert out.read_bytes() == rc.text_of(recs)
    assert container.verify_file(arc, str(fq))["identical"]
