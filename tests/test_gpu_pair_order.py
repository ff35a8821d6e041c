"""A pair of FASTQ files kept in input order: `minicom -1 A_1.fastq -2 A_2.fastq -p [-Q [-N]]`, `minicom -d` with and
without -G, `-d -c A_1.fastq -C A_2.fastq`, and container.compress_fastq_pair.  The read part is tied to the single-file -p route: the stream
files of `minicompe -p A_1 A_2` are those of `minicomsg -p` on the two files behind one another, byte for byte."""
import os
import subprocess
import tarfile

import numpy as np
import pytest

import mate_name_cases as mc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _minicom(args, cwd):
    p = subprocess.run(["bash", os.path.join(ROOT, "bin", "minicom")] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    return p.returncode, p.stdout.decode(errors="replace")


def _fastq(names, plus, reads, quals) -> bytes:
    return b"".join(b"@" + a + b"\n" + r.tobytes() + b"\n+" + p + b"\n" + q.tobytes() + b"\n" for a, p, r, q in zip(names, plus, reads, quals))


def _pair(n, L, seed):
    """2 x n reads of L bases from a small genome, reads with an N, all-A reads and an all-N read among them in both files;
    Illumina-style names ` 1:` / ` 2:` and mixed '+' lines; (names1, plus1, reads1, quals1, names2, plus2, reads2, quals2)"""
    import qual_cases as qc
    from minicom_amd import synth
    reads = synth.synth_reads(seed, 2 * n, L)
    r1, r2 = reads[:n].copy(), reads[n:].copy()
    rng = np.random.default_rng(seed)
    for r in (r1, r2):
        for i in rng.integers(0, n, 12):
            r[int(i), int(rng.integers(0, L))] = ord("N")
        for i in rng.integers(0, n, 5):
            r[int(i), :] = ord("A")
        r[int(rng.integers(0, n)), :] = ord("N")
    q = qc.synth_quals(seed + 1, 2 * n, L)
    a, b = mc.illumina_pair(seed + 2, n)
    return a, mc.nc.mixed_plus(a, seed), r1, q[:n], b, mc.nc.mixed_plus(b, seed + 3), r2, q[n:]


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """2 x 3000 reads of 100 bases as A_1.fastq / A_2.fastq, and `minicom -1 A_1.fastq -2 A_2.fastq -p -Q -N -G -t 2`"""
    d = tmp_path_factory.mktemp("pair_order")
    P = _pair(3000, 100, 31)
    f1, f2 = _fastq(*P[:4]), _fastq(*P[4:])
    (d / "A_1.fastq").write_bytes(f1); (d / "A_2.fastq").write_bytes(f2)
    rc, out = _minicom(["-1", "A_1.fastq", "-2", "A_2.fastq", "-p", "-Q", "-N", "-G", "-t", "2"], d)
    assert rc == 0, out[-3000:]
    return d, P, f1, f2


def test_stream_files_are_those_of_the_single_file_route(pair, tmp_path):
    """`minicompe -p A_1 A_2` against `minicomsg -p` on `cat A_1 A_2`: the same stream files byte for byte, beside pe_order.txt; an odd
    total is refused"""
    d, P, f1, f2 = pair
    (tmp_path / "cat.fastq").write_bytes(f1 + f2)
    (tmp_path / "pe").mkdir(); (tmp_path / "sg").mkdir()
    a = subprocess.run([os.path.join(ROOT, "bin", "minicompe"), str(d / "A_1.fastq"), str(d / "A_2.fastq"), str(tmp_path / "pe"), "-p", "-t", "2"], capture_output=True, text=True)
    b = subprocess.run([os.path.join(ROOT, "bin", "minicomsg"), str(tmp_path / "cat.fastq"), str(tmp_path / "sg"), "-p", "-t", "2"], capture_output=True, text=True)
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    pe, sg = sorted(os.listdir(tmp_path / "pe")), sorted(os.listdir(tmp_path / "sg"))
    assert pe == sorted(sg + ["pe_order.txt"]) and len(sg) > 8
    for name in sg:
        assert (tmp_path / "pe" / name).read_bytes() == (tmp_path / "sg" / name).read_bytes(), name
    assert (tmp_path / "pe" / "pe_order.txt").read_bytes() == b"3000\n"
    (tmp_path / "odd.fastq").write_bytes(_fastq(P[4][:-1], P[5][:-1], P[6][:-1], P[7][:-1]))           # 2999 records
    (tmp_path / "no").mkdir()
    c = subprocess.run([os.path.join(ROOT, "bin", "minicompe"), str(d / "A_1.fastq"), str(tmp_path / "odd.fastq"), str(tmp_path / "no"), "-p"], capture_output=True, text=True)
    assert c.returncode == 1 and not (tmp_path / "no" / "pe_order.txt").exists()


def test_round_trip_gives_both_input_files_back(pair, tmp_path):
    """-d with and without -G: _dec_1.fastq and _dec_2.fastq are the two inputs byte for byte; the archive carries the marker, two quality
    members and two name members, the second of kind 2"""
    d, P, f1, f2 = pair
    arc = d / "A_comp_pe_order.minicom"
    with tarfile.open(arc) as t:
        names = {os.path.basename(m.name) for m in t.getmembers()}
        assert {"pe_order.txt", "qual_1.mcq", "qual_2.mcq", "name_1.mcn", "name_2.mcn"} <= names and "name.mcn" not in names
        by_name = {os.path.basename(m.name): m for m in t.getmembers()}
        n1, n2 = (t.extractfile(by_name[k]).read() for k in ("name_1.mcn", "name_2.mcn"))
    assert n1[5] in (0, 1) and n2[5] == 2 and len(n2) < len(n1)
    for flags in (["-G"], []):
        (tmp_path / "A_comp_pe_order.minicom").write_bytes(arc.read_bytes())
        rc, out = _minicom(["-d", "A_comp_pe_order.minicom"] + flags, tmp_path)
        assert rc == 0, out[-3000:]
        assert (tmp_path / "A_comp_pe_order_dec_1.fastq").read_bytes() == f1, flags
        assert (tmp_path / "A_comp_pe_order_dec_2.fastq").read_bytes() == f2, flags
        for k in (1, 2):
            (tmp_path / ("A_comp_pe_order_dec_%d.fastq" % k)).unlink()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["A_comp_pe_order.minicom"]


def test_without_N_and_without_Q(pair, tmp_path):
    """-p -Q alone: records `@<j+1>` with a bare '+' in both files, the right reads and qualities; -p alone: the two .reads files in input order;
    host and GPU routes agree"""
    import qual_cases as qc
    d, P, f1, f2 = pair
    for k in (1, 2):
        (tmp_path / ("A_%d.fastq" % k)).write_bytes((f1, f2)[k - 1])
    rc, out = _minicom(["-1", "A_1.fastq", "-2", "A_2.fastq", "-p", "-Q", "-G", "-t", "2"], tmp_path)
    assert rc == 0, out[-3000:]
    with tarfile.open(tmp_path / "A_comp_pe_order.minicom") as t:
        assert not [m.name for m in t.getmembers() if m.name.endswith(".mcn")]
    for flags in (["-G"], []):
        rc, out = _minicom(["-d", "A_comp_pe_order.minicom"] + flags, tmp_path)
        assert rc == 0, out[-3000:]
        assert (tmp_path / "A_comp_pe_order_dec_1.fastq").read_bytes() == qc.fastq_bytes(P[2], P[3]), flags
        assert (tmp_path / "A_comp_pe_order_dec_2.fastq").read_bytes() == qc.fastq_bytes(P[6], P[7]), flags
    (tmp_path / "A_comp_pe_order.minicom").unlink()
    rc, out = _minicom(["-1", "A_1.fastq", "-2", "A_2.fastq", "-p", "-t", "2"], tmp_path)
    assert rc == 0, out[-3000:]
    for flags in (["-G"], []):
        rc, out = _minicom(["-d", "A_comp_pe_order.minicom"] + flags, tmp_path)
        assert rc == 0, out[-3000:]
        assert (tmp_path / "A_comp_pe_order_dec_1.reads").read_bytes() == b"".join(r.tobytes() + b"\n" for r in P[2]), flags
        assert (tmp_path / "A_comp_pe_order_dec_2.reads").read_bytes() == b"".join(r.tobytes() + b"\n" for r in P[6]), flags


def test_verify(pair, tmp_path):
    """-d -c A_1.fastq -C A_2.fastq: 0; 2 after exchanging the quality lines of two records of file 2, after changing one name in file 2, after
    exchanging two records of file 1; 1 with name_1.mcn taken out of the archive, which does not decode either; nothing is left behind"""
    d, P, f1, f2 = pair
    a1, p1, r1, q1, a2, p2, r2, q2 = P
    (tmp_path / "a.minicom").write_bytes((d / "A_comp_pe_order.minicom").read_bytes())
    rc, out = _minicom(["-d", "a.minicom", "-c", str(d / "A_1.fastq"), "-C", str(d / "A_2.fastq")], tmp_path)
    assert rc == 0 and out.count("identical") == 5, out[-3000:]
    qs = q2.copy(); qs[[700, 701]] = qs[[701, 700]]
    assert not np.array_equal(qs[700], q2[700])
    (tmp_path / "qual.fastq").write_bytes(_fastq(a2, p2, r2, qs))
    an = list(a2); an[1234] = an[1234][:-1] + b"X"
    (tmp_path / "name.fastq").write_bytes(_fastq(an, p2, r2, q2))
    order = list(range(3000)); order[10], order[2000] = order[2000], order[10]
    assert not np.array_equal(r1[10], r1[2000])
    (tmp_path / "swap.fastq").write_bytes(_fastq([a1[i] for i in order], [p1[i] for i in order], r1[order], q1[order]))
    for f_1, f_2, what in ((str(d / "A_1.fastq"), "qual.fastq", "quality lines of file 2"), (str(d / "A_1.fastq"), "name.fastq", "names and '+' lines of file 2"),
                           ("swap.fastq", str(d / "A_2.fastq"), "reads of both files")):
        rc, out = _minicom(["-d", "a.minicom", "-c", f_1, "-C", f_2], tmp_path)
        assert rc == 2 and "DIFFERENT: " + what in out, (what, rc, out[-2000:])
    with tarfile.open(tmp_path / "a.minicom") as t, tarfile.open(tmp_path / "b.minicom", "w", format=tarfile.GNU_FORMAT) as o:
        for m in t.getmembers():
            if m.isfile() and os.path.basename(m.name) != "name_1.mcn":
                o.addfile(m, t.extractfile(m))
    rc, out = _minicom(["-d", "b.minicom", "-c", str(d / "A_1.fastq"), "-C", str(d / "A_2.fastq")], tmp_path)
    assert rc == 1, out[-2000:]
    rc, out = _minicom(["-d", "b.minicom"], tmp_path)
    assert rc == 1, out[-2000:]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a.minicom", "b.minicom", "name.fastq", "qual.fastq", "swap.fastq"]


def test_python_route(pair, tmp_path):
    """container.compress_fastq_pair -> unpack -> decompress_file (host and GPU) -> verify_file"""
    from minicom_amd import container
    d, P, f1, f2 = pair
    arc = str(tmp_path / "c.minicom")
    sizes = container.compress_fastq_pair(str(d / "A_1.fastq"), str(d / "A_2.fastq"), arc, quality=True, names=True, codec="rans", device=0, threads=2)
    assert sizes["n_pairs"] == 3000 and sizes["pe_order.txt"] == 5 and sizes["name_2.mcn"] < sizes["name_1.mcn"]
    kinds = container.unpack(arc, str(tmp_path / "u"))
    assert kinds == {"order": True, "paired": False, "pair_order": True, "quality": True, "names": True}
    for dev in (0, None):
        assert container.decompress_file(arc, str(tmp_path / "o1.fastq"), str(tmp_path / "o2.fastq"), device=dev) == 3000
        assert (tmp_path / "o1.fastq").read_bytes() == f1 and (tmp_path / "o2.fastq").read_bytes() == f2, dev
    rep = container.verify_file(arc, str(d / "A_1.fastq"), str(d / "A_2.fastq"))
    assert rep["identical"] and set(rep) == {"identical", "reads", "quality_1", "quality_2", "names_1", "names_2"} and rep["reads"]["n_input"] == 6000
    rep = container.verify_file(arc, str(d / "A_2.fastq"), str(d / "A_1.fastq"))
    assert not rep["identical"] and not rep["names_1"]["identical"] and rep["names_1"]["differing"] == 3000
    with pytest.raises(ValueError):
        container.compress_fastq_pair(str(d / "A_1.fastq"), str(d / "A_2.fastq"), str(tmp_path / "never.minicom"), names=True, quality=False)
    assert not (tmp_path / "never.minicom").exists()


@pytest.mark.parametrize("L", [37, 256])
def test_edge_lengths(tmp_path, L):
    """2 x 300 reads of 37 and of 256 bases through -p -Q -N -G and back, on both decode routes"""
    P = _pair(300, L, 7 + L)
    f1, f2 = _fastq(*P[:4]), _fastq(*P[4:])
    (tmp_path / "B_1.fastq").write_bytes(f1); (tmp_path / "B_2.fastq").write_bytes(f2)
    rc, out = _minicom(["-1", "B_1.fastq", "-2", "B_2.fastq", "-p", "-Q", "-N", "-G", "-t", "2"], tmp_path)
    assert rc == 0, out[-3000:]
    for flags in (["-G"], []):
        rc, out = _minicom(["-d", "B_comp_pe_order.minicom"] + flags, tmp_path)
        assert rc == 0, out[-3000:]
        assert (tmp_path / "B_comp_pe_order_dec_1.fastq").read_bytes() == f1 and (tmp_path / "B_comp_pe_order_dec_2.fastq").read_bytes() == f2, (L, flags)
