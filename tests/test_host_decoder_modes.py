"""The host decoder (minicom_amd/host/mcom_decompress.cpp) over one hand-made folder of stream files per mode -- default, -p, paired end:
the decoded text, byte for byte, and the verdict on every named corruption.  The folders are a dozen reads of eight bases (the size of
tests/fuzz_reorder.cpp's streams()): counted, near-constant, N and packed reads and one contig of three members, two of them at the same
begin position and one reverse-complemented; a second variant has two stream sets.  The expectations are literals: what the decoder gave
before its three copies of the stream walk became one walker with three sinks, so that the walker answers to them.  No GPU in this file."""
import struct

import pytest

MODES = ("default", "order", "pe")


def _u32(*v):
    return struct.pack("<%dI" % len(v), *v)


def _u16(*v):
    return struct.pack("<%dH" % len(v), *v)


def folder(mode, nth=1):
    """12 reads (nth = 1) or 14 (nth = 2) of 8 bases; -p: the ids are a permutation, paired end: 6 (7) pairs"""
    f = {
        "AA.txt": b"3C\n", "TT.txt": b"0\n", "NN.txt": b"",
        "single_N.seq": b"ACGTNACG\n",
        "single.seq": bytes([0x1B, 0xE4, 0x27, 0x8D]),
        "ref.bin.0": bytes([0x1B, 0xB1, 0x4E]),
        "beg_pos.bin.0": _u32(3) + _u16(0, 0, 2),               # two members at position 0, one at 2
        "dir.bin.0": bytes([0x02]),                             # the second member is reverse-complemented
        "dif_char.txt.0": b"0\n2G\n0\n",
    }
    if nth == 2:
        f.update({"ref.bin.1": bytes([0xE4, 0x1B, 0x93]), "beg_pos.bin.1": _u32(2) + _u16(0, 3), "dir.bin.1": bytes([0x01]), "dif_char.txt.1": b"1T\n\n"})
    n = 12 if nth == 1 else 14
    if mode == "default":
        f["info.txt"] = b"8 %d\n2 1 1\n" % nth
    elif mode == "order":
        f["info.txt"] = b"8 %d\n2 1 1\n%d\n" % (nth, n)
        f.update({"allA.ids.bin": _u32(3, 4), "allT.ids.bin": _u32(10), "allN.ids.bin": _u32(0), "AA.ids.bin": _u32(5), "TT.ids.bin": _u32(1), "NN.ids.bin": b"",
                  "singleFile.ids.bin": _u32(2, 7), "Nfile.ids.bin": _u32(11),
                  "ids.bin.0": _u32(4, 2, 8),                   # 4, then a difference (same begin position): 6, then 8
                  "pe_order.txt": b"%d\n" % (n // 2)})
        if nth == 2:
            f["ids.bin.1"] = _u32(13, 12)
    else:
        f["info.txt"] = b"8 %d\n%d\n2 1 1\n" % (nth, n // 2)
        f.update({"file.bin.sp": bytes([0xAA, 0x00]), "peids.bin.sp": _u32(3, 0, 5, 1), "file.bin.0": bytes([0x06]), "peids.bin.0": _u32(4, 2)})
        if nth == 2:
            f.update({"file.bin.1": bytes([0x02]), "peids.bin.1": _u32(6)})
    return f


def padded_folder(mode):
    """L = 3 and three reads in single.seq: 9 bases in 3 bytes, so the padding of the last byte spells a fourth read (AAA)"""
    f = {"AA.txt": b"", "TT.txt": b"", "NN.txt": b"", "single_N.seq": b"", "single.seq": bytes([0x1B, 0x1E, 0x02]),
         "ref.bin.0": b"", "beg_pos.bin.0": b"", "dir.bin.0": b"", "dif_char.txt.0": b""}
    if mode == "default":
        f["info.txt"] = b"3 1\n1 0 0\n"
    elif mode == "order":
        f["info.txt"] = b"3 1\n1 0 0\n4\n"
        f.update({"allA.ids.bin": _u32(2), "allT.ids.bin": b"", "allN.ids.bin": b"", "AA.ids.bin": b"", "TT.ids.bin": b"", "NN.ids.bin": b"",
                  "singleFile.ids.bin": _u32(0, 1, 2), "Nfile.ids.bin": b"", "ids.bin.0": b""})
    else:
        f["info.txt"] = b"3 1\n2\n1 0 0\n"
        f.update({"file.bin.sp": bytes([0x0A]), "peids.bin.sp": _u32(1, 0), "file.bin.0": b"", "peids.bin.0": b""})
    return f


def decode(mode, files, tmp_path, entry=None):
    """the output file(s) as bytes (paired end: a pair of them), or None when the folder is refused"""
    from minicom_amd import McomError, pipeline
    d = tmp_path / "arch"
    d.mkdir(exist_ok=True)
    for p in d.iterdir():
        p.unlink()
    for name, data in files.items():
        (d / name).write_bytes(data)
    o1, o2 = tmp_path / "o1", tmp_path / "o2"
    for o in (o1, o2):
        if o.exists():
            o.unlink()
    try:
        if entry == "order_pe":
            n = pipeline.decompress_order_pe(str(d), str(o1), str(o2))
        elif mode == "pe":
            n = pipeline.decompress_pe(str(d), str(o1), str(o2))
        else:
            n = pipeline.decompress(str(d), str(o1), order=mode == "order")
    except McomError:
        if mode == "order":
            assert not o1.exists() and not o2.exists()          # the -p routes write after every check
        return None
    two = mode == "pe" or entry == "order_pe"
    out = (o1.read_bytes(), o2.read_bytes()) if two else o1.read_bytes()
    assert n == (out[0] if two else out).count(b"\n")
    return out


def cut(name, size):
    def edit(f):
        assert 0 <= size < len(f[name])
        f[name] = f[name][:size]
    return edit


def put(name, data):
    def edit(f):
        f[name] = data
    return edit


def drop(name):
    def edit(f):
        del f[name]
    return edit


def corruptions(mode):
    """name -> edit of folder(mode)"""
    c = {
        "short_N_line": put("single_N.seq", b"ACGTNAC\n"),
        "beg_pos_cut_in_header": cut("beg_pos.bin.0", 2),
        "beg_pos_cut_in_delta": cut("beg_pos.bin.0", 7),
        "ref_one_byte_short": cut("ref.bin.0", 2),
        "dif_char_without_last_newline": cut("dif_char.txt.0", 6),
    }
    for name in folder(mode):
        c["missing_" + name] = drop(name)
    c.pop("missing_pe_order.txt", None)                         # (no stream file: it has a case of its own below)
    if mode == "default":
        c["info_counts_more_reads"] = put("info.txt", b"8 1\n3 1 1\n")          # (no id bytes or file bits to set it against: more reads, no refusal)
    if mode == "order":
        for name in ("allA.ids.bin", "AA.ids.bin", "singleFile.ids.bin", "Nfile.ids.bin", "ids.bin.0"):
            c["one_entry_short_" + name] = cut(name, len(folder(mode)[name]) - 4)
        c["id_named_twice"] = put("allT.ids.bin", _u32(3))
        c["id_named_twice_in_contig"] = put("ids.bin.0", _u32(4, 2, 6))
        c["id_equal_n_seq"] = put("allT.ids.bin", _u32(12))
        c["id_equal_n_seq_in_contig"] = put("ids.bin.0", _u32(4, 2, 12))
        c["info_n_seq_one_more"] = put("info.txt", b"8 1\n2 1 1\n13\n")
        c["info_n_seq_beyond_id_bytes"] = put("info.txt", b"8 1\n2 1 1\n4000000000000\n")
    if mode == "pe":
        for name in ("peids.bin.sp", "peids.bin.0"):
            c["one_entry_short_" + name] = cut(name, len(folder(mode)[name]) - 4)
        c["mate_named_twice"] = put("peids.bin.0", _u32(4, 3))
        c["mate_equal_half"] = put("peids.bin.sp", _u32(3, 0, 6, 1))
        c["mate_equal_half_in_contig"] = put("peids.bin.0", _u32(6, 2))
        c["file_bits_left_is_not_half"] = put("file.bin.sp", bytes([0xAB, 0x00]))
        c["file_bits_left_is_not_half_in_contig"] = put("file.bin.0", bytes([0x02]))
        c["info_half_one_more"] = put("info.txt", b"8 1\n7\n2 1 1\n")
        c["info_half_beyond_file_bits"] = put("info.txt", b"8 1\n4000000000000\n2 1 1\n")
    return c


# ---- what the decoder gives: the text of the good folders --------------------------------------------------------------------------------
_DEFAULT_1 = b"AAAAAAAA\nAAAAAAAA\nTTTTTTTT\nNNNNNNNN\nAAACAAAA\nTTTTTTTT\nACGTNACG\nTGCAACGT\nTCGACTAG\nTGCACATG\nCATGTCCA\nCACATGGT\n"
_DEFAULT_2 = _DEFAULT_1 + b"TGCAACAT\nTTGCATAC\n"
_ORDER_1 = b"NNNNNNNN\nTTTTTTTT\nTGCAACGT\nAAAAAAAA\nTGCACATG\nAAACAAAA\nCATGTCCA\nAAAAAAAA\nCACATGGT\nTCGACTAG\nTTTTTTTT\nACGTNACG\n"
_ORDER_2 = _ORDER_1 + b"TTGCATAC\nTGCAACAT\n"
_PE_1 = (b"AAAAAAAA\nTTTTTTTT\nAAACAAAA\nACGTNACG\nTCGACTAG\nTGCACATG\n", b"NNNNNNNN\nTGCAACGT\nCACATGGT\nAAAAAAAA\nCATGTCCA\nTTTTTTTT\n")
_PE_2 = (_PE_1[0] + b"TGCAACAT\n", _PE_1[1] + b"TTGCATAC\n")
TEXT = {("default", 1): _DEFAULT_1, ("default", 2): _DEFAULT_2, ("order", 1): _ORDER_1, ("order", 2): _ORDER_2, ("pe", 1): _PE_1, ("pe", 2): _PE_2}

# the padding of single.seq's last byte: the default and the paired-end walk take floor(4 bytes / L) reads, the phantom AAA among them (the
# paired-end folder then has one read too many for its file bits); the -p walk stops, without refusing, where singleFile.ids.bin ends
PADDED = {"default": b"AAA\nTGC\nAGT\nCAG\nAAA\n", "order": b"TGC\nAGT\nAAA\nCAG\n", "pe": None}

# every corruption not named here is refused; the default mode has neither ids nor file bits to notice reads that are missing or too many
ACCEPTED = {
    ("default", "beg_pos_cut_in_header"): _DEFAULT_1[:9 * 9],
    ("default", "info_counts_more_reads"): b"AAAAAAAA\n" + _DEFAULT_1,
}


@pytest.mark.parametrize("nth", (1, 2))
@pytest.mark.parametrize("mode", MODES)
def test_decoded_text(mode, nth, tmp_path):
    assert decode(mode, folder(mode, nth), tmp_path) == TEXT[mode, nth]


@pytest.mark.parametrize("mode", MODES)
def test_padding_of_single_seq(mode, tmp_path):
    assert decode(mode, padded_folder(mode), tmp_path) == PADDED[mode]


@pytest.mark.parametrize("mode", MODES)
def test_verdict_on_every_corruption(mode, tmp_path):
    got = {}
    for name, edit in corruptions(mode).items():
        f = folder(mode)
        edit(f)
        got[name] = decode(mode, f, tmp_path)
    assert got == {name: ACCEPTED.get((mode, name)) for name in got}


def test_pe_order_txt_must_state_half_the_reads(tmp_path):
    good = folder("order")
    assert decode("order", good, tmp_path, entry="order_pe") == (_ORDER_1[:6 * 9], _ORDER_1[6 * 9:])
    for text in (b"5\n", b"7\n", b"6", b"", b"six\n"):
        assert decode("order", dict(good, **{"pe_order.txt": text}), tmp_path, entry="order_pe") is None, text
    f = dict(good)
    del f["pe_order.txt"]
    assert decode("order", f, tmp_path, entry="order_pe") is None
