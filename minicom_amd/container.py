"""The `.minicom` container: what the reference's `minicom` script does with the stream files after the binary has
written them (reference minicom:110-172 single end, :232-293 paired end, :304-403 the way back).

The reference groups the per-thread streams into inner tars (`refbin.tar`, `dirbin.tar`, `begposbin.tar`,
`dif_char.tar`, with `-p` `idsbin.tar`, paired end `peidsbin.tar` and `filebin.tar`), runs every inner tar and the
five single files through the external `bsc` (7z for `peidsbin.tar`) and tars the results together with `info.txt`.
Those binaries are fetched over the network by the reference's `install.sh` and do not exist here, so the entropy
stage is built in: every member goes through one of the codecs below and carries its codec as file extension.
`codec="bsc"` runs a `bsc` binary found on PATH with the reference's flags and then produces the reference's own
member names; everything else about the layout is the reference's, so an archive written with `bsc` present is
what the reference's script unpacks.

`codec="rans"` is the project's own entropy stage: a static rANS coder whose host twin and GPU kernels emit the
same bytes.  With `device=None` the members are coded by the host twin, with an integer by that GPU (libmcom_hip.so through
libmcom_host.so); every other codec is packaging on the host.  The stream files themselves are the parity boundary
(tests/test_streams.py compares them byte for byte with the reference's).

`codec="bwt"` is the block-sorting coder on top of it (Burrows-Wheeler transform per 1 MiB block, move-to-front,
the ranks as a `.rans` member), with the same two routes and the same meaning of `device`.
"""
import bz2
import glob
import io
import lzma
import os
import shutil
import subprocess
import tarfile
import zlib
from concurrent.futures import ThreadPoolExecutor

# inner tar -> the stream files it takes (shell patterns of the reference script)
GROUPS = (
    ("idsbin", ("ids.bin.*", "*.ids.bin")),          # minicom:110-118, only with -p
    ("dif_char", ("dif_char.txt.*",)),               # :121-124
    ("begposbin", ("beg_pos.bin.*",)),               # :126-129
    ("peidsbin", ("peids.bin.*",)),                  # :243-247, paired end only
    ("refbin", ("ref.bin.*",)),                      # :131-134
    ("dirbin", ("dir.bin.*",)),                      # :139-142
    ("filebin", ("file.bin.*",)),                    # :259-262, paired end only
)
SINGLES = ("single_N.seq", "single.seq", "AA.txt", "TT.txt", "NN.txt")      # :136-137, :144-146
NAME_MEMBER = "name.mcn"          # read names and '+' texts of a -p -Q archive: stored as it is
REORDERED_MEMBERS = ("rqual.mcq", "rqual_1.mcq", "rqual_2.mcq")     # quality values in the archive's own order
READ_ORDER = "read_order.bin"     # temporary of compress_fastq(quality_reordered=True): never a member
PAIR_ORDER = "pe_order.txt"       # marks a pair kept in input order: one line, the number of pairs; stored as it is
PAIR_MEMBERS = ("qual_1.mcq", "qual_2.mcq", "name_1.mcn", "name_2.mcn")     # its quality values and names, file by file; name_2 is coded against name_1
LOSSY_MARKER = "qual_lossy.txt"   # marks quality values stored with bounded loss: the canonical spec and a newline; stored as it is
RAGGED_MEMBERS = ("len.bin", "odd.seq", "odd.qual")   # reads of differing lengths: through the codec like the singles; len.bin marks the archive
ODD_ALIGN_MEMBER = "odd.aln"      # odd reads coded against the contigs: through the codec like odd.seq, which then holds the others
AGREE_MARKER = "qual_agree.txt"   # marks quality values of agreeing bases stored as one Phred value: `Q C` and a newline; stored as it is
DIGEST_MEMBER = "digest.txt"      # the digest of the input of an archive made with digest=True (`minicom -K`): plain text, stored as it is
QUALITY_MEMBER = "qual.mcq"       # quality values of a -p archive: coded by its own coder, stored as it is
CODECS = ("xz", "bz2", "gz", "raw", "bsc", "rans", "bwt")


def _encode(data: bytes, codec: str) -> bytes:
    if codec == "xz":
        return lzma.compress(data, preset=6)
    if codec == "bz2":
        return bz2.compress(data, 9)
    if codec == "gz":
        return zlib.compress(data, 6)
    if codec == "raw":
        return data
    raise ValueError("unknown codec " + codec)


def _decode(data: bytes, codec: str) -> bytes:
    if codec == "xz":
        return lzma.decompress(data)
    if codec == "bz2":
        return bz2.decompress(data)
    if codec == "gz":
        return zlib.decompress(data)
    if codec == "raw":
        return data
    raise ValueError("unknown codec " + codec)


def _bsc(args, src: bytes, tmpdir: str, tag: str) -> bytes:
    exe = shutil.which("bsc")
    if not exe:
        raise RuntimeError("codec 'bsc' needs a bsc binary on PATH (the reference's install.sh fetches one)")
    a, b = os.path.join(tmpdir, tag + ".in"), os.path.join(tmpdir, tag + ".out")
    with open(a, "wb") as f:
        f.write(src)
    subprocess.run([exe, args[0], a, b] + list(args[1:]), check=True, stdout=subprocess.DEVNULL)
    with open(b, "rb") as f:
        out = f.read()
    os.remove(a); os.remove(b)
    return out


def _rans(data: bytes, pack_it: bool, device, tmpdir: str, tag: str, codec: str = "rans") -> bytes:
    """One member through the built-in entropy stage: the host twin on the bytes, or -- device given -- the file route on that GPU."""
    from . import pipeline
    if device is None and codec == "bwt":
        return pipeline.bwt_encode(data) if pack_it else pipeline.bwt_decode(data)
    if device is None:
        return pipeline.rans_encode(data) if pack_it else pipeline.rans_decode(data)
    a, b = os.path.join(tmpdir, tag + ".rin"), os.path.join(tmpdir, tag + ".rout")
    with open(a, "wb") as f:
        f.write(data)
    try:
        pipeline.entropy_file(a, b, pack_it, device, codec=codec)
        with open(b, "rb") as f:
            return f.read()
    finally:
        for p in (a, b):
            if os.path.exists(p):
                os.remove(p)


def _inner_tar(folder: str, names) -> bytes:
    """`tar -cf X.tar -C X .` of the reference: plain member names, sorted for a reproducible archive."""
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.GNU_FORMAT) as t:
        for n in sorted(names):
            ti = tarfile.TarInfo(n)
            ti.size = os.path.getsize(os.path.join(folder, n))
            ti.mode = 0o644
            with open(os.path.join(folder, n), "rb") as f:
                t.addfile(ti, f)
    return buf.getvalue()


def pack(folder: str, out_path: str, codec: str = "xz", threads: int = 8, device: int | None = None) -> dict:
    """Stream files in `folder` (as cluster_dump left them) -> one `.minicom` file.  Returns the member sizes.
    device (codecs "rans" and "bwt" only): None = the host twin, an integer = that GPU, one member at a time."""
    if codec not in CODECS:
        raise ValueError("codec must be one of %s" % (CODECS,))
    if not os.path.isfile(os.path.join(folder, "info.txt")):
        raise FileNotFoundError("no info.txt in %s: not a stream directory" % folder)
    members = []                                         # (name without codec extension, bytes)
    for group, patterns in GROUPS:
        names = sorted({os.path.basename(p) for pat in patterns for p in glob.glob(os.path.join(folder, pat))})
        if names:
            members.append((group + ".tar", _inner_tar(folder, names)))
    for s in SINGLES + RAGGED_MEMBERS + (ODD_ALIGN_MEMBER,):
        p = os.path.join(folder, s)
        if os.path.isfile(p):
            with open(p, "rb") as f:
                members.append((s, f.read()))
    ext = codec

    def enc(item):
        name, data = item
        if codec == "bsc":                               # minicom:115 etc.: bsc e IN OUT -b64p -tN -e2
            return name + ".bsc", _bsc(("e", "-b64p", "-t%d" % threads, "-e2"), data, folder, name)
        if codec == "rans":
            return name + ".rans", _rans(data, True, device, folder, name)
        if codec == "bwt":
            return name + ".bwt", _rans(data, True, device, folder, name, codec="bwt")
        return name + "." + ext, _encode(data, codec)

    with ThreadPoolExecutor(max(1, threads) if device is None else 1) as ex:
        packed = list(ex.map(enc, members))
    if os.path.isfile(os.path.join(folder, QUALITY_MEMBER)):     # coded already: stored as it is, no codec on top
        with open(os.path.join(folder, QUALITY_MEMBER), "rb") as f:
            packed.append((QUALITY_MEMBER, f.read()))
    if os.path.isfile(os.path.join(folder, NAME_MEMBER)):        # likewise (section 3.10)
        with open(os.path.join(folder, NAME_MEMBER), "rb") as f:
            packed.append((NAME_MEMBER, f.read()))
    for m in REORDERED_MEMBERS + (PAIR_ORDER,) + PAIR_MEMBERS + (LOSSY_MARKER, AGREE_MARKER, DIGEST_MEMBER):   # likewise (sections 3.11, 3.12, 3.13, 3.17 and 3.18)
        if os.path.isfile(os.path.join(folder, m)):
            with open(os.path.join(folder, m), "rb") as f:
                packed.append((m, f.read()))
    sizes = {}
    with tarfile.open(out_path, mode="w", format=tarfile.GNU_FORMAT) as t:
        with open(os.path.join(folder, "info.txt"), "rb") as f:
            info = f.read()
        for name, data in [("info.txt", info)] + packed:
            ti = tarfile.TarInfo(name)
            ti.size = len(data)
            ti.mode = 0o644
            t.addfile(ti, io.BytesIO(data))
            sizes[name] = len(data)
    return sizes


def unpack(path: str, folder: str, threads: int = 8, device: int | None = None) -> dict:
    """`.minicom` file -> the stream files in `folder` (created if absent).  Returns what the archive says about itself:
    {"order": bool, "paired": bool} as the reference's script decides them (minicom:326-334), and "quality": True for an archive
    that carries quality values (the member qual.mcq, left in the folder as it is), "quality_reordered": True for one that carries them
    in its own order (rqual.mcq, or rqual_1.mcq and rqual_2.mcq), "pair_order": True for a pair kept in input order (pe_order.txt; then
    "quality" / "names" speak of qual_1.mcq + qual_2.mcq / name_1.mcn + name_2.mcn), "ragged": True for an archive of reads of differing
    lengths (len.bin), "quality_lossy": the text of qual_lossy.txt for
    an archive whose quality values went through a lossy transform (the file is left in the folder, where the
    verifiers look for it), "quality_agree": the text of qual_agree.txt (`Q C`) for an archive made with quality_agree (section 3.17).
    device: where `.rans` and `.bwt` members are decoded -- None = the host twin, an integer = that GPU."""
    os.makedirs(folder, exist_ok=True)
    with tarfile.open(path, mode="r") as t:
        items = [(m.name.lstrip("./"), t.extractfile(m).read()) for m in t.getmembers() if m.isfile()]
    kinds = {"order": False, "paired": False}

    def dec(item):
        name, data = item
        if name == "info.txt" or name == QUALITY_MEMBER or name == NAME_MEMBER or name in REORDERED_MEMBERS or name == PAIR_ORDER or name in PAIR_MEMBERS or name == LOSSY_MARKER or name == AGREE_MARKER or name == DIGEST_MEMBER:
            return name, data
        base, ext = name.rsplit(".", 1)
        if ext == "bsc":
            return base, _bsc(("d", "-t%d" % threads), data, folder, base)
        if ext == "7z":
            raise RuntimeError("member %s needs 7z; archives written here use one codec for every member" % name)
        if ext == "rans":
            return base, _rans(data, False, device, folder, base)
        if ext == "bwt":
            return base, _rans(data, False, device, folder, base, codec="bwt")
        return base, _decode(data, ext)

    with ThreadPoolExecutor(max(1, threads) if device is None else 1) as ex:
        plain = list(ex.map(dec, items))
    for name, data in plain:
        if name == QUALITY_MEMBER:
            kinds["quality"] = True
        if name == NAME_MEMBER:
            kinds["names"] = True
        if name in REORDERED_MEMBERS:
            kinds["quality_reordered"] = True
        if name == PAIR_ORDER:
            kinds["pair_order"] = True
        if name == RAGGED_MEMBERS[0]:
            kinds["ragged"] = True
        if name == LOSSY_MARKER:
            kinds["quality_lossy"] = data.decode("latin-1").rstrip("\n")      # (as stored: the verifiers judge whether it is a spec)
        if name == AGREE_MARKER:
            kinds["quality_agree"] = data.decode("latin-1").rstrip("\n")     # (as stored, `Q C`: the verifiers judge whether it parses)
        if name == DIGEST_MEMBER:
            kinds["digest"] = True
        if name in PAIR_MEMBERS:
            kinds["quality" if name.endswith(".mcq") else "names"] = True
        if name.startswith("idsbin.tar"):
            kinds["order"] = True
        if name.startswith("filebin.tar"):
            kinds["paired"] = True
        if name.endswith(".tar"):
            with tarfile.open(fileobj=io.BytesIO(data), mode="r") as t:
                for m in t.getmembers():
                    if m.isfile():
                        n = os.path.basename(m.name)
                        with open(os.path.join(folder, n), "wb") as f:
                            f.write(t.extractfile(m).read())
        else:
            with open(os.path.join(folder, name), "wb") as f:
                f.write(data)
    return kinds


# ---- end to end: what `minicom -r IN [-p]`, `minicom -1 IN1 -2 IN2` and `minicom -d X.minicom` amount to -------------
def compress_fastq(path: str, out_path: str, path2: str | None = None, order: bool = False, codec: str = "xz",
                   device: int = 0, threads: int = 8, quality: bool = False, names: bool = False, quality_reordered: bool = False,
                   quality_lossy=None, ragged: bool = False, quality_agree=None, digest: bool = False, ragged_align: bool = False, **params) -> dict:
    """FASTQ/FASTA (plain or .gz; path2 = the mates' file) -> `.minicom`.  The hot path runs on `device` (there is no CPU
    fallback), the stream writer and the packaging on the host -- except the codecs "rans" and "bwt", whose members are coded on `device` too.
    quality=True (`minicom -Q`; needs order=True and no path2, because only the -p archive keeps the order that says which quality row
    belongs to which read): the quality lines are gathered and coded on `device` and travel as the member qual.mcq.  Read names and the
    text of the `+` line are not kept, unless names=True (`minicom -N`; needs order=True and quality=True): they travel as the member
    name.mcn, coded on `device`, and decompress_file then gives the input file back byte for byte.
    quality_reordered=True (`minicom -q`; not with order, quality or names; allowed with path2): the quality rows are put into the archive's
    own order on `device` and travel as rqual.mcq (rqual_1.mcq and rqual_2.mcq for a pair); decompress_file gives four-line records in that
    order, named by their row.
    quality_lossy (`minicom -b SPEC`; needs quality or quality_reordered): a lossy spec (`ill8`, `thr:T:LO:HI`,
    `pblock:P`); the quality rows go through mcom_qual_transform on `device` in front of the coder, and the archive says so in
    qual_lossy.txt.
    quality_agree (`minicom -a Q[:C]`; needs order=True and quality=True, or quality_reordered=True without path2; not with ragged): (Q, C) or Q alone (C = 3);
    the quality value of every base that agrees with its contig's consensus at a place at least C member reads cover is stored as Phred Q.
    The mask is made on `device` from the stream files just dumped; the archive says so in qual_agree.txt.  With quality_lossy: agreement first.
    ragged=True (`minicom -p -V`; needs order=True; not with path2, quality_reordered or quality_lossy): the
    reads may differ in length.  Those of the modal length are the archive's reads, the others travel in len.bin, odd.seq and odd.qual;
    a file of one length gives the archive made without it.
    ragged_align=True (`minicom -p -V -A`; needs ragged=True): the reads of another length are searched for in the
    contigs on `device`; those found travel in odd.aln as a place and their differences, odd.seq keeps the others.  Where none is found
    the archive is the one made with ragged alone.
    digest=True (`minicom -K`; every mode): one more pass over the input on `device` stores its digest as
    digest.txt (without the quality keys beside quality_lossy or quality_agree); decompress_file then checks what it wrote against it, and
    test_file tests the archive.  Without it the archive does not change.  Returns pack()'s member sizes plus the read count (with ragged: "n_reads"
    counts the reads of the modal length, "n_records" all)."""
    import tempfile
    from .hip import McomError
    from .pipeline import Pipeline
    lossy = _lossy_spec(quality_lossy, quality or quality_reordered)
    agree = _agree_spec(quality_agree, ((quality and order) or (quality_reordered and path2 is None)) and not ragged)
    if order and path2 is not None:
        raise ValueError("-p is a single-end option (reference minicom:439-476)")
    if quality and (not order or path2 is not None):
        raise ValueError("quality values are kept by the order-preserving single-end mode only (order=True, no path2)")
    if names and not (order and quality):
        raise ValueError("names are kept beside the quality values of an order-preserving archive only (order=True, quality=True)")
    if quality_reordered and (order or quality or names):
        raise ValueError("quality_reordered keeps the quality values in the archive's own order: not with order, quality or names")
    if ragged and (not order or path2 is not None or quality_reordered or lossy is not None):
        raise ValueError("ragged keeps reads of differing lengths of one file in its input order: order=True, no path2, no quality_reordered, no quality_lossy")
    if ragged_align and not ragged:
        raise ValueError("ragged_align codes the reads of another length that ragged keeps against the contigs: without ragged=True there are none")
    if ragged:
        with tempfile.TemporaryDirectory(dir=os.path.dirname(os.path.abspath(out_path)) or ".") as td:
            sizes = _compress_ragged(path, out_path, td, codec, device, threads, quality, names, params, digest, ragged_align)
        if sizes is not None:
            return sizes                                             # (None: one length after all -- on as without ragged)
    p = Pipeline.from_fastq(path, device=device, path2=path2, host_threads=threads, **params)
    try:
        p.pre_process()
        with tempfile.TemporaryDirectory(dir=os.path.dirname(os.path.abspath(out_path)) or ".") as td:
            if quality_reordered:
                p.keep_read_order(True)
            p.cluster_dump(td, order=order, paired=path2 is not None)
            if quality_reordered:
                from .pipeline import fastq_quality_member
                order_path = os.path.join(td, READ_ORDER)
                mask_path = os.path.join(td, "agree.mask")              # a temporary like the order: never a member
                if agree is not None:
                    from .pipeline import agree_mask, fastq_quality_member_agree
                    agree_mask(td, agree[1], device=device, out_path=mask_path)
                for fq, member in ((path, "rqual.mcq"),) if path2 is None else ((path, "rqual_1.mcq"), (path2, "rqual_2.mcq")):
                    if agree is not None:
                        fastq_quality_member_agree(fq, p.L, os.path.join(td, member), mask_path, agree[0], device=device, order_path=order_path, lossy=lossy)
                    else:
                        fastq_quality_member(fq, p.L, os.path.join(td, member), device=device, order_path=order_path, lossy=lossy)
                os.remove(order_path)
                if agree is not None:
                    os.remove(mask_path)
            mask = _agree_mask(td, agree, device) if quality else None
            if quality:
                _quality_member(path, p.n, p.L, device, os.path.join(td, QUALITY_MEMBER), lossy, agree, mask, 0)
            if names:
                from .pipeline import fastq_name_member
                n_names = fastq_name_member(path, os.path.join(td, NAME_MEMBER), device=device)
                if n_names != p.n:
                    raise McomError("%s: %d names for %d reads" % (path, n_names, p.n))
            _mark_lossy(td, lossy)
            _mark_agree(td, agree)
            if digest:
                _digest_member(td, path, path2, lossy is None and agree is None, device, p.n if path2 is None else p.n // 2)
            sizes = pack(td, out_path, codec=codec, threads=threads, device=device if codec in ("rans", "bwt") else None)
        sizes["n_reads"] = p.n
        return sizes
    finally:
        p.close()


def _compress_ragged(path, out_path, td, codec, device, threads, quality, names, params, digest=False, align=False):
    """compress_fastq(ragged=True) in the order of `minicom -p -V`: lengths, the core over the reads of the modal length, the quality
    values, the names, the container.  None when every read has one length."""
    from .hip import McomError
    from .pipeline import Pipeline, fastq_lengths, fastq_name_member, fastq_quality_member_ragged
    len_path = os.path.join(td, RAGGED_MEMBERS[0])
    n, L, n_odd = fastq_lengths(path, len_path, device=device)
    if not n_odd:
        return None
    p = Pipeline.from_fastq_ragged(path, L, len_path, os.path.join(td, RAGGED_MEMBERS[1]), device=device, host_threads=threads, **params)
    try:
        p.pre_process()
        p.cluster_dump(td, order=True, paired=False)
        if align:                                                    # the odd reads against the contigs just dumped; an empty odd.seq is no member
            from .pipeline import odd_align_folder
            odd_align_folder(td, device=device)
            odd_seq = os.path.join(td, RAGGED_MEMBERS[1])
            if os.path.isfile(os.path.join(td, ODD_ALIGN_MEMBER)) and os.path.getsize(odd_seq) == 0:
                os.remove(odd_seq)
        if quality:
            n_rows = fastq_quality_member_ragged(path, L, len_path, os.path.join(td, QUALITY_MEMBER), os.path.join(td, RAGGED_MEMBERS[2]), device=device)
            if n_rows != p.n:
                raise McomError("%s: %d quality lines for %d reads" % (path, n_rows, p.n))
        if names:
            n_names = fastq_name_member(path, os.path.join(td, NAME_MEMBER), device=device)
            if n_names != n:
                raise McomError("%s: %d names for %d records" % (path, n_names, n))
        if digest:
            _digest_member(td, path, None, True, device, n)
        sizes = pack(td, out_path, codec=codec, threads=threads, device=device if codec in ("rans", "bwt") else None)
        sizes["n_reads"] = p.n
        sizes["n_records"] = n
        return sizes
    finally:
        p.close()


def compress_fastq_pair(path1: str, path2: str, out_path: str, quality: bool = False, names: bool = False, codec: str = "xz", device: int = 0,
                        threads: int = 8, quality_lossy=None, quality_agree=None, digest: bool = False, **params) -> dict:
    """Two FASTQ files of a pair -> a `.minicom` archive that keeps both in input order (`minicom -1 A_1.fastq -2 A_2.fastq -p [-Q [-N]]`,
    DESIGN.md section 3.12): the order-preserving members of the second file's reads behind the first's, and pe_order.txt.  quality=True:
    qual_1.mcq and qual_2.mcq; names=True (needs quality=True): name_1.mcn and name_2.mcn, the second coded against the first file's names
    -- decompress_file then gives both input files back byte for byte.  quality_lossy, quality_agree (need quality=True): as for
    compress_fastq; rows [0, n) of the agreement mask belong to the first file and rows [n, 2 n) to the second.  digest=True: as for compress_fastq, the digest of the pair.
    Returns pack()'s member sizes plus the number of pairs."""
    import tempfile
    from .hip import McomError
    from .pipeline import Pipeline, fastq_name_member
    if names and not quality:
        raise ValueError("names are kept beside the quality values only (quality=True)")
    lossy = _lossy_spec(quality_lossy, quality)
    agree = _agree_spec(quality_agree, quality)
    p = Pipeline.from_fastq(path1, device=device, path2=path2, host_threads=threads, **params)
    try:
        p.pre_process()
        with tempfile.TemporaryDirectory(dir=os.path.dirname(os.path.abspath(out_path)) or ".") as td:
            p.cluster_dump_order_pe(td)
            half = p.n // 2
            mask = _agree_mask(td, agree, device)
            for k, fq in ((1, path1), (2, path2)):
                if quality:
                    _quality_member(fq, half, p.L, device, os.path.join(td, "qual_%d.mcq" % k), lossy, agree, mask, (k - 1) * half)
                if names:
                    n_names = fastq_name_member(fq, os.path.join(td, "name_%d.mcn" % k), device=device, mate_path=path1 if k == 2 else None)
                    if n_names != half:
                        raise McomError("%s: %d names for %d reads" % (fq, n_names, half))
            _mark_lossy(td, lossy)
            _mark_agree(td, agree)
            if digest:
                _digest_member(td, path1, path2, lossy is None and agree is None, device, half)
            sizes = pack(td, out_path, codec=codec, threads=threads, device=device if codec in ("rans", "bwt") else None)
        sizes["n_pairs"] = half
        return sizes
    finally:
        p.close()


def _digest_member(folder: str, path: str, path2, with_qual: bool, device: int, n_archive: int) -> None:
    """digest.txt of the input into the folder; the run fails when it counts other records than the archive does"""
    from .hip import McomError
    from .pipeline import digest_parse, fastq_digest
    out = os.path.join(folder, DIGEST_MEMBER)
    n = digest_parse(fastq_digest(path, path2, with_qual=with_qual, device=device, out_path=out))["n"]
    if n != n_archive:
        os.remove(out)
        raise McomError("%s: the digest counts %d records, the archive %d" % (path, n, n_archive))


def _lossy_spec(quality_lossy, keeps_quality: bool):
    """the canonical text of compress_fastq's quality_lossy (None: none); ValueError without quality values or for a spec the parser refuses"""
    if quality_lossy is None:
        return None
    from .hip import McomError
    from .pipeline import qual_lossy_text
    if not keeps_quality:
        raise ValueError("quality_lossy changes the quality values that quality / quality_reordered keep: without either there are none")
    try:
        return qual_lossy_text(quality_lossy)
    except McomError as e:
        raise ValueError(str(e)) from None


def _agree_spec(quality_agree, allowed: bool):
    """(Q, C) of compress_fastq's quality_agree (None: none); ValueError where there are no quality values in input order or for numbers out of range"""
    if quality_agree is None:
        return None
    if not allowed:
        raise ValueError("quality_agree changes the quality values of an order-preserving archive (order=True or a pair, quality=True) or of one file kept with quality_reordered; not with ragged or a paired-end archive of the default mode")
    q, c = (quality_agree, 3) if isinstance(quality_agree, int) else tuple(quality_agree)
    if not (isinstance(q, int) and isinstance(c, int) and 0 <= q <= 93 and 1 <= c <= 255):
        raise ValueError("quality_agree is (Q, C) with Q 0 .. 93 and C 1 .. 255")
    return q, c


def _agree_mask(folder: str, agree, device: int):
    """the agreement mask of the stream files in `folder` as a uint8 device matrix (None without agree)"""
    if agree is None:
        return None
    import torch
    from .pipeline import agree_mask
    mask, _, _ = agree_mask(folder, agree[1], device=device)
    return torch.from_numpy(mask).to(f"cuda:{int(device)}")


def _mark_agree(folder: str, agree) -> None:
    if agree is not None:
        with open(os.path.join(folder, AGREE_MARKER), "wb") as f:
            f.write(b"%d %d\n" % agree)


def _mark_lossy(folder: str, lossy) -> None:
    if lossy is not None:
        with open(os.path.join(folder, LOSSY_MARKER), "wb") as f:
            f.write(lossy.encode() + b"\n")


def _quality_member(fastq: str, n: int, L: int, device: int, out_path: str, lossy=None, agree=None, mask=None, first_mask_row: int = 0) -> None:
    """the quality lines of `fastq` -> rows on the device [-> the agreement transform] [-> the lossy transform, in place] -> a `.mcq` member in out_path"""
    from .hip import Context, McomError
    from .pipeline import fastq_qualities
    rows = fastq_qualities(fastq, L, device=device)
    if int(rows.shape[0]) != n:
        raise McomError("%s: %d quality lines for %d reads" % (fastq, int(rows.shape[0]), n))
    ctx = Context(device)
    if agree is not None:
        rows, _ = ctx.qual_agree(rows, mask, agree[0], first_mask_row=first_mask_row, in_place=True)
    if lossy is not None:
        rows, _ = ctx.qual_transform(rows, lossy, in_place=True)
    member = ctx.qual_encode(rows)
    with open(out_path, "wb") as f:
        f.write(member.cpu().numpy().tobytes())


def decompress_file(path: str, out_path: str, out_path2: str | None = None, threads: int = 8, device: int | None = None, gzip: bool = False,
                    records: tuple[int, int] | None = None) -> int:
    """`.minicom` -> reads, one per line: the original order for an archive written with -p, two files (line i of both a
    pair) for a paired-end archive.  Returns the number of reads (pairs for paired end).  device=None: host only; an
    integer: `.rans` and `.bwt` members decoded and the reads rebuilt on that GPU (pipeline.decompress(..., device=)); the other codecs
    are host code either way.  An archive with quality values (compress_fastq(quality=True)) gives FASTQ instead: four-line records
    `@<i+1>`, read, `+`, qualities -- or, for an archive that carries name.mcn (compress_fastq(names=True)), the records with their names
    and `+` texts: the input file.  gzip=True: the output file(s) are BGZF (gzip members of 65280 bytes of text
    each) -- compressed on the GPU by the decoders' tails when `device` is given and the paths end in `.gz` (on that route the suffix
    alone decides, with or without the keyword), otherwise the plain file is written beside the archive's members first and
    pipeline.bgzf_file turns it into the same bytes.  An archive made with quality_agree (qual_agree.txt) is decoded as ever; that its
    quality values are lossy is said in one line on stderr, as `minicom -d` says it.  An archive made with digest=True (digest.txt) is
    checked: the files just written are digested as the input was (pipeline.digest_check, on `device` when given) and McomError says which
    part differs; the files are kept.  records=(first, count): only records first .. first + count - 1 (first from 0, clipped at the
    archive's end) of a -p archive (pipeline.decompress_range): the slice of what the call writes without it;
    McomError for an archive without the input order, one made with -q or -V, and first > n.  A range is not checked against a digest."""
    import tempfile
    outs = [o for o in (out_path, out_path2) if o is not None]
    if gzip and not (device is not None and all(o.endswith(".gz") for o in outs)):
        from .pipeline import bgzf_file
        with tempfile.TemporaryDirectory(dir=os.path.dirname(os.path.abspath(out_path)) or ".") as plain:
            tmp = [os.path.join(plain, "out_%d" % k) for k in range(len(outs))]
            n = decompress_file(path, tmp[0], tmp[1] if len(tmp) > 1 else None, threads=threads, device=device, records=records)
            for t, o in zip(tmp, outs):
                bgzf_file(t, o, device=device)
        return n
    with tempfile.TemporaryDirectory(dir=os.path.dirname(os.path.abspath(out_path)) or ".") as td:
        kinds = unpack(path, td, threads=threads, device=device)
        if records is not None:
            from .pipeline import decompress_range
            if kinds.get("pair_order") and out_path2 is None:
                raise ValueError("an archive of a pair decodes into two files")
            return decompress_range(td, out_path, int(records[0]), int(records[1]), device=device, fastq=bool(kinds.get("quality") or kinds.get("names")),
                                    out_path2=out_path2 if kinds.get("pair_order") else None)
        n = _decode_folder(td, kinds, out_path, out_path2, device)
        if kinds.get("digest"):
            from .hip import McomError
            from .pipeline import digest_check
            rep = digest_check(td, out_path, out_path2, device=device)
            if not rep["identical"]:
                raise McomError("%s: the decompressed files are not the compressed input (%s differs); they were kept" % (path, rep["first_diff"]))
        return n


def _decode_folder(td: str, kinds: dict, out_path: str, out_path2, device) -> int:
    """the stream files of an unpacked archive -> its output file(s), by what unpack says about it"""
    from .pipeline import decompress, decompress_fastq, decompress_pe
    if kinds.get("quality_agree") is not None:                   # as `minicom -d` says it; the decoders do not change
        import sys
        print("minicom: the quality values of this archive are lossy: agreeing bases stored as Phred %s (coverage >= %s)" % tuple((kinds["quality_agree"].split(" ") + ["?", "?"])[:2]), file=sys.stderr)
    if kinds.get("pair_order"):                                  # seen first: its other members are those of a -p archive
        from .pipeline import decompress_order_pe
        if out_path2 is None:
            raise ValueError("an archive of a pair decodes into two files")
        return decompress_order_pe(td, out_path, out_path2, device=device, fastq=bool(kinds.get("quality") or kinds.get("names")))
    if kinds.get("quality_reordered"):
        from .pipeline import decompress_fastq_reordered, decompress_fastq_pe
        if kinds["paired"]:
            if out_path2 is None:
                raise ValueError("a paired-end archive decodes into two files")
            return decompress_fastq_pe(td, out_path, out_path2, device=device)
        return decompress_fastq_reordered(td, out_path, device=device)
    if kinds.get("quality"):
        return decompress_fastq(td, out_path, device=device)
    if kinds["paired"]:
        if out_path2 is None:
            raise ValueError("a paired-end archive decodes into two files")
        return decompress_pe(td, out_path, out_path2, device=device)
    return decompress(td, out_path, order=kinds["order"], device=device)


def test_file(path: str, threads: int = 8, device: int | None = None) -> dict:
    """`minicom -d X.minicom -T`: an archive made with digest=True is decoded into a temporary folder beside it and the result checked
    against the stored digest; nothing is kept.  Returns pipeline.digest_check's report ("identical", "compared", "differing", ...);
    McomError for an archive without digest.txt."""
    import tempfile
    from .hip import McomError
    from .pipeline import digest_check
    with tempfile.TemporaryDirectory(dir=os.path.dirname(os.path.abspath(path)) or ".") as td:
        folder = os.path.join(td, "members")
        kinds = unpack(path, folder, threads=threads, device=device)
        if not kinds.get("digest"):
            raise McomError("%s holds no digest.txt: it was made without digest=True (`minicom -K`)" % path)
        two = bool(kinds["paired"] or kinds.get("pair_order"))
        fastq = bool(kinds.get("quality") or kinds.get("names") or kinds.get("quality_reordered"))
        outs = [os.path.join(td, "out_%d.%s" % (k + 1, "fastq" if fastq else "reads")) for k in range(2 if two else 1)]
        _decode_folder(folder, kinds, outs[0], outs[1] if two else None, device)
        return digest_check(folder, outs[0], outs[1] if two else None, device=device)


test_file.__test__ = False        # (not a test: pytest collects by name)


def verify_file(path: str, fastq: str, fastq2: str | None = None, threads: int = 8, device: int = 0) -> dict:
    """`.minicom` against the FASTQ it was made from, on GPU `device`, without writing a read: pipeline.verify's report.  The mode comes
    from the members, as in decompress_file: a paired-end archive needs `fastq2`, a -p archive is held line against line, any other
    one as a multiset of reads.  For an archive made with quality_lossy the FASTQ file's quality rows go through the transform that
    qual_lossy.txt names before they are compared (the report gets "quality_lossy": its spec; McomError when the file holds no spec).
    For an archive made with quality_agree the agreement mask is rebuilt from the archive on `device` and the file's quality rows go through it
    first (the report gets "quality_agree": (Q, C); McomError when qual_agree.txt does not parse).
    An archive with quality values is held against the quality lines as well: the report gets
    "quality" (pipeline.verify_quality's) and "identical" is true only when both checks say so; one with names likewise gets "names"
    (pipeline.verify_names's)."""
    import tempfile
    from .hip import McomError
    from .pipeline import verify, verify_quality
    if not os.path.isfile(path):
        raise McomError("no such archive: %s" % path)
    with tempfile.TemporaryDirectory(dir=os.path.dirname(os.path.abspath(path)) or ".") as td:
        kinds = unpack(path, td, threads=threads, device=device)
        from .pipeline import qual_lossy_marker
        lossy = qual_lossy_marker(td)                                # (McomError for a marker that is no spec)
        from .pipeline import qual_agree_marker
        agree = qual_agree_marker(td)                                # (McomError for a marker that does not parse)
        tag = lambda r: dict(r, **({"quality_lossy": lossy} if lossy is not None else {}), **({"quality_agree": agree} if agree is not None else {}))
        if kinds.get("pair_order"):
            from .pipeline import verify_order_pe
            if fastq2 is None:
                raise McomError("an archive of a pair is verified against two FASTQ files")
            return tag(verify_order_pe(td, fastq, fastq2, device=device))
        if kinds["paired"] != (fastq2 is not None):
            raise McomError("a paired-end archive is verified against two FASTQ files, any other against one")
        if kinds.get("quality_reordered"):
            from .pipeline import verify_records
            return tag(verify_records(td, fastq, fastq2, device=device))
        if kinds.get("ragged"):                                      # part by part, then the names as ever
            from .pipeline import verify_ragged
            rep = verify_ragged(td, fastq, device=device)
            if kinds.get("names"):
                from .pipeline import verify_names
                rep["names"] = verify_names(td, fastq, device=device)
                rep["identical"] = rep["identical"] and rep["names"]["identical"]
            return rep
        rep = tag(verify(td, fastq, fastq2, order=kinds["order"], device=device))
        if kinds.get("quality"):
            rep["quality"] = verify_quality(td, fastq, device=device)
            rep["identical"] = rep["identical"] and rep["quality"]["identical"]
        if kinds.get("names"):
            from .pipeline import verify_names
            rep["names"] = verify_names(td, fastq, device=device)
            rep["identical"] = rep["identical"] and rep["names"]["identical"]
        return rep
