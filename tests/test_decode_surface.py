"""The device decoder's public surface, checked where there is no GPU: the entry points exist in the headers and the libraries, the GPU route
fails loudly (no output file, no quiet host decode) while the host route still decodes, and the command line knows --gpu."""
import gzip
import io
import os
import re
import subprocess
import tarfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_ENTRIES = ["mcomh_decompress_gpu", "mcomh_decompress_order_gpu", "mcomh_decompress_pe_gpu"]
DECODE_ENTRIES = ["mcom_decode_walk_headers", "mcom_decode_line_index", "mcom_decode_member_table", "mcom_decode_list_ids", "mcom_decode_member_ids",
                  "mcom_decode_pe_dest", "mcom_decode_check_lines", "mcom_decode_reads"]


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_host_header_declares_and_library_exports_the_gpu_decoders():
    from minicom_amd import pipeline
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcom_host.h")).read(), flags=re.S)
    lib = pipeline.load_host_library()
    for name in GPU_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in pipeline.HOST_ABI_SYMBOLS
        getattr(lib, name)


def test_hip_library_exports_the_decode_entries():
    import minicom_amd
    lib = minicom_amd.load_library()
    for name in DECODE_ENTRIES:
        assert name in minicom_amd.ABI_SYMBOLS, name
        getattr(lib, name)
    assert [s for s in minicom_amd.ABI_SYMBOLS if s.startswith("mcom_decode_")] == sorted(DECODE_ENTRIES)


def test_walk_headers_is_plain_host_code():
    """the serial part of the decoder needs no GPU: contig headers of a hand-made beg_pos.bin, and a chain that leaves the file"""
    import ctypes as C
    import numpy as np
    import minicom_amd
    lib = minicom_amd.load_library()
    img = b"".join([np.uint32(2).tobytes(), np.array([0, 7], "<u2").tobytes(), np.uint32(0).tobytes(), np.uint32(1).tobytes(), np.array([65535], "<u2").tobytes(), b"\x01\x02"])
    buf = np.frombuffer(img, dtype=np.uint8)
    nc, nm = C.c_uint64(), C.c_uint64()
    moff = np.zeros(4, dtype=np.uint64)
    assert lib.mcom_decode_walk_headers(buf.ctypes.data, buf.size, moff.ctypes.data, 3, C.byref(nc), C.byref(nm)) == 0
    assert (nc.value, nm.value, moff.tolist()) == (3, 3, [0, 2, 2, 3])
    bad = np.frombuffer(np.uint32(1 << 31).tobytes() + b"\0" * 8, dtype=np.uint8)
    assert lib.mcom_decode_walk_headers(bad.ctypes.data, bad.size, None, 0, C.byref(nc), C.byref(nm)) != 0


@pytest.mark.skipif(_have_gpu(), reason="what the GPU route does without a GPU")
def test_gpu_route_fails_loudly_without_a_gpu_and_the_host_route_still_decodes(golden_dir, tmp_path):
    from minicom_amd.hip import McomError
    from minicom_amd.pipeline import decompress
    d = tmp_path / "streams"; d.mkdir()
    with gzip.open(os.path.join(golden_dir, "streams_stages_L100.tar.gz"), "rb") as g:
        tf = tarfile.open(fileobj=io.BytesIO(g.read()))
        for m in tf.getmembers():
            (d / m.name).write_bytes(tf.extractfile(m).read())
    out = tmp_path / "gpu.txt"
    with pytest.raises(McomError):
        decompress(str(d), str(out), device=0)
    assert not out.exists()
    host = tmp_path / "host.txt"
    assert decompress(str(d), str(host), device=None) > 0 and host.stat().st_size > 0


def test_command_line_knows_gpu():
    exe = os.path.join(ROOT, "bin", "decompress")
    for argv in ([exe, "--gpu"], [exe, "--gpu", "dir", "out", "false"]):
        r = subprocess.run(argv, capture_output=True, text=True)
        assert r.returncode == 1 and "usage: decompress [--gpu]" in r.stderr, r.stderr
    assert "--gpu" in open(os.path.join(ROOT, "bin", "minicom")).read()
