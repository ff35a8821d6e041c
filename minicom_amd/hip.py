"""ctypes binding of libmcom_hip.so (include/mcom.h) over torch CUDA(=HIP) tensors."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MM_DTYPE = np.dtype([("x", "<u8"), ("y", "<u8")])


class McomError(RuntimeError):
    pass


class DecodeSrc(C.Structure):
    """mcom_decode_src of include/mcom.h"""
    _fields_ = [("d_text", C.c_void_p), ("text_bytes", C.c_uint64), ("d_line_start", C.c_void_p), ("verbatim", C.c_int),
                ("d_ref", C.c_void_p), ("ref_bytes", C.c_uint64), ("ref_const", C.c_int),
                ("d_cid", C.c_void_p), ("d_pos", C.c_void_p), ("d_coff", C.c_void_p), ("n_contigs", C.c_uint64),
                ("d_dir", C.c_void_p), ("dir_bytes", C.c_uint64)]


DECODE_F_BOUNDS, DECODE_F_LINE, DECODE_F_DUP, DECODE_F_DEST = 1, 2, 4, 8


class VerifyTable(C.Structure):
    """mcom_verify_table of include/mcom.h"""
    _fields_ = [("d_rows", C.c_void_p), ("d_mates", C.c_void_p), ("pitch", C.c_uint64), ("n", C.c_uint64)]


class VerifyParts(C.Structure):
    """mcom_verify_parts of include/mcom.h"""
    _fields_ = [("d_part", C.c_void_p * 4), ("n_parts", C.c_int), ("pitch", C.c_uint64), ("n", C.c_uint64)]


class VerifyReport(C.Structure):
    """mcom_verify_report of include/mcom.h"""
    _fields_ = [("n_a", C.c_uint64), ("n_b", C.c_uint64), ("missing", C.c_uint64), ("extra", C.c_uint64), ("differing", C.c_uint64),
                ("first_diff", C.c_uint64), ("exact_runs", C.c_uint64), ("missing_ex", C.c_uint64 * 8), ("extra_ex", C.c_uint64 * 8),
                ("n_missing_ex", C.c_uint32), ("n_extra_ex", C.c_uint32), ("identical", C.c_int)]


class QualLossySpec(C.Structure):
    """mcom_qual_lossy_spec of include/mcom.h = mcomh_qual_lossy_spec of include/mcom_host.h"""
    ILL8, THR, PBLOCK, LUT = 1, 2, 3, 4
    _fields_ = [("kind", C.c_uint32), ("p", C.c_uint32 * 3), ("lut", C.c_uint8 * 256)]

    @classmethod
    def from_lut(cls, lut):
        """a general byte map: 256 values; the transform refuses one that is not idempotent"""
        s = cls(); s.kind = cls.LUT
        lut = np.asarray(lut, dtype=np.uint8).reshape(256)
        C.memmove(s.lut, lut.ctypes.data, 256)
        return s


class QualLossyReport(C.Structure):
    """mcom_qual_lossy_report of include/mcom.h"""
    _fields_ = [("changed", C.c_uint64), ("sum_abs", C.c_uint64), ("sum_sq", C.c_uint64), ("max_abs", C.c_uint64)]

    def as_dict(self) -> dict:
        return {"changed": int(self.changed), "sum_abs": int(self.sum_abs), "sum_sq": int(self.sum_sq), "max_abs": int(self.max_abs)}


class QualAgreeReport(C.Structure):
    """mcom_qual_agree_report of include/mcom.h = mcomh_qual_agree_report of include/mcom_host.h"""
    _fields_ = [("changed", C.c_uint64), ("sum_abs", C.c_uint64), ("sum_sq", C.c_uint64), ("max_abs", C.c_uint64), ("mask_bits", C.c_uint64)]

    def as_dict(self) -> dict:
        return {"changed": int(self.changed), "sum_abs": int(self.sum_abs), "sum_sq": int(self.sum_sq), "max_abs": int(self.max_abs), "mask_bits": int(self.mask_bits)}


class RaggedSrc(C.Structure):
    """mcom_ragged_src of include/mcom.h"""
    _fields_ = [("d_reads", C.c_void_p), ("read_pitch", C.c_uint64), ("d_quals", C.c_void_p), ("qual_pitch", C.c_uint64), ("n_even", C.c_uint64),
                ("d_odd_seq", C.c_void_p), ("d_odd_qual", C.c_void_p), ("odd_bytes", C.c_uint64), ("d_slot", C.c_void_p), ("d_len", C.c_void_p), ("n", C.c_uint64),
                ("d_names", C.c_void_p), ("names_bytes", C.c_uint64), ("d_rec_off", C.c_void_p), ("L", C.c_uint32)]


def _gzip_member_dtype():
    import numpy as np
    return np.dtype([("in_off", "<u8"), ("in_bytes", "<u8"), ("out_off", "<u8"), ("isize", "<u4"), ("crc", "<u4")])


GZIP_MEMBER_DTYPE = _gzip_member_dtype()     # mcom_gzip_member of include/mcom.h
SCAN_STEP_DTYPE = np.dtype([("op", "<u4"), ("width", "<u4"), ("a", "<u8"), ("b", "<u8"), ("n", "<u8")])   # mcom_test_scan_step of include/mcom_test.h
SCAN_STEP_SCAN, SCAN_STEP_READBACK, SCAN_STEP_LAUNCH, SCAN_STEP_COPY, SCAN_STEP_SYNC = 0, 1, 2, 3, 4


def rans_hint(model: int, stride: int = 1) -> int:
    """MCOM_RANS_HINT of include/mcom.h"""
    return 0x100 | (model << 4) | stride


def lib_path() -> str:
    return os.path.join(HERE, "lib", "libmcom_hip.so")


def header_path() -> str:
    return os.path.join(os.path.dirname(HERE), "include", "mcom.h")


def _declared_symbols() -> list[str]:
    """every entry point include/mcom.h (the boundary) and include/mcom_test.h (test hooks) declare"""
    names = set()
    for h in (header_path(), os.path.join(os.path.dirname(header_path()), "mcom_test.h")):
        txt = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        names |= set(re.findall(r"\b(mcom_[a-z0-9_]+)\s*\(", txt))
    return sorted(names)


ABI_SYMBOLS = _declared_symbols()

_lib = None


def load_library():
    """Loads the HIP library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise McomError(f"{p} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(there is no CPU fallback for the product path)")
    # PyTorch ships its own libamdhip64.so.7; whichever HIP runtime is mapped first serves the whole process,
    # and torch.cuda stops working when it is not torch's.  So torch is always imported before our library.
    import torch  # noqa: F401
    L = C.CDLL(p)
    vp, sz, i32, u32, u64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint64
    L.mcom_create.restype = i32; L.mcom_create.argtypes = [C.POINTER(vp), i32, vp]
    L.mcom_destroy.restype = None; L.mcom_destroy.argtypes = [vp]
    L.mcom_set_stream.restype = i32; L.mcom_set_stream.argtypes = [vp, vp]
    L.mcom_sync.restype = i32; L.mcom_sync.argtypes = [vp]
    L.mcom_last_error.restype = C.c_char_p; L.mcom_last_error.argtypes = [vp]
    L.mcom_version.restype = C.c_char_p; L.mcom_version.argtypes = []
    L.mcom_prof_enable.restype = i32; L.mcom_prof_enable.argtypes = [vp, i32]
    L.mcom_prof_reset.restype = i32; L.mcom_prof_reset.argtypes = [vp]
    L.mcom_prof_read.restype = i32; L.mcom_prof_read.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(u64)]
    L.mcom_prof_kernels.restype = i32; L.mcom_prof_kernels.argtypes = [vp, C.c_char_p, C.c_char_p, sz, C.POINTER(sz)]
    L.mcom_process_reads.restype = i32
    L.mcom_process_reads.argtypes = [vp, vp, sz, sz, i32, i32, i32, u32, vp, vp, vp, vp, vp]
    L.mcom_special_reads.restype = i32
    L.mcom_special_reads.argtypes = [vp, vp, sz, vp, u32, vp]
    L.mcom_process_reads_packed.restype = i32
    L.mcom_process_reads_packed.argtypes = [vp, vp, vp, sz, i32, i32, i32, u32, vp, vp, vp, vp, vp]
    L.mcom_sketch_reads.restype = i32
    L.mcom_sketch_reads.argtypes = [vp, vp, vp, sz, i32, i32, u32, vp]
    L.mcom_hash64_batch.restype = i32; L.mcom_hash64_batch.argtypes = [vp, vp, sz, i32, vp]
    L.mcom_encode_byte.restype = i32; L.mcom_encode_byte.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, i32, vp]
    L.mcom_radix_sort_128x.restype = i32; L.mcom_radix_sort_128x.argtypes = [vp, vp, sz]
    L.mcom_sort_group.restype = i32
    L.mcom_sort_group.argtypes = [vp, vp, sz, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    L.mcom_sketch_contigs.restype = i32
    L.mcom_sketch_contigs.argtypes = [vp, vp, vp, vp, sz, i32, i32, u32, vp, vp, sz, C.POINTER(u64)]
    L.mcom_pack_contigs.restype = i32; L.mcom_pack_contigs.argtypes = [vp, vp, vp, vp, u32, u64, vp]
    L.mcom_idx_build.restype = i32; L.mcom_idx_build.argtypes = [vp, vp, sz, i32, i32, C.POINTER(vp)]
    L.mcom_radix_sort_128x_ref_order.restype = i32; L.mcom_radix_sort_128x_ref_order.argtypes = [vp, vp, sz]
    L.mcom_idx_destroy.restype = None; L.mcom_idx_destroy.argtypes = [vp, vp]
    L.mcom_idx_get.restype = i32; L.mcom_idx_get.argtypes = [vp, vp, vp, sz, vp, vp]
    L.mcom_idx_records.restype = i32; L.mcom_idx_records.argtypes = [vp, vp, vp, C.POINTER(sz)]
    L.mcom_match_pro.restype = i32; L.mcom_match_pro.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.mcom_find_next_candidates.restype = i32
    L.mcom_find_next_candidates.argtypes = [vp, vp, vp, sz, vp, vp, vp, i32, vp, sz, vp]
    L.mcom_find_next_candidates_new.restype = i32
    L.mcom_find_next_candidates_new.argtypes = [vp, vp, vp, sz, vp, vp, vp, i32, u32, vp, sz, vp]
    L.mcom_dict_layout.restype = i32; L.mcom_dict_layout.argtypes = [i32, i32, vp, vp]
    L.mcom_gather_rows.restype = i32; L.mcom_gather_rows.argtypes = [vp, vp, vp, sz, i32, vp]
    L.mcom_poly_filter.restype = i32; L.mcom_poly_filter.argtypes = [vp, vp, vp, vp, sz, i32, i32, vp]
    L.mcom_dicts_build.restype = i32; L.mcom_dicts_build.argtypes = [vp, vp, sz, i32, i32, C.POINTER(vp)]
    L.mcom_dicts_free.restype = None; L.mcom_dicts_free.argtypes = [vp, vp]
    L.mcom_dicts_info.restype = i32; L.mcom_dicts_info.argtypes = [vp, C.POINTER(i32), vp, vp]
    L.mcom_dicts_lookup.restype = i32; L.mcom_dicts_lookup.argtypes = [vp, vp, i32, vp, sz, vp, vp]
    L.mcom_dicts_ids.restype = i32; L.mcom_dicts_ids.argtypes = [vp, vp, i32, vp]
    L.mcom_realign_pass.restype = i32
    L.mcom_realign_pass.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, u64, i32, i32, vp, vp]
    L.mcom_cindex_plan.restype = i32
    L.mcom_cindex_plan.argtypes = [u64, u32, i32, i32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.mcom_cindex_build.restype = i32
    L.mcom_cindex_build.argtypes = [vp, vp, vp, vp, u32, u64, i32, i32, u64, vp, u64]
    L.mcom_dicts_eligible.restype = i32
    L.mcom_dicts_eligible.argtypes = [vp, vp, vp, i32, vp]
    L.mcom_realign_pass_reads.restype = i32
    L.mcom_realign_pass_reads.argtypes = [vp, vp, u64, vp, vp, vp, sz, vp, vp, vp, u32, i32, i32, i32, vp, vp]
    L.mcom_dicts_screen.restype = i32
    L.mcom_dicts_screen.argtypes = [vp, vp, sz, i32, i32, i32, C.POINTER(i32)]
    L.mcom_claims_resolve.restype = i32
    L.mcom_claims_resolve.argtypes = [vp, vp, vp, sz, u32, vp, vp, vp, C.POINTER(u64)]
    L.mcom_scan_u64.restype = i32; L.mcom_scan_u64.argtypes = [vp, vp, vp, sz]
    L.mcom_contig_layout.restype = i32; L.mcom_contig_layout.argtypes = [vp, vp, sz, vp, vp, C.POINTER(u64)]
    L.mcom_group_consensus.restype = i32; L.mcom_group_consensus.argtypes = [vp, vp, vp, vp, u32, i32, i32, i32, vp, vp, vp, vp, vp, i32]
    L.mcom_groups_to_contigs.restype = i32
    L.mcom_groups_to_contigs.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, vp, i32, u64, u64, u64, vp, u64, vp, vp, u64, vp, u64, vp, vp, u64, C.POINTER(u64)]
    L.mcom_merge_members.restype = i32; L.mcom_merge_members.argtypes = [vp, vp, vp, vp, sz, i32, i32, vp, vp, vp, C.POINTER(u64)]
    L.mcom_merge_consensus_jobs.restype = i32; L.mcom_merge_consensus_jobs.argtypes = [vp, vp, vp, vp, vp, sz, u64, i32, vp, vp, vp, vp]
    L.mcom_contigs_carry.restype = i32; L.mcom_contigs_carry.argtypes = [vp, vp, vp, vp, vp, sz, vp, sz, sz, vp, vp, vp, vp, vp, C.POINTER(u64)]
    L.mcom_resketch_merged.restype = i32
    L.mcom_resketch_merged.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, u64, i32, i32, vp, vp, sz, C.POINTER(u64), C.POINTER(u64)]
    L.mcom_members_finalize.restype = i32
    L.mcom_members_finalize.argtypes = [vp, vp, vp, sz, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), i32, i32, vp, vp]
    L.mcom_compact_live.restype = i32; L.mcom_compact_live.argtypes = [vp, vp, vp, sz, vp, C.POINTER(u64)]
    L.mcom_window_layout.restype = i32; L.mcom_window_layout.argtypes = [vp, vp, sz, i32, vp, C.POINTER(u64), C.POINTER(u64)]
    L.mcom_records_carry.restype = i32; L.mcom_records_carry.argtypes = [vp, vp, vp, vp, sz, u32, u32, vp, sz, vp, C.POINTER(u64)]
    L.mcom_claim_pairs.restype = i32
    L.mcom_claim_pairs.argtypes = [vp, vp, sz, sz, i32, vp, vp, C.POINTER(u64), C.POINTER(i32)]
    # decoder (csrc/decode.hip)
    L.mcom_decode_walk_headers.restype = i32; L.mcom_decode_walk_headers.argtypes = [vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.mcom_decode_line_index.restype = i32; L.mcom_decode_line_index.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), vp]
    L.mcom_decode_member_table.restype = i32; L.mcom_decode_member_table.argtypes = [vp, vp, u64, vp, u64, u64, i32, vp, vp, vp, C.POINTER(u64), vp]
    L.mcom_decode_list_ids.restype = i32; L.mcom_decode_list_ids.argtypes = [vp, vp, u64, vp]
    L.mcom_decode_member_ids.restype = i32; L.mcom_decode_member_ids.argtypes = [vp, vp, u64, vp, vp, vp, vp]
    L.mcom_decode_pe_dest.restype = i32; L.mcom_decode_pe_dest.argtypes = [vp, vp, u64, u64, u64, vp, u64, u64, u64, vp, C.POINTER(u64), vp]
    L.mcom_decode_check_lines.restype = i32; L.mcom_decode_check_lines.argtypes = [vp, vp, u64, vp, u64, i32, i32, vp]
    L.mcom_decode_reads.restype = i32; L.mcom_decode_reads.argtypes = [vp, C.POINTER(DecodeSrc), u64, i32, vp, u64, vp, u64, vp, vp]
    L.mcom_range_check_dest.restype = i32; L.mcom_range_check_dest.argtypes = [vp, vp, u64, u64, u64, vp, vp]
    L.mcom_range_decode_reads.restype = i32; L.mcom_range_decode_reads.argtypes = [vp, C.POINTER(DecodeSrc), u64, i32, vp, u64, u64, u64, vp, vp]
    L.mcom_verify_room.restype = u64; L.mcom_verify_room.argtypes = [u64, u64]
    L.mcom_verify_ordered.restype = i32; L.mcom_verify_ordered.argtypes = [vp, C.POINTER(VerifyTable), C.POINTER(VerifyTable), i32, C.POINTER(VerifyReport)]
    L.mcom_verify_multiset.restype = i32; L.mcom_verify_multiset.argtypes = [vp, C.POINTER(VerifyTable), C.POINTER(VerifyTable), i32, C.POINTER(VerifyReport)]
    L.mcom_set_verify_hash_bits.restype = i32; L.mcom_set_verify_hash_bits.argtypes = [vp, i32]
    L.mcom_rans_bound.restype = u64; L.mcom_rans_bound.argtypes = [u64]
    L.mcom_rans_encode.restype = i32; L.mcom_rans_encode.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), i32]
    L.mcom_rans_decode.restype = i32; L.mcom_rans_decode.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
    L.mcom_fastq_quality_rows.restype = i32; L.mcom_fastq_quality_rows.argtypes = [vp, vp, u64, vp, u64, u64, C.c_uint32, vp, u64, vp]
    L.mcom_fastq_emit.restype = i32; L.mcom_fastq_emit.argtypes = [vp, vp, u64, vp, u64, u64, u64, C.c_uint32, vp, C.POINTER(u64)]
    L.mcom_qual_bound.restype = u64; L.mcom_qual_bound.argtypes = [u64, C.c_uint32]
    L.mcom_qual_encode.restype = i32; L.mcom_qual_encode.argtypes = [vp, vp, u64, C.c_uint32, u64, vp, u64, C.POINTER(u64), i32]
    L.mcom_qual_gather_rows.restype = i32; L.mcom_qual_gather_rows.argtypes = [vp, vp, u64, C.c_uint32, u64, vp, u64, vp, u64, vp]
    L.mcom_dump_read_order.restype = i32; L.mcom_dump_read_order.argtypes = [vp, vp, u64, vp, u64, C.c_uint32, vp, C.POINTER(u64)]
    L.mcom_verify_multiset_parts.restype = i32; L.mcom_verify_multiset_parts.argtypes = [vp, C.POINTER(VerifyParts), C.POINTER(VerifyParts), i32, C.POINTER(VerifyReport)]
    L.mcom_agree_coverage.restype = i32; L.mcom_agree_coverage.argtypes = [vp, vp, vp, vp, u64, u64, i32, u64, vp, vp]
    L.mcom_agree_mask.restype = i32; L.mcom_agree_mask.argtypes = [vp, C.POINTER(DecodeSrc), u64, i32, vp, u64, u64, vp, u64, C.c_uint32, vp, u64, vp]
    L.mcom_qual_agree.restype = i32; L.mcom_qual_agree.argtypes = [vp, vp, u64, C.c_uint32, u64, vp, u64, u64, C.c_uint32, C.POINTER(QualAgreeReport)]
    L.mcom_qual_transform.restype = i32; L.mcom_qual_transform.argtypes = [vp, vp, u64, C.c_uint32, u64, C.POINTER(QualLossySpec), C.POINTER(QualLossyReport)]
    L.mcom_bgzf_bound.restype = u64; L.mcom_bgzf_bound.argtypes = [u64]
    L.mcom_bgzf_encode.restype = i32; L.mcom_bgzf_encode.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), i32]
    L.mcom_gzip_walk.restype = i32; L.mcom_gzip_walk.argtypes = [vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.mcom_gzip_inflate.restype = i32; L.mcom_gzip_inflate.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, C.POINTER(u64), C.POINTER(u64)]
    L.mcom_test_qual_pblock_tile_rows.restype = C.c_uint32; L.mcom_test_qual_pblock_tile_rows.argtypes = []
    L.mcom_test_scan_u32.restype = i32; L.mcom_test_scan_u32.argtypes = [vp, vp, vp, sz]
    L.mcom_test_scan_constants.restype = None; L.mcom_test_scan_constants.argtypes = [C.POINTER(u32)] * 5
    L.mcom_test_n_cu.restype = i32; L.mcom_test_n_cu.argtypes = [vp]
    L.mcom_test_scan_script.restype = i32; L.mcom_test_scan_script.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, sz, vp, sz]
    L.mcom_qual_info.restype = i32; L.mcom_qual_info.argtypes = [vp, u64, C.POINTER(u64), C.POINTER(C.c_uint32)]
    L.mcom_qual_decode.restype = i32; L.mcom_qual_decode.argtypes = [vp, vp, u64, vp, u64, u64, C.POINTER(u64), C.POINTER(C.c_uint32)]
    L.mcom_qual_decode_rows.restype = i32; L.mcom_qual_decode_rows.argtypes = [vp, vp, u64, u64, u64, vp, u64, C.POINTER(u64), C.POINTER(C.c_uint32)]
    L.mcom_name_bound.restype = u64; L.mcom_name_bound.argtypes = [u64]
    L.mcom_name_encode.restype = i32; L.mcom_name_encode.argtypes = [vp, vp, u64, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.mcom_name_info.restype = i32; L.mcom_name_info.argtypes = [vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.mcom_name_decode.restype = i32; L.mcom_name_decode.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64), vp]
    L.mcom_name_encode_mate.restype = i32; L.mcom_name_encode_mate.argtypes = [vp, vp, u64, u64, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.mcom_name_info_mate.restype = i32; L.mcom_name_info_mate.argtypes = [vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.mcom_name_decode_mate.restype = i32; L.mcom_name_decode_mate.argtypes = [vp, vp, u64, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.mcom_name_text_offsets.restype = i32; L.mcom_name_text_offsets.argtypes = [vp, vp, u64, u64, vp]
    L.mcom_name_compare.restype = i32; L.mcom_name_compare.argtypes = [vp, vp, vp, u64, vp, vp, u64, u64, C.POINTER(u64), C.POINTER(u64)]
    L.mcom_fastq_name_text.restype = i32; L.mcom_fastq_name_text.argtypes = [vp, vp, u64, vp, u64, u64, vp, u64, C.POINTER(u64), vp, vp]
    L.mcom_fastq_emit_named.restype = i32; L.mcom_fastq_emit_named.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, C.c_uint32, vp, C.POINTER(u64)]
    L.mcom_fastq_record_hashes.restype = i32; L.mcom_fastq_record_hashes.argtypes = [vp, vp, u64, vp, u64, u64, i32, u64, vp, vp, vp, vp]
    L.mcom_digest_reduce.restype = i32; L.mcom_digest_reduce.argtypes = [vp, vp, vp, vp, vp, vp, vp, u64, vp]
    L.mcom_fastq_lengths.restype = i32; L.mcom_fastq_lengths.argtypes = [vp, vp, u64, vp, u64, u64, vp, vp, vp]
    L.mcom_ragged_index.restype = i32; L.mcom_ragged_index.argtypes = [vp, vp, u64, C.c_uint32, vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.mcom_fastq_ragged_rows.restype = i32; L.mcom_fastq_ragged_rows.argtypes = [vp, vp, u64, vp, u64, u64, i32, C.c_uint32, vp, vp, u64, vp, u64, u64, vp, u64, vp]
    L.mcom_fastq_emit_ragged.restype = i32; L.mcom_fastq_emit_ragged.argtypes = [vp, C.POINTER(RaggedSrc), u64, u64, vp, u64, C.POINTER(u64)]
    L.mcom_odd_text_append.restype = i32; L.mcom_odd_text_append.argtypes = [vp, vp, u64, u64, vp, u64, u64]
    L.mcom_odd_index_build.restype = i32; L.mcom_odd_index_build.argtypes = [vp, vp, u64, C.POINTER(vp)]
    L.mcom_odd_index_free.restype = None; L.mcom_odd_index_free.argtypes = [vp, vp]
    L.mcom_odd_index_size.restype = u64; L.mcom_odd_index_size.argtypes = [vp]
    L.mcom_odd_index_copy.restype = i32; L.mcom_odd_index_copy.argtypes = [vp, vp, vp]
    L.mcom_odd_align.restype = i32; L.mcom_odd_align.argtypes = [vp, vp, vp, u64, vp, vp, u64, vp]
    L.mcom_odd_align_encode.restype = i32; L.mcom_odd_align_encode.argtypes = [vp, vp, vp, vp, u64, vp, u64, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64)]
    L.mcom_odd_align_decode.restype = i32; L.mcom_odd_align_decode.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, u64, vp, C.POINTER(u32)]
    L.mcom_bwt_bound.restype = u64; L.mcom_bwt_bound.argtypes = [u64]
    L.mcom_bwt_encode.restype = i32; L.mcom_bwt_encode.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
    L.mcom_bwt_decode.restype = i32; L.mcom_bwt_decode.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
    L.mcom_synth_reads.restype = i32
    L.mcom_synth_reads.argtypes = [vp, u64, u64, i32, i32, C.c_double, u64, u64, vp, sz]
    L.mcom_synth_reads_genome.restype = i32
    L.mcom_synth_reads_genome.argtypes = [vp, u64, u64, i32, i32, C.c_double, i32, u64, u64, vp, sz]
    _lib = L
    return L


def words_per_read(L: int) -> int:
    return (2 * L + 63) // 64


def _torch():
    import torch
    return torch


class Context:
    """One context per process / GPU (mcom_ctx).  All tensors must live on this context's device."""

    def __init__(self, device: int = 0, stream=None):
        torch = _torch()
        if not torch.cuda.is_available():
            raise McomError("no GPU visible: the minicom_amd product path has no CPU fallback")
        self.lib = load_library()
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self._stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        h = C.c_void_p()
        rc = self.lib.mcom_create(C.byref(h), device, C.c_void_p(self._stream.cuda_stream))
        if rc:
            raise McomError(f"mcom_create failed ({rc})")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.lib.mcom_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers
    def _check(self, rc: int):
        if rc:
            raise McomError(f"mcom error {rc}: {self.lib.mcom_last_error(self._h).decode()}")

    def _p(self, t, dtype=None):
        if t is None:
            return C.c_void_p(0)
        assert t.is_cuda and t.is_contiguous(), "device, contiguous tensors only"
        if dtype is not None:
            assert t.dtype == dtype, (t.dtype, dtype)
        return C.c_void_p(t.data_ptr())

    def sync(self):
        self._check(self.lib.mcom_sync(self._h))

    def empty_records(self, n: int):
        torch = _torch()
        return torch.empty((n, 2), dtype=torch.int64, device=self.device)  # mm128_t = 2 x u64, viewed as int64

    # -- include/mcom.h entry points
    def process_reads(self, ascii_, L: int, k: int, e: int = 4, rid0: int = 0, want_nmask: bool = False):
        """mcom_process_reads.  ascii_: uint8 [n, pitch] on the device.  Returns dict of device tensors."""
        torch = _torch()
        n, pitch = ascii_.shape
        W = words_per_read(L)
        packed = torch.empty((n, W), dtype=torch.int64, device=self.device)
        cls = torch.empty(n, dtype=torch.uint8, device=self.device)
        ncnt = torch.empty(n, dtype=torch.int16, device=self.device)
        nmask = torch.empty((n, (L + 63) // 64), dtype=torch.int64, device=self.device) if want_nmask else None
        rec = self.empty_records(n)
        self._check(self.lib.mcom_process_reads(self._h, self._p(ascii_, torch.uint8), pitch, n, L, k, e, rid0,
                                                self._p(packed), self._p(cls), self._p(ncnt), self._p(nmask), self._p(rec)))
        return {"packed": packed, "cls": cls, "ncnt": ncnt, "nmask": nmask, "rec": rec}

    def process_reads_packed(self, in_packed, in_nmask, L: int, k: int, e: int = 4, rid0: int = 0, in_place: bool = False):
        """mcom_process_reads_packed: reads as a packing parser sends them (int64 [n, W] codes with 0 at an N, int64 [n, ceil(L/64)] N flags)."""
        torch = _torch()
        n = int(in_packed.shape[0])
        packed = in_packed if in_place else torch.empty_like(in_packed)
        nmask = in_nmask if in_place else torch.empty_like(in_nmask)
        cls = torch.empty(n, dtype=torch.uint8, device=self.device)
        ncnt = torch.empty(n, dtype=torch.int16, device=self.device)
        rec = self.empty_records(n)
        self._check(self.lib.mcom_process_reads_packed(self._h, self._p(in_packed, torch.int64), self._p(in_nmask, torch.int64), n, L, k, e, rid0,
                                                       self._p(packed), self._p(cls), self._p(ncnt), self._p(nmask), self._p(rec)))
        return {"packed": packed, "cls": cls, "ncnt": ncnt, "nmask": nmask, "rec": rec}

    def special_reads(self, cls, cap: int = 1 << 20):
        """mcom_special_reads: the reads of another class than 0 as (rid << 8 | class), in no particular order.  Returns (list int64 [min(count, cap)], count)."""
        torch = _torch()
        n = int(cls.shape[0])
        out = torch.empty(max(cap, 1), dtype=torch.int64, device=self.device)
        cnt = torch.zeros(2, dtype=torch.int32, device=self.device)
        self._check(self.lib.mcom_special_reads(self._h, self._p(cls, torch.uint8), n, self._p(out), cap, self._p(cnt)))
        self.sync()
        c = int(cnt[0].item())
        return out[: min(c, cap)], c

    def sketch_reads(self, packed, L: int, k: int, rids=None, rid0: int = 0, out=None):
        """mcom_sketch_reads.  packed: int64 [N, W]; rids: optional int32 [n] row selector."""
        torch = _torch()
        n = int(rids.shape[0]) if rids is not None else int(packed.shape[0])
        rec = out if out is not None else self.empty_records(n)
        self._check(self.lib.mcom_sketch_reads(self._h, self._p(packed, torch.int64),
                                               self._p(rids, torch.int32) if rids is not None else C.c_void_p(0),
                                               n, L, k, rid0, self._p(rec)))
        return rec

    def hash64(self, kmers, k: int):
        """mcom_hash64_batch: hash64 (sketch.c:27-37) of int64 k-mers."""
        torch = _torch()
        out = torch.empty_like(kmers)
        self._check(self.lib.mcom_hash64_batch(self._h, self._p(kmers, torch.int64), int(kmers.shape[0]), k, self._p(out)))
        return out

    def encode_byte(self, rows, cg, contig, pos, dirs, L: int):
        """mcom_encode_byte: the cost test of kthread_hash_realign.c:283-314 for (read row, contig window) pairs."""
        torch = _torch()
        n = int(rows.shape[0])
        ok = torch.empty(max(n, 1), dtype=torch.uint8, device=self.device)
        self._check(self.lib.mcom_encode_byte(self._h, self._p(rows, torch.int64), self._p(cg["cbits"]), self._p(cg["coff"]), self._p(contig, torch.int32),
                                              self._p(pos, torch.int32), self._p(dirs, torch.uint8), n, L, self._p(ok)))
        return ok[:n]

    def radix_sort_128x(self, rec):
        """mcom_radix_sort_128x: in place, by x ascending, stable."""
        torch = _torch()
        self._check(self.lib.mcom_radix_sort_128x(self._h, self._p(rec, torch.int64), int(rec.shape[0])))
        return rec

    def counter(self, name: str) -> int:
        self.lib.mcom_counter.restype = C.c_uint64; self.lib.mcom_counter.argtypes = [C.c_void_p, C.c_char_p]
        return int(self.lib.mcom_counter(self._h, name.encode()))

    def set_segment_capacity(self, records: int):
        """Test hook of mcom_sort_group: segments above `records` go through the nine-pass fallback (0 = default 4096)."""
        self.lib.mcom_set_segment_capacity.restype = C.c_int; self.lib.mcom_set_segment_capacity.argtypes = [C.c_void_p, C.c_uint32]
        self._check(self.lib.mcom_set_segment_capacity(self._h, records))

    def set_index_capacity(self, entries: int):
        """Test hook of mcom_cindex_build: partitions above `entries` use the scattered placement (negative = default)."""
        self.lib.mcom_set_index_capacity.restype = C.c_int; self.lib.mcom_set_index_capacity.argtypes = [C.c_void_p, C.c_int]
        self._check(self.lib.mcom_set_index_capacity(self._h, entries))

    def set_sketch_kernel(self, wave_per_string):
        """Test hook of mcom_sketch_contigs: 1 / True = the wave-per-string kernel, 2 = the lane-per-string kernel with the 64-bit ring,
        0 / False = the default choice (the ring of 32-bit prefixes for odd k)."""
        self.lib.mcom_set_sketch_kernel.restype = C.c_int; self.lib.mcom_set_sketch_kernel.argtypes = [C.c_void_p, C.c_int]
        self._check(self.lib.mcom_set_sketch_kernel(self._h, int(wave_per_string)))

    def set_sketch_prefix_bits(self, bits: int):
        """Test hook: the prefix width of the prefix ring (14 by default, in 16-bit words; above 14 in 32-bit words); a few bits make prefix ties the rule."""
        self.lib.mcom_set_sketch_prefix_bits.restype = C.c_int; self.lib.mcom_set_sketch_prefix_bits.argtypes = [C.c_void_p, C.c_int]
        self._check(self.lib.mcom_set_sketch_prefix_bits(self._h, bits))

    def set_claim_route(self, route: int):
        """Test hook of mcom_claim_pairs: 0 = default (one launch, the launch-per-round loop behind it), 1 = the loop at once, 2 = the
        one-launch kernel's first barrier gives up (poison flag trips, the loop takes over), 3 = the one-launch kernel without the
        single-workgroup tail."""
        self.lib.mcom_set_claim_route.restype = C.c_int; self.lib.mcom_set_claim_route.argtypes = [C.c_void_p, C.c_int]
        self._check(self.lib.mcom_set_claim_route(self._h, route))

    def set_eval_route(self, route: int):
        """Test hook of mcom_find_next_candidates*: 0 = default (one lane per pair, candidates staged by the evaluation kernel), 1 = a flag
        per pair, a scan over the flags and k_fn_emit, 4 / 8 / 16 = the default with a group of that many lanes per pair."""
        self.lib.mcom_set_eval_route.restype = C.c_int; self.lib.mcom_set_eval_route.argtypes = [C.c_void_p, C.c_int]
        self._check(self.lib.mcom_set_eval_route(self._h, route))

    def claim_fallbacks(self) -> int:
        self.lib.mcom_claim_fallbacks.restype = C.c_int; self.lib.mcom_claim_fallbacks.argtypes = [C.c_void_p]
        return int(self.lib.mcom_claim_fallbacks(self._h))

    def set_screen_route(self, route: int):
        """Test hook of mcom_dicts_screen: 0 = default (keys binned by counter range, counted in LDS; the global-atomics kernel behind it),
        1 = the global-atomics kernel at once, 2 = regions of a few keys (every input overflows: the fall-back runs)."""
        self.lib.mcom_set_screen_route.restype = C.c_int; self.lib.mcom_set_screen_route.argtypes = [C.c_void_p, C.c_int]
        self._check(self.lib.mcom_set_screen_route(self._h, route))

    def screen_fallbacks(self) -> int:
        self.lib.mcom_screen_fallbacks.restype = C.c_int; self.lib.mcom_screen_fallbacks.argtypes = [C.c_void_p]
        return int(self.lib.mcom_screen_fallbacks(self._h))

    def set_consensus_capacity(self, members: int):
        """Test hook of the merge consensus: units that more than `members` members reach use the wave-per-tile kernel (0 = default 127)."""
        self.lib.mcom_set_consensus_capacity.restype = C.c_int; self.lib.mcom_set_consensus_capacity.argtypes = [C.c_void_p, C.c_uint32]
        self._check(self.lib.mcom_set_consensus_capacity(self._h, members))

    def sort_group(self, rec, L: int, k_orig: int, kmer: int, b: int = 14):
        """mcom_sort_group.  Returns dict(sorted, singles, members, group_off) trimmed to their counts."""
        torch = _torch()
        n = int(rec.shape[0])
        srt = self.empty_records(n)
        singles = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        sord = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        members = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        goff = torch.empty(n // 2 + 2, dtype=torch.int32, device=self.device)
        cnt = (C.c_uint64 * 4)()
        self._check(self.lib.mcom_sort_group(self._h, self._p(rec, torch.int64), n, L, k_orig, kmer, b, self._p(srt),
                                             self._p(singles), self._p(sord), self._p(members), self._p(goff), cnt))
        nv, ns, ng, nm = (int(x) for x in cnt)
        return {"sorted": srt, "n_valid": nv, "singles": singles[:ns], "single_ord": sord[:ns], "members": members[:nm], "group_off": goff[:ng + 1] if n else goff[:0],
                "n_groups": ng}

    # -- contigs
    def upload_contigs(self, refs):
        """Host list of contig strings (bytes) -> device (seq uint8, off int64 [n+1], coff int64 [n], clen int32 [n], cbits)."""
        torch = _torch()
        lens = np.array([len(r) for r in refs], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        words = (2 * lens + 63) // 64 + 1
        coff = np.concatenate([[0], np.cumsum(words)[:-1]]).astype(np.int64) if len(refs) else np.zeros(0, np.int64)
        total = int(words.sum())
        seq = torch.from_numpy(np.frombuffer(b"".join(refs) + b"\0", dtype=np.uint8).copy()).to(self.device)
        d_off = torch.from_numpy(off).to(self.device)
        d_coff = torch.from_numpy(coff).to(self.device)
        d_clen = torch.from_numpy(lens.astype(np.int32)).to(self.device)
        cbits = torch.zeros(total + 1, dtype=torch.int64, device=self.device)
        self._check(self.lib.mcom_pack_contigs(self._h, self._p(seq), self._p(d_off), self._p(d_coff), len(refs), total, self._p(cbits)))
        return {"seq": seq, "off": d_off, "coff": d_coff, "clen": d_clen, "cbits": cbits, "n": len(refs), "lens": lens}

    def unpack_contigs(self, cbits, coff, off, n: int, byte_lo: int, byte_hi: int, seq):
        """mcom_unpack_contigs: the strings of n contigs from their packed words, into seq (uint8, 16-byte aligned) at off[c]."""
        self.lib.mcom_unpack_contigs.restype = C.c_int
        self.lib.mcom_unpack_contigs.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
        self._check(self.lib.mcom_unpack_contigs(self._h, self._p(cbits), self._p(coff), self._p(off), n, byte_lo, byte_hi, self._p(seq)))

    def sketch_contigs(self, seq, off, n: int, w: int, k: int, max_per_contig: int = 0, ids=None):
        """mcom_sketch_contigs.  Returns (moff int32 [n+1], records int64 [total,2])."""
        torch = _torch()
        moff = torch.empty(n + 1, dtype=torch.int32, device=self.device)
        total = C.c_uint64(0)
        cap = max(1024, 2 * n * (max_per_contig if max_per_contig else 4))
        while True:
            out = self.empty_records(cap)
            rc = self.lib.mcom_sketch_contigs(self._h, self._p(seq), self._p(off), self._p(ids), n, w, k, max_per_contig,
                                              self._p(moff), self._p(out), cap, C.byref(total))
            if rc == -4:
                cap = int(total.value)
                continue
            self._check(rc)
            return moff, out[: int(total.value)]

    def idx_build(self, rec, k: int, b: int = 14):
        """mcom_idx_build: b > 0 reproduces the reference's bucket order, b = 0 is one stable sort by x."""
        return Index(self, rec, k, b)

    def radix_sort_128x_ref_order(self, rec):
        """mcom_radix_sort_128x_ref_order: in place, the reference's exact (unstable) element order."""
        torch = _torch()
        self._check(self.lib.mcom_radix_sort_128x_ref_order(self._h, self._p(rec, torch.int64), int(rec.shape[0])))
        return rec

    def match_pro(self, cg, a, pa, b, pb):
        torch = _torch()
        n = int(a.shape[0])
        out = torch.empty(n, dtype=torch.int32, device=self.device)
        self._check(self.lib.mcom_match_pro(self._h, self._p(cg["cbits"]), self._p(cg["coff"]), self._p(cg["clen"]),
                                            self._p(a, torch.int32), self._p(pa, torch.int32), self._p(b, torch.int32), self._p(pb, torch.int32), n, self._p(out)))
        return out

    def find_next_candidates(self, idx, query, cg, cbthr: int):
        """mcom_find_next_candidates.  Returns (pairs int64 [n_pass,2], n_pairs_tested)."""
        cnt = (C.c_uint64 * 2)()
        cap = max(1024, int(query.shape[0]))
        while True:
            out = self.empty_records(cap)
            rc = self.lib.mcom_find_next_candidates(self._h, idx._h, self._p(query), int(query.shape[0]), self._p(cg["cbits"]),
                                                    self._p(cg["coff"]), self._p(cg["clen"]), cbthr, self._p(out), cap, cnt)
            if rc == -4:
                cap = int(cnt[1])
                continue
            self._check(rc)
            return out[: int(cnt[1])], int(cnt[0])

    def minimizer_prefix_ord(self, moff, rec, ord_, m: int):
        """mcom_minimizer_prefix_ord: the first m records of contigs ord_[0 ..] (None: all, in order), concatenated.  Returns (moff2, records)."""
        torch = _torch()
        self.lib.mcom_minimizer_prefix_ord.restype = C.c_int
        self.lib.mcom_minimizer_prefix_ord.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        n = int(ord_.shape[0]) if ord_ is not None else int(moff.shape[0]) - 1
        moff2 = torch.empty(n + 1, dtype=torch.int32, device=self.device)
        out = self.empty_records(max(n * m, 1))
        tot = C.c_uint64()
        self._check(self.lib.mcom_minimizer_prefix_ord(self._h, self._p(moff, torch.int32), self._p(rec), self._p(ord_, torch.int32) if ord_ is not None else None, n, m,
                                                       self._p(moff2), self._p(out), C.byref(tot)))
        return moff2, out[: int(tot.value)]

    def find_next_candidates_ord(self, idx, rec, roff, ord_, cg, cbthr: int, first_new: int = 0, n_new: int = 0):
        """mcom_find_next_candidates_ord: queries = the records of contigs ord_[0 ..] (None: all) of a store.  Returns (pairs, n_pairs_listed)."""
        self.lib.mcom_find_next_candidates_ord.restype = C.c_int
        self.lib.mcom_find_next_candidates_ord.argtypes = [C.c_void_p] * 5 + [C.c_size_t] + [C.c_void_p] * 3 + [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
        torch = _torch()
        n = int(ord_.shape[0]) if ord_ is not None else int(roff.shape[0]) - 1
        cnt = (C.c_uint64 * 2)()
        cap = 1024
        while True:
            out = self.empty_records(cap)
            rc = self.lib.mcom_find_next_candidates_ord(self._h, idx._h, self._p(rec), self._p(roff, torch.int32), self._p(ord_, torch.int32) if ord_ is not None else None, n,
                                                        self._p(cg["cbits"]), self._p(cg["coff"]), self._p(cg["clen"]), cbthr, first_new, n_new, self._p(out), cap, cnt)
            if rc == -4:
                cap = int(cnt[1])
                continue
            self._check(rc)
            return out[: int(cnt[1])], int(cnt[0])

    # -- Stage 2
    def gather_rows(self, packed, rids, L: int):
        torch = _torch()
        n = int(rids.shape[0])
        out = torch.empty((n, words_per_read(L)), dtype=torch.int64, device=self.device)
        self._check(self.lib.mcom_gather_rows(self._h, self._p(packed, torch.int64), self._p(rids, torch.int32), n, L, self._p(out)))
        return out

    def poly_filter(self, sgbits, L: int, thr: int, nmask=None, rids=None):
        torch = _torch()
        n = int(sgbits.shape[0])
        flag = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._check(self.lib.mcom_poly_filter(self._h, self._p(sgbits, torch.int64), self._p(nmask), self._p(rids), n, L, thr, self._p(flag)))
        return flag

    def dicts_build(self, sgbits, L: int, ininumdict: int = 0):
        return Dicts(self, sgbits, L, ininumdict)

    def realign_pass(self, dicts, sgbits, sgflag, cbits, coff, woff, n_windows: int, thr: int, maxsearch: int, stats: bool = False):
        """mcom_realign_pass.  Returns (claim int64 [n_sg], stats tensor or None)."""
        torch = _torch()
        n_sg = int(sgbits.shape[0])
        claim = torch.empty(max(n_sg, 1), dtype=torch.int64, device=self.device)
        st = torch.zeros(3, dtype=torch.int64, device=self.device) if stats else None
        self._check(self.lib.mcom_realign_pass(self._h, dicts._h, self._p(sgbits, torch.int64), self._p(sgflag, torch.uint8),
                                               self._p(cbits, torch.int64), self._p(coff, torch.int64), self._p(woff, torch.int64),
                                               int(coff.shape[0]), int(n_windows), thr, maxsearch, self._p(claim), self._p(st)))
        return claim[:n_sg], st

    def cindex_build(self, cbits, coff, woff, n_windows: int, L: int, ininumdict: int = 0):
        """mcom_cindex_plan + mcom_cindex_build.  Returns (index words int64, n_parts)."""
        torch = _torch()
        ne, parts, nw = C.c_uint64(), C.c_uint64(), C.c_uint64()
        n_contigs = int(coff.shape[0])
        self._check(self.lib.mcom_cindex_plan(int(n_windows), n_contigs, L, ininumdict, C.byref(ne), C.byref(parts), C.byref(nw)))
        words = int(nw.value)
        for attempt in range(5):                                            # MCOM_E_OVERFLOW: this set's repeats need a larger extension area
            keys = torch.empty(words, dtype=torch.int64, device=self.device)
            rc = self.lib.mcom_cindex_build(self._h, self._p(cbits, torch.int64), self._p(coff, torch.int64), self._p(woff, torch.int64),
                                            n_contigs, int(n_windows), L, ininumdict, parts.value, self._p(keys), words)
            if rc != -4:
                break
            words += max(words, 8 * (int(ne.value) // 7 + 1024))
        self._check(rc)
        return keys, parts.value

    def cindex_build_shares(self, cbits, coff, woff, n_windows: int, L: int, ranks: int, ininumdict: int = 0):
        """The ONE index over all contigs cut by key into `ranks` shares, all of them built on this GPU: mcom_cindex_plan_shared,
        mcom_cindex_entries over the whole set (grouped by owning share) and mcom_cindex_place per share -- what R ranks do with an
        all-to-all of the entries in between (host/mcom_pipeline.cpp).  Returns [(index words int64, geom)] by share."""
        torch = _torch()
        u64 = C.c_uint64
        self.lib.mcom_cindex_plan_shared.restype = C.c_int
        self.lib.mcom_cindex_plan_shared.argtypes = [u64, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int] + [C.POINTER(u64)] * 4
        self.lib.mcom_cindex_entries.restype = C.c_int
        self.lib.mcom_cindex_entries.argtypes = [C.c_void_p] * 4 + [C.c_uint32] * 3 + [C.c_int, C.c_int, u64, C.c_void_p, C.c_void_p, u64, C.POINTER(u64)]
        self.lib.mcom_cindex_place.restype = C.c_int
        self.lib.mcom_cindex_place.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, u64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, u64, C.c_void_p, u64]
        n_contigs = int(coff.shape[0])
        ne, share, geom0, nw = u64(), u64(), u64(), u64()
        self._check(self.lib.mcom_cindex_plan_shared(int(n_windows), n_contigs, L, ininumdict, ranks, 0, C.byref(ne), C.byref(share), C.byref(geom0), C.byref(nw)))
        cap = int(ne.value) + 1
        key = torch.empty(cap, dtype=torch.int32, device=self.device)
        slot = torch.empty(cap, dtype=torch.int64, device=self.device)
        counts = (u64 * ranks)()
        self._check(self.lib.mcom_cindex_entries(self._h, self._p(cbits, torch.int64), self._p(coff, torch.int64), self._p(woff, torch.int64), n_contigs, 0, n_contigs,
                                                 L, ininumdict, geom0.value, self._p(key), self._p(slot), cap, counts))
        out, at = [], 0
        for q in range(ranks):
            g, nwq = u64(), u64()
            self._check(self.lib.mcom_cindex_plan_shared(int(n_windows), n_contigs, L, ininumdict, ranks, q, C.byref(ne), C.byref(share), C.byref(g), C.byref(nwq)))
            n = int(counts[q])
            words = int(nwq.value)
            for attempt in range(5):                                        # MCOM_E_OVERFLOW: a larger extension area (place overwrites its input: copies)
                k, sl = key[at:at + n].clone(), slot[at:at + n].clone()
                kt, st = torch.empty(n + 1, dtype=torch.int32, device=self.device), torch.empty(n + 1, dtype=torch.int64, device=self.device)
                keys = torch.empty(words, dtype=torch.int64, device=self.device)
                rc = self.lib.mcom_cindex_place(self._h, self._p(k), self._p(sl), n, 0, self._p(kt), self._p(st), L, ininumdict, g.value, self._p(keys), words)
                if rc != -4:
                    break
                words += max(words, 8 * (int(ne.value) // 7 + 1024))
            self._check(rc)
            self.sync()
            out.append((keys, g.value))
            at += n
        return out

    def set_lookup_route(self, route: int):
        """Test hook of the Stage-2 lookups over a share of the keys: 0 = default (a thread per owned task, k_realign_owned), 1 = several
        (direction, dictionary) pairs per lane of the whole-index kernel."""
        self.lib.mcom_set_lookup_route.restype = C.c_int; self.lib.mcom_set_lookup_route.argtypes = [C.c_void_p, C.c_int]
        self._check(self.lib.mcom_set_lookup_route(self._h, route))

    def dicts_eligible(self, dicts, sgbits, maxsearch: int):
        torch = _torch()
        el = torch.zeros(max(int(sgbits.shape[0]), 1), dtype=torch.int32, device=self.device)
        self._check(self.lib.mcom_dicts_eligible(self._h, dicts._h, self._p(sgbits, torch.int64), maxsearch, self._p(el)))
        return el

    def dicts_screen(self, sgbits, L: int, maxsearch: int, ininumdict: int = 0) -> bool:
        """mcom_dicts_screen: False proves that no dictionary bin exceeds maxsearch."""
        torch = _torch()
        out = C.c_int(0)
        self._check(self.lib.mcom_dicts_screen(self._h, self._p(sgbits, torch.int64), int(sgbits.shape[0]), L, ininumdict, maxsearch, C.byref(out)))
        return bool(out.value)

    def realign_pass_reads(self, cindex, sgbits, sgflag, cbits, coff, woff, L: int, thr: int, ininumdict: int = 0, elig=None,
                           stats: bool = False):
        """mcom_realign_pass_reads.  cindex = cindex_build's result.  Returns (claim int64 [n_sg], stats or None)."""
        torch = _torch()
        keys, lg = cindex
        n_sg = int(sgbits.shape[0])
        claim = torch.empty(max(n_sg, 1), dtype=torch.int64, device=self.device)
        st = torch.zeros(3, dtype=torch.int64, device=self.device) if stats else None
        self._check(self.lib.mcom_realign_pass_reads(self._h, self._p(keys), lg, self._p(sgbits, torch.int64),
                                                     self._p(sgflag, torch.uint8), self._p(elig), n_sg, self._p(cbits, torch.int64),
                                                     self._p(coff, torch.int64), self._p(woff, torch.int64), int(coff.shape[0]), L,
                                                     ininumdict, thr, self._p(claim), self._p(st)))
        return claim[:n_sg], st

    # -- the device-resident contig set (include/mcom.h, "the contig set of combine_cluster")
    def scan_u64(self, x):
        torch = _torch()
        out = torch.empty_like(x)
        self._check(self.lib.mcom_scan_u64(self._h, self._p(x, torch.int64), self._p(out), int(x.shape[0])))
        return out

    def contig_layout(self, soff):
        """mcom_contig_layout.  Returns (coff_words int64 [n+1], clen int32 [n], total_words)."""
        torch = _torch()
        n = int(soff.shape[0]) - 1
        coff = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        clen = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        tw = C.c_uint64()
        self._check(self.lib.mcom_contig_layout(self._h, self._p(soff, torch.int64), n, self._p(coff), self._p(clen), C.byref(tw)))
        return coff, clen[:n], int(tw.value)

    def group_consensus(self, packed, members, goff, L: int, k_orig: int, e: int, stride=None):
        """mcom_group_consensus.  members is rewritten in place.  Returns dict(keep, nkept, sv, reflen, refs, stride).
        stride: bytes between two groups' strings in refs (None: 2L rounded up to 16; one that is no multiple of 4 keeps every group
        away from the bit-sliced kernel)."""
        torch = _torch()
        ng, nm = int(goff.shape[0]) - 1, int(members.shape[0])
        stride = (2 * L + 15) & ~15 if stride is None else int(stride)
        assert stride >= 0
        o = dict(keep=torch.empty(max(nm, 1), dtype=torch.uint8, device=self.device), nkept=torch.empty(max(ng, 1), dtype=torch.int32, device=self.device),
                 sv=torch.empty(max(ng, 1), dtype=torch.int16, device=self.device), reflen=torch.empty(max(ng, 1), dtype=torch.int16, device=self.device),
                 refs=torch.zeros(max(ng, 1) * stride + 16, dtype=torch.uint8, device=self.device), stride=stride)
        self._check(self.lib.mcom_group_consensus(self._h, self._p(packed, torch.int64), self._p(members, torch.int64), self._p(goff, torch.int32), ng, L, k_orig, e,
                                                  self._p(o["keep"]), self._p(o["nkept"]), self._p(o["sv"]), self._p(o["reflen"]), self._p(o["refs"]), stride))
        return o

    def groups_to_contigs(self, members, goff, gc, cap_chars: int, cap_members: int, cap_contigs: int):
        """mcom_groups_to_contigs into a fresh set.  Returns dict(seq, soff, mem, moff, rej_rid, rej_group, counts)."""
        torch = _torch()
        ng = int(goff.shape[0]) - 1
        seq = torch.zeros(cap_chars + 16, dtype=torch.uint8, device=self.device)
        soff = torch.zeros(cap_contigs + 2, dtype=torch.int64, device=self.device)
        mem = torch.zeros(cap_members + 1, dtype=torch.int64, device=self.device)
        moff = torch.zeros(cap_contigs + 2, dtype=torch.int64, device=self.device)
        rr = torch.zeros(int(members.shape[0]) + 1, dtype=torch.int32, device=self.device)
        rg = torch.zeros(int(members.shape[0]) + 1, dtype=torch.int32, device=self.device)
        cnt = (C.c_uint64 * 4)()
        self._check(self.lib.mcom_groups_to_contigs(self._h, self._p(members, torch.int64), self._p(goff, torch.int32), ng, self._p(gc["keep"]), self._p(gc["nkept"]),
                                                    self._p(gc["sv"]), self._p(gc["reflen"]), self._p(gc["refs"]), gc["stride"], 0, 0, 0, self._p(seq), cap_chars,
                                                    self._p(soff), self._p(mem), cap_members, self._p(moff), cap_contigs + 1, self._p(rr), self._p(rg),
                                                    int(members.shape[0]), cnt))
        nc, nch, nmm, nrj = (int(v) for v in cnt)
        return dict(seq=seq[:nch], soff=soff[:nc + 1], mem=mem[:nmm], moff=moff[:nc + 1], rej_rid=rr[:nrj], rej_group=rg[:nrj], counts=(nc, nch, nmm, nrj))

    def merge_members(self, mem, moff, jobs, L: int, key_bits: int):
        """mcom_merge_members.  jobs: int32 [nj, 4].  Returns (jm, jmoff, jroff, totals)."""
        torch = _torch()
        nj = int(jobs.shape[0])
        jm = torch.empty(int(mem.shape[0]) + 1, dtype=torch.int64, device=self.device)
        jmoff = torch.empty(nj + 1, dtype=torch.int64, device=self.device)
        jroff = torch.empty(nj + 1, dtype=torch.int64, device=self.device)
        tot = (C.c_uint64 * 3)()
        self._check(self.lib.mcom_merge_members(self._h, self._p(mem, torch.int64), self._p(moff, torch.int64), self._p(jobs, torch.int32), nj, L, key_bits,
                                                self._p(jm), self._p(jmoff), self._p(jroff), tot))
        return jm[: int(tot[0])], jmoff, jroff, tuple(int(v) for v in tot)

    def merge_consensus_jobs(self, packed, jm, jmoff, jroff, total_chars: int, L: int, jobs=None, seq=None, soff=None):
        torch = _torch()
        nj = int(jmoff.shape[0]) - 1
        refs = torch.zeros(total_chars + 16, dtype=torch.uint8, device=self.device)
        self._check(self.lib.mcom_merge_consensus_jobs(self._h, self._p(packed, torch.int64), self._p(jm, torch.int64), self._p(jmoff, torch.int64),
                                                       self._p(jroff, torch.int64), nj, total_chars, L, self._p(refs), self._p(jobs), self._p(seq), self._p(soff)))
        self.sync()
        return refs[:total_chars]

    def contigs_carry(self, seq, soff, mem, moff, flag, nj: int, seq2, soff2, mem2, moff2):
        """mcom_contigs_carry: appends the unflagged contigs behind the nj merged ones already in the *2 arrays."""
        torch = _torch()
        n = int(soff.shape[0]) - 1
        nkeep = int((flag == 0).sum())
        keepidx = torch.empty(max(nkeep, 1), dtype=torch.int32, device=self.device)
        tot = (C.c_uint64 * 2)()
        self._check(self.lib.mcom_contigs_carry(self._h, self._p(seq), self._p(soff, torch.int64), self._p(mem, torch.int64), self._p(moff, torch.int64), n,
                                                self._p(flag, torch.uint8), nj, nkeep, self._p(seq2), self._p(soff2, torch.int64), self._p(mem2, torch.int64),
                                                self._p(moff2, torch.int64), self._p(keepidx), tot))
        return keepidx[:nkeep], (int(tot[0]), int(tot[1]))

    def order_next(self, ord_, n: int, flag, first_new: int, nj: int):
        """mcom_order_next: the list of the next merge round.  ord_ int32 [n] or None (0 .. n-1), flag uint8 indexed by contig."""
        torch = _torch()
        self.lib.mcom_order_next.restype = C.c_int
        self.lib.mcom_order_next.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint64)]
        out = torch.empty(max(n + nj, 1), dtype=torch.int32, device=self.device)
        nk = C.c_uint64()
        self._check(self.lib.mcom_order_next(self._h, self._p(ord_, torch.int32) if ord_ is not None else None, n, self._p(flag, torch.uint8) if flag is not None else None,
                                             first_new, nj, self._p(out), C.byref(nk)))
        return out[: nj + int(nk.value)], int(nk.value)

    def contigs_gather(self, seq, soff, mem, moff, idx):
        """mcom_contigs_gather: contigs idx[...] of a set as a set of their own.  Returns (seq2, soff2, mem2, moff2)."""
        torch = _torch()
        self.lib.mcom_contigs_gather.restype = C.c_int
        self.lib.mcom_contigs_gather.argtypes = [C.c_void_p] * 6 + [C.c_size_t] + [C.c_void_p] * 4 + [C.POINTER(C.c_uint64)]
        k = int(idx.shape[0])
        seq2 = torch.empty(int(seq.shape[0]) + 16, dtype=torch.uint8, device=self.device)
        mem2 = torch.empty(int(mem.shape[0]) + 1, dtype=torch.int64, device=self.device)
        soff2 = torch.empty(k + 1, dtype=torch.int64, device=self.device); moff2 = torch.empty(k + 1, dtype=torch.int64, device=self.device)
        tot = (C.c_uint64 * 2)()
        self._check(self.lib.mcom_contigs_gather(self._h, self._p(seq), self._p(soff, torch.int64), self._p(mem, torch.int64), self._p(moff, torch.int64),
                                                 self._p(idx, torch.int32), k, self._p(seq2), self._p(soff2), self._p(mem2), self._p(moff2), tot))
        return seq2[: int(tot[0])], soff2, mem2[: int(tot[1])], moff2

    def offsets_append(self, rel, base: int, dst, at: int):
        """mcom_offsets_append / _u32: dst[at + j] = base + rel[j] for the n + 1 entries of rel."""
        torch = _torch()
        n = int(rel.shape[0]) - 1
        if rel.dtype == torch.int64:
            self.lib.mcom_offsets_append.restype = C.c_int; self.lib.mcom_offsets_append.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p]
            self._check(self.lib.mcom_offsets_append(self._h, self._p(rel), n, base, C.c_void_p(dst.data_ptr() + 8 * at)))
        else:
            self.lib.mcom_offsets_append_u32.restype = C.c_int; self.lib.mcom_offsets_append_u32.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
            self._check(self.lib.mcom_offsets_append_u32(self._h, self._p(rel, torch.int32), n, base, C.c_void_p(dst.data_ptr() + 4 * at)))

    def members_finalize(self, mem, moff, passes, key_bits: int):
        """mcom_members_finalize.  mem int64 [M], moff int64 [n+1]; passes: list of (contig int32 [k], member int64 [k]).
        Returns (mem2 int64, moff2 int64 [n+1])."""
        torch = _torch()
        n = int(moff.shape[0]) - 1
        m = len(passes)
        total = int(mem.shape[0]) + sum(int(c.shape[0]) for c, _ in passes)
        mem2 = torch.empty(max(total, 1), dtype=torch.int64, device=self.device)
        moff2 = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        ac = (C.c_void_p * max(m, 1))(*[self._p(c, torch.int32).value if c.shape[0] else None for c, _ in passes])
        am = (C.c_void_p * max(m, 1))(*[self._p(v, torch.int64).value if v.shape[0] else None for _, v in passes])
        an = (C.c_uint64 * max(m, 1))(*[int(c.shape[0]) for c, _ in passes])
        self._check(self.lib.mcom_members_finalize(self._h, self._p(mem, torch.int64), self._p(moff, torch.int64), n, int(mem.shape[0]), ac, am, an, m, key_bits,
                                                   self._p(mem2), self._p(moff2)))
        return mem2[:total], moff2

    def compact_live(self, ids, flag):
        """mcom_compact_live: the ids whose flag is zero, in order."""
        torch = _torch()
        n = int(ids.shape[0])
        out = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        cnt = C.c_uint64()
        self._check(self.lib.mcom_compact_live(self._h, self._p(ids, torch.int32), self._p(flag, torch.uint8), n, self._p(out), C.byref(cnt)))
        return out[: int(cnt.value)]

    def window_layout(self, soff, L: int):
        """mcom_window_layout.  Returns (woff int64 [n+1], n_windows, longest contig)."""
        torch = _torch()
        n = int(soff.shape[0]) - 1
        woff = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        nw, ml = C.c_uint64(), C.c_uint64()
        self._check(self.lib.mcom_window_layout(self._h, self._p(soff, torch.int64), n, L, self._p(woff), C.byref(nw), C.byref(ml)))
        return woff, int(nw.value), int(ml.value)

    def records_carry(self, rec, roff, keepidx, first_id: int, base: int, rec2, roff2):
        torch = _torch()
        tot = C.c_uint64()
        self._check(self.lib.mcom_records_carry(self._h, self._p(rec), self._p(roff, torch.int32), self._p(keepidx, torch.int32), int(keepidx.shape[0]), first_id, base,
                                                self._p(rec2), int(rec2.shape[0]), self._p(roff2, torch.int32), C.byref(tot)))
        return int(tot.value)

    def resketch_merged(self, jobs, soff, rec, roff, seq2, soff2, merged_chars: int, w: int, k: int):
        """mcom_resketch_merged.  Returns (roff2 int32 [nj+1], records int64 [total,2], bases sketched)."""
        torch = _torch()
        nj = int(jobs.shape[0])
        roff2 = torch.empty(nj + 1, dtype=torch.int32, device=self.device)
        tot, sk = C.c_uint64(), C.c_uint64()
        cap = max(1024, merged_chars // 8 + nj)
        while True:
            out = self.empty_records(cap)
            rc = self.lib.mcom_resketch_merged(self._h, self._p(jobs, torch.int32), nj, self._p(soff), self._p(rec), self._p(roff, torch.int32),
                                               self._p(seq2), self._p(soff2), merged_chars, w, k, self._p(roff2), self._p(out), cap,
                                               C.byref(tot), C.byref(sk))
            if rc == -4 and int(tot.value) > cap:
                cap = int(tot.value)
                continue
            self._check(rc)
            return roff2, out[: int(tot.value)], int(sk.value)

    def claim_pairs(self, pairs, n_contigs: int, max_rounds: int = 4096):
        """mcom_claim_pairs.  pairs: int64 [n, 2] records in visiting order.  Returns (jobs int32 [nj, 4], flag uint8 [n_contigs], rounds)."""
        torch = _torch()
        n = int(pairs.shape[0])
        jobs = torch.empty((max(n_contigs // 2 + 1, 1), 4), dtype=torch.int32, device=self.device)
        flag = torch.empty(max(n_contigs, 1), dtype=torch.uint8, device=self.device)
        nj, rounds = C.c_uint64(), C.c_int()
        self._check(self.lib.mcom_claim_pairs(self._h, self._p(pairs), n, n_contigs, max_rounds, self._p(jobs), self._p(flag), C.byref(nj), C.byref(rounds)))
        return jobs[: nj.value], flag[:n_contigs], rounds.value

    def claims_resolve(self, claim, rids, n_contigs: int, flag):
        """mcom_claims_resolve.  flag is updated in place; returns (contig int32 [nwon], member int64 [nwon])."""
        torch = _torch()
        n = int(claim.shape[0])
        ac = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        am = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        nw = C.c_uint64()
        self._check(self.lib.mcom_claims_resolve(self._h, self._p(claim, torch.int64), self._p(rids, torch.int32), n, n_contigs,
                                                 self._p(flag, torch.uint8), self._p(ac), self._p(am), C.byref(nw)))
        return ac[:nw.value], am[:nw.value]

    def synth_reads(self, seed: int, n_reads: int, L: int, coverage: int = 30, sub_rate: float = 0.005,
                    first: int = 0, count: int | None = None, pitch: int | None = None, genome: str = "uniform"):
        """mcom_synth_reads_genome; genome: "uniform" or "repeats" (device generator only)."""
        torch = _torch()
        if count is None:
            count = n_reads - first
        pitch = pitch or L
        out = torch.empty((count, pitch), dtype=torch.uint8, device=self.device)
        self._check(self.lib.mcom_synth_reads_genome(self._h, seed, n_reads, L, coverage, sub_rate, {"uniform": 0, "repeats": 1}[genome], first, count, self._p(out), pitch))
        return out

    # ---- decoder (csrc/decode.hip).  uint64 / uint32 arrays travel as int64 / int32 tensors, bytes as uint8 -------------------
    def _dflag(self):
        torch = _torch()
        return torch.zeros(1, dtype=torch.int32, device=self.device)

    def decode_walk_headers(self, bpos: np.ndarray):
        """mcom_decode_walk_headers on a host uint8 array.  Returns moff (uint64 [n_contigs + 1]); McomError when the chain leaves the file."""
        b = np.ascontiguousarray(bpos, dtype=np.uint8)
        nc, nm = C.c_uint64(), C.c_uint64()
        if self.lib.mcom_decode_walk_headers(b.ctypes.data, b.size, None, 0, C.byref(nc), C.byref(nm)):
            raise McomError("beg_pos.bin: a contig's deltas leave the file")
        moff = np.zeros(nc.value + 1, dtype=np.uint64)
        if self.lib.mcom_decode_walk_headers(b.ctypes.data, b.size, moff.ctypes.data, nc.value, C.byref(nc), C.byref(nm)):
            raise McomError("beg_pos.bin: a contig's deltas leave the file")
        return moff

    def decode_line_index(self, text):
        """mcom_decode_line_index.  text: uint8 device tensor.  Returns (line_start int64 [n_lines + 1], flag)."""
        torch = _torch()
        n = C.c_uint64()
        flag = self._dflag()
        nb = int(text.shape[0])
        self._check(self.lib.mcom_decode_line_index(self._h, self._p(text, torch.uint8) if nb else None, nb, None, 0, C.byref(n), self._p(flag)))
        start = torch.empty(n.value + 1, dtype=torch.int64, device=self.device)
        self._check(self.lib.mcom_decode_line_index(self._h, self._p(text, torch.uint8) if nb else None, nb, self._p(start), n.value, C.byref(n), self._p(flag)))
        self.sync()
        return start, int(flag.item())

    def decode_member_table(self, bpos, moff, L: int):
        """mcom_decode_member_table.  bpos: uint8 device tensor, moff: int64 device tensor [n_contigs + 1] (decode_walk_headers).
        Returns (cid int32 [n], pos int32 [n], coff int64 [n_contigs + 1], ref_bases, flag)."""
        torch = _torch()
        nc = int(moff.shape[0]) - 1
        nm = int(moff[-1].item())
        cid = torch.zeros(max(nm, 1), dtype=torch.int32, device=self.device)
        pos = torch.zeros(max(nm, 1), dtype=torch.int32, device=self.device)
        coff = torch.zeros(nc + 1, dtype=torch.int64, device=self.device)
        rb = C.c_uint64()
        flag = self._dflag()
        self._check(self.lib.mcom_decode_member_table(self._h, self._p(bpos, torch.uint8) if bpos.numel() else None, int(bpos.shape[0]), self._p(moff, torch.int64), nc, nm, L,
                                                      self._p(cid), self._p(pos), self._p(coff), C.byref(rb), self._p(flag)))
        return cid[:nm], pos[:nm], coff, int(rb.value), int(flag.item())

    def decode_list_ids(self, delta):
        torch = _torch()
        n = int(delta.shape[0])
        dest = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        self._check(self.lib.mcom_decode_list_ids(self._h, self._p(delta, torch.int32) if n else None, n, self._p(dest)))
        self.sync()
        return dest[:n]

    def decode_member_ids(self, ids, moff, cid, pos):
        torch = _torch()
        n = int(ids.shape[0])
        dest = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        if n:
            self._check(self.lib.mcom_decode_member_ids(self._h, self._p(ids, torch.int32), n, self._p(moff, torch.int64), self._p(cid.contiguous(), torch.int32),
                                                        self._p(pos.contiguous(), torch.int32), self._p(dest)))
        self.sync()
        return dest[:n]

    def decode_pe_dest(self, fbits, n: int, peids, zero_base: int, half: int, bit0: int = 0):
        """mcom_decode_pe_dest.  Returns (dest int64 [n], ones, flag); a refused row is -1."""
        torch = _torch()
        dest = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        ones = C.c_uint64()
        flag = self._dflag()
        self._check(self.lib.mcom_decode_pe_dest(self._h, self._p(fbits, torch.uint8) if fbits.numel() else None, int(fbits.shape[0]), bit0, n,
                                                 self._p(peids, torch.int32) if peids.numel() else None, int(peids.shape[0]), zero_base, half, self._p(dest), C.byref(ones), self._p(flag)))
        return dest[:n], int(ones.value), int(flag.item())

    def decode_reads(self, n: int, L: int, n_rows: int, text=None, line_start=None, verbatim=False, ref=None, ref_const="A", cid=None, pos=None, coff=None,
                     dirbits=None, dest=None, dest0: int = 0, out=None, seen=None, check=True):
        """mcom_decode_check_lines + mcom_decode_reads into `out` (uint8 [n_rows * (L + 1)], made when None).  Returns (out, flag)."""
        torch = _torch()
        if out is None:
            out = torch.zeros(n_rows * (L + 1), dtype=torch.uint8, device=self.device)
        flag = self._dflag()
        src, ptr, keep = self._decode_src(n, text, line_start, verbatim, ref, ref_const, cid, pos, coff, dirbits)
        if check and src.d_text:
            self._check(self.lib.mcom_decode_check_lines(self._h, src.d_text, src.text_bytes, src.d_line_start, n, L, int(verbatim), self._p(flag)))
        self._check(self.lib.mcom_decode_reads(self._h, C.byref(src), n, L, ptr(dest, torch.int64), dest0, self._p(out), n_rows, self._p(seen) if seen is not None else None, self._p(flag)))
        self.sync()
        return out, int(flag.item())

    def _decode_src(self, n, text, line_start, verbatim, ref, ref_const, cid, pos, coff, dirbits):
        """the mcom_decode_src of decode_reads' keyword arguments: (src, ptr, keep) -- ptr(tensor, dtype) gives a device address and keeps the
        tensor alive in `keep`, which the caller holds until the call has been synchronised"""
        torch = _torch()
        src = DecodeSrc()
        keep = []
        def ptr(t, dt):
            if t is None or t.numel() == 0:
                return None
            t = t.contiguous(); keep.append(t)
            assert t.is_cuda and t.dtype == dt, (t.dtype, dt)
            return t.data_ptr()
        src.d_text = ptr(text, torch.uint8) if text is not None and line_start is not None else None
        if text is not None and line_start is not None and src.d_text is None and n:       # an empty text with lines asked for: one byte nobody reads
            text = torch.zeros(1, dtype=torch.uint8, device=self.device); keep.append(text); src.d_text = text.data_ptr(); src.text_bytes = 0
        else:
            src.text_bytes = int(text.shape[0]) if text is not None else 0
        src.d_line_start = ptr(line_start, torch.int64); src.verbatim = int(verbatim)
        src.d_ref = ptr(ref, torch.uint8); src.ref_bytes = int(ref.shape[0]) if ref is not None else 0; src.ref_const = ord(ref_const)
        src.d_cid = ptr(cid, torch.int32); src.d_pos = ptr(pos, torch.int32); src.d_coff = ptr(coff, torch.int64); src.n_contigs = (int(coff.shape[0]) - 1) if coff is not None else 0
        src.d_dir = ptr(dirbits, torch.uint8); src.dir_bytes = int(dirbits.shape[0]) if dirbits is not None else 0
        return src, ptr, keep

    # ---- a window of rows (`minicom -d -R`) ----
    def decode_check_dest(self, n: int, n_rows: int, dest=None, dest0: int = 0, seen=None):
        """mcom_range_check_dest over the n reads of one source: destinations dest (int64 device vector; None: dest0 + m) against n_rows
        rows.  seen: an int32 device vector of n_rows / 32 + 1 zeroed words shared by the sources of an archive (made when None).  Returns
        (flag, seen): DECODE_F_DEST for a destination >= n_rows, DECODE_F_DUP for a row named twice.  Nothing is decoded."""
        torch = _torch()
        if seen is None:
            seen = torch.zeros(n_rows // 32 + 1, dtype=torch.int32, device=self.device)
        flag = self._dflag()
        d = dest.contiguous() if dest is not None and dest.numel() else None
        self._check(self.lib.mcom_range_check_dest(self._h, self._p(d, torch.int64) if d is not None else None, dest0, n, n_rows, self._p(seen), self._p(flag)))
        self.sync()
        return int(flag.item()), seen

    def decode_reads_window(self, n: int, L: int, win_first: int, win_count: int, text=None, line_start=None, verbatim=False, ref=None, ref_const="A", cid=None, pos=None,
                            coff=None, dirbits=None, dest=None, dest0: int = 0, out=None):
        """mcom_range_decode_reads: the reads of the source (decode_reads' keyword arguments) whose destination lies in [win_first,
        win_first + win_count) to row destination - win_first of `out` (uint8, win_count * (L + 1) bytes at any address, made when None).
        Nothing else is decoded or written.  Returns (out, flag)."""
        torch = _torch()
        if out is None:
            out = torch.zeros(max(win_count * (L + 1), 1), dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < win_count * (L + 1):
            raise McomError("decode_reads_window: out must hold %d rows of %d + 1 bytes" % (win_count, L))
        flag = self._dflag()
        src, ptr, keep = self._decode_src(n, text, line_start, verbatim, ref, ref_const, cid, pos, coff, dirbits)
        self._check(self.lib.mcom_range_decode_reads(self._h, C.byref(src), n, L, ptr(dest, torch.int64), dest0, win_first, win_count, out.data_ptr(), self._p(flag)))
        self.sync()
        return out, int(flag.item())

    # ---- consensus agreement (`minicom -a Q[:C]`) ----
    def decode_coverage(self, cid, pos, coff, L: int, ref_bases: int, out=None):
        """mcom_agree_coverage over the member table of ONE stream set (decode_member_table).  Returns (cov uint8 [ref_bases], flag);
        out: a uint8 device tensor of at least ref_bases entries to write into instead of a fresh one."""
        torch = _torch()
        nm = int(cid.shape[0])
        cov = out if out is not None else torch.zeros(max(ref_bases, 1), dtype=torch.uint8, device=self.device)
        assert cov.is_cuda and cov.dtype == torch.uint8 and cov.is_contiguous() and cov.numel() >= ref_bases
        flag = self._dflag()
        self._check(self.lib.mcom_agree_coverage(self._h, self._p(cid.contiguous(), torch.int32) if nm else None, self._p(pos.contiguous(), torch.int32) if nm else None,
                                                  self._p(coff, torch.int64), int(coff.shape[0]) - 1, nm, L, int(ref_bases), self._p(cov), self._p(flag)))
        return (cov if out is not None else cov[:ref_bases]), int(flag.item())

    def decode_agree(self, n: int, L: int, n_rows: int, cov=None, min_cov: int = 3, text=None, line_start=None, verbatim=False, ref=None, ref_const="A", cid=None, pos=None, coff=None,
                     dirbits=None, dest=None, dest0: int = 0, mask=None, mask_pitch: int | None = None):
        """mcom_agree_mask: the sibling of decode_reads over the same source.  mask: uint8 [n_rows * mask_pitch] (made, zeroed, when None;
        mask_pitch defaults to ceil(L / 8)).  Returns (mask, flag)."""
        torch = _torch()
        mb = (L + 7) // 8
        if mask_pitch is None:
            mask_pitch = mb
        if mask is None:
            mask = torch.zeros(n_rows * mask_pitch, dtype=torch.uint8, device=self.device)
        flag = self._dflag()
        src = DecodeSrc()
        keep = []
        def ptr(t, dt):
            if t is None or t.numel() == 0:
                return None
            t = t.contiguous(); keep.append(t)
            assert t.is_cuda and t.dtype == dt, (t.dtype, dt)
            return t.data_ptr()
        src.d_text = ptr(text, torch.uint8) if text is not None and line_start is not None else None
        if text is not None and line_start is not None and src.d_text is None and n:
            text = torch.zeros(1, dtype=torch.uint8, device=self.device); keep.append(text); src.d_text = text.data_ptr(); src.text_bytes = 0
        else:
            src.text_bytes = int(text.shape[0]) if text is not None else 0
        src.d_line_start = ptr(line_start, torch.int64); src.verbatim = int(verbatim)
        src.d_ref = ptr(ref, torch.uint8); src.ref_bytes = int(ref.shape[0]) if ref is not None else 0; src.ref_const = ord(ref_const)
        src.d_cid = ptr(cid, torch.int32); src.d_pos = ptr(pos, torch.int32); src.d_coff = ptr(coff, torch.int64); src.n_contigs = (int(coff.shape[0]) - 1) if coff is not None else 0
        src.d_dir = ptr(dirbits, torch.uint8); src.dir_bytes = int(dirbits.shape[0]) if dirbits is not None else 0
        self._check(self.lib.mcom_agree_mask(self._h, C.byref(src), n, L, ptr(dest, torch.int64), dest0, n_rows, ptr(cov, torch.uint8), int(cov.shape[0]) if cov is not None else 0,
                                               int(min_cov), self._p(mask), int(mask_pitch), self._p(flag)))
        self.sync()
        return mask, int(flag.item())

    def qual_agree(self, rows, mask, Q: int, first_mask_row: int = 0, in_place: bool = False):
        """mcom_qual_agree.  rows: uint8 device matrix [n, L] with contiguous rows (any row stride >= L, any address); mask: uint8 device
        matrix [m, >= ceil(L / 8)] with contiguous rows, m >= first_mask_row + n.  Returns (the transformed matrix, the report as a dict of
        exact integers: changed, sum_abs, sum_sq, max_abs, mask_bits).  The matrix is a copy unless in_place."""
        torch = _torch()
        if rows.dim() != 2 or rows.dtype != torch.uint8 or (rows.shape[0] and rows.stride(1) != 1) or mask.dim() != 2 or mask.dtype != torch.uint8 or (mask.shape[0] and mask.stride(1) != 1):
            raise McomError("qual_agree: uint8 matrices with contiguous rows")
        n, L = int(rows.shape[0]), int(rows.shape[1])
        if first_mask_row < 0 or first_mask_row + n > int(mask.shape[0]):
            raise McomError("qual_agree: the mask has no row for every quality row")
        if not in_place:
            rows = rows.contiguous().clone()
        pitch = int(rows.stride(0)) if n > 1 else L
        mask_pitch = int(mask.stride(0)) if mask.shape[0] > 1 else int(mask.shape[1])
        rep = QualAgreeReport()
        self._check(self.lib.mcom_qual_agree(self._h, rows.data_ptr() if n else None, n, L, pitch, mask.data_ptr() if mask.numel() else None, mask_pitch, int(first_mask_row), int(Q), C.byref(rep)))
        return rows, rep.as_dict()

    # ---- the built-in entropy stage (csrc/entropy.hip) ----
    def rans_encode(self, raw, model=None, stride=1, out=None):
        """mcom_rans_encode.  raw: uint8 device tensor.  model None: chosen by estimated size; 0 stored, 1 order-0, 2 order-1 with
        `stride` 1, 2 or 4 force one.  Returns the `.rans` member as a uint8 device tensor.  out: a uint8 device tensor to write the
        member into (a slice of a larger buffer, as the container passes; its length is the room offered) instead of a fresh one."""
        torch = _torch()
        n = int(raw.shape[0])
        hint = 0 if model is None else rans_hint(model, stride)
        cap = int(out.shape[0]) if out is not None else 32 + n if model is None else int(self.lib.mcom_rans_bound(n))
        if out is None:
            out = torch.empty(cap, dtype=torch.uint8, device=self.device)
        got = C.c_uint64()
        self._check(self.lib.mcom_rans_encode(self._h, self._p(raw, torch.uint8) if n else None, n, self._p(out), cap, C.byref(got), hint))
        return out[:got.value]

    def bgzf_encode(self, raw, eof=True, out=None):
        """mcom_bgzf_encode.  raw: uint8 device tensor at any address.  Returns the BGZF members of its bytes, one
        per 65280, as a uint8 device tensor; eof=True closes them with the empty member a file ends with.  out: a uint8 device tensor to
        write into (its length is the room offered: McomError when it is too small) instead of a fresh one of mcom_bgzf_bound bytes."""
        torch = _torch()
        n = int(raw.shape[0])
        cap = int(out.shape[0]) if out is not None else int(self.lib.mcom_bgzf_bound(n))
        if out is None:
            out = torch.empty(cap, dtype=torch.uint8, device=self.device)
        got = C.c_uint64()
        self._check(self.lib.mcom_bgzf_encode(self._h, raw.data_ptr() if n else None, n, out.data_ptr(), cap, C.byref(got), 1 if eof else 0))
        return out[:got.value]

    def gzip_inflate(self, members_tensor, table, out=None):
        """mcom_gzip_inflate.  members_tensor: uint8 device tensor at any address that holds the DEFLATE payloads;
        table: numpy array of GZIP_MEMBER_DTYPE (what pipeline.gzip_walk returns), or a uint8 device tensor of the same bytes.  out: a
        uint8 device tensor to inflate into (its length is the room offered) instead of a fresh one that ends with the last slot.
        Returns (text, statuses): two uint8 device tensors, the statuses MCOM_GZIP_* per member.  McomError for a table whose payloads or
        slots leave the buffers or whose slots overlap or are out of order."""
        torch = _torch()
        import numpy as np
        if isinstance(table, np.ndarray):
            tab = np.ascontiguousarray(table, dtype=GZIP_MEMBER_DTYPE)
            n = int(tab.shape[0])
            room = int((tab["out_off"] + tab["isize"]).max()) if n else 0
            d_tab = torch.from_numpy(tab.view(np.uint8).reshape(-1).copy()).to(self.device) if n else torch.empty(0, dtype=torch.uint8, device=self.device)
        else:
            d_tab = table
            n = int(d_tab.shape[0]) // GZIP_MEMBER_DTYPE.itemsize
            room = None
        if out is None:
            if room is None:
                raise McomError("gzip_inflate: a table on the device needs `out`")
            out = torch.empty(room, dtype=torch.uint8, device=self.device)
        status = torch.zeros(max(n, 1), dtype=torch.uint8, device=self.device)
        bad, first = C.c_uint64(), C.c_uint64()
        nin, nout = int(members_tensor.shape[0]), int(out.shape[0])
        self._check(self.lib.mcom_gzip_inflate(self._h, members_tensor.data_ptr() if nin else None, nin, d_tab.data_ptr() if n else None, n,
                                               out.data_ptr() if nout else None, nout, status.data_ptr(), C.byref(bad), C.byref(first)))
        return out, status[:n]

    def rans_decode(self, member, cap=None, out=None):
        """mcom_rans_decode.  member: uint8 device tensor.  Returns the raw bytes as a uint8 device tensor; McomError for a member that is
        truncated, malformed or fails its CRC-32.  cap: room to offer (default: what the member's header asks for, at most 1 TB).
        out: a uint8 device tensor to decode into (its length is the room offered) instead of a fresh one."""
        torch = _torch()
        n = int(member.shape[0])
        if cap is None:
            head = bytes(member[:16].cpu().numpy()) if n >= 16 else b""
            cap = int.from_bytes(head[8:16], "little") if len(head) == 16 else 0
            if cap > 1 << 40:
                raise McomError("rans_decode: the header asks for %d bytes" % cap)
        if out is not None:
            cap = int(out.shape[0])
        else:
            out = torch.empty(max(cap, 1), dtype=torch.uint8, device=self.device)
        got = C.c_uint64()
        self._check(self.lib.mcom_rans_decode(self._h, self._p(member, torch.uint8) if n else None, n, self._p(out), cap, C.byref(got)))
        return out[:got.value]

    # ---- quality values (csrc/qual.hip) ----
    def qual_encode(self, rows, model=None, out=None):
        """mcom_qual_encode.  rows: uint8 device tensor [n, L] whose rows are contiguous (any row stride >= L, any address).  model
        None: chosen by estimated size, and the embedded `.rans` member where that is smaller; 0 .. 4 or "rans" force one.  Returns the
        `.mcq` member as a uint8 device tensor.  out: a uint8 device tensor to write the member into."""
        torch = _torch()
        if rows.dim() != 2 or rows.dtype != torch.uint8 or (rows.shape[0] and rows.stride(1) != 1):
            raise McomError("qual_encode: a uint8 matrix with contiguous rows")
        n, L = int(rows.shape[0]), int(rows.shape[1])
        pitch = int(rows.stride(0)) if n > 1 else L
        cap = int(out.shape[0]) if out is not None else int(self.lib.mcom_qual_bound(n, L))
        if not cap or pitch < L:
            raise McomError("qual_encode: rows of %d bytes" % L)
        if out is None:
            out = torch.empty(cap, dtype=torch.uint8, device=self.device)
        hint = 0 if model is None else 0x180 if model == "rans" else 0x100 | int(model)
        got = C.c_uint64()
        self._check(self.lib.mcom_qual_encode(self._h, rows.data_ptr() if n else None, n, L, pitch, self._p(out), cap, C.byref(got), hint))
        return out[:got.value]

    def qual_decode(self, member, out=None):
        """mcom_qual_decode.  member: uint8 device tensor.  Returns the quality matrix as a uint8 device tensor [n, L]; McomError for a
        member that is truncated, malformed or fails its CRC-32.  out: a uint8 device tensor [rows, >= L] with contiguous rows to decode
        into (its first dimension is the room offered); the result is then a view of it."""
        torch = _torch()
        n_in = int(member.shape[0])
        head = bytes(member[:64].cpu().numpy())
        n, L = C.c_uint64(), C.c_uint32()
        if self.lib.mcom_qual_info(head if head else None, n_in, C.byref(n), C.byref(L)):
            raise McomError("qual_decode: not a .mcq member")
        n, L = int(n.value), int(L.value)
        if out is None:
            out = torch.empty((max(n, 1), L), dtype=torch.uint8, device=self.device)
        if out.dim() != 2 or out.dtype != torch.uint8 or out.stride(1) != 1 or int(out.shape[1]) < L:
            raise McomError("qual_decode: out must be a uint8 matrix with contiguous rows of at least %d bytes" % L)
        pitch = int(out.stride(0)) if int(out.shape[0]) > 1 else max(L, int(out.shape[1]))
        gn, gL = C.c_uint64(), C.c_uint32()
        self._check(self.lib.mcom_qual_decode(self._h, self._p(member, torch.uint8), n_in, out.data_ptr(), pitch, int(out.shape[0]), C.byref(gn), C.byref(gL)))
        return out[:n, :L]

    def qual_decode_rows(self, member, first: int, count: int, pitch: int | None = None, out=None):
        """mcom_qual_decode_rows: rows first .. first + count - 1 of a `.mcq` member (uint8 device tensor; count
        clipped at the member's end) as a uint8 device matrix [count, L].  Only the touched segments are decoded and the member's CRC-32 is
        not checked, unless the range is the whole member.  pitch: the row stride of a fresh result (default L); out: a uint8 device matrix
        [>= count, >= L] with contiguous rows to decode into instead.  McomError for a refused member and for first > n."""
        torch = _torch()
        n_in = int(member.shape[0])
        head = bytes(member[:64].cpu().numpy())
        n, L = C.c_uint64(), C.c_uint32()
        if self.lib.mcom_qual_info(head if head else None, n_in, C.byref(n), C.byref(L)):
            raise McomError("qual_decode_rows: not a .mcq member")
        n, L = int(n.value), int(L.value)
        if first < 0 or count < 0 or first > n:
            raise McomError("qual_decode_rows: rows %d .. + %d of %d" % (first, count, n))
        count = min(int(count), n - int(first))
        if out is None:
            pitch = L if pitch is None else int(pitch)
            if pitch < L:
                raise McomError("qual_decode_rows: pitch %d below L = %d" % (pitch, L))
            out = torch.empty((max(count, 1), pitch), dtype=torch.uint8, device=self.device)
        if out.dim() != 2 or out.dtype != torch.uint8 or out.stride(1) != 1 or int(out.shape[1]) < L or int(out.shape[0]) < count:
            raise McomError("qual_decode_rows: out must be a uint8 matrix of at least %d contiguous rows of at least %d bytes" % (count, L))
        row_pitch = int(out.stride(0)) if int(out.shape[0]) > 1 else max(L, int(out.shape[1]))
        gn, gL = C.c_uint64(), C.c_uint32()
        self._check(self.lib.mcom_qual_decode_rows(self._h, self._p(member, torch.uint8), n_in, int(first), count, out.data_ptr(), row_pitch, C.byref(gn), C.byref(gL)))
        return out[:count, :L]

    GATHER_F_BOUNDS, GATHER_F_DUP = 1, 2

    def qual_gather_rows(self, rows, order, out=None):
        """mcom_qual_gather_rows.  rows: uint8 device matrix [n_src, L] with contiguous rows (any row stride >= L,
        any address); order: int32 / uint32 device vector of n_rows source row numbers.  Returns (out, flags): out row j = rows[order[j]]
        as a uint8 device matrix [n_rows, L] (out given: written into it, rows of at least L bytes), flags the OR of GATHER_F_BOUNDS (an
        entry >= n_src: its output row is left as it was) and GATHER_F_DUP (a source row named twice).  With n_rows == n_src, flags == 0
        proves a permutation."""
        torch = _torch()
        if rows.dim() != 2 or rows.dtype != torch.uint8 or (rows.shape[0] and rows.stride(1) != 1):
            raise McomError("qual_gather_rows: a uint8 matrix with contiguous rows")
        if order.dim() != 1 or order.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or (order.shape[0] > 1 and order.stride(0) != 1):
            raise McomError("qual_gather_rows: the order is a contiguous vector of 32-bit row numbers")
        n_src, L, n_rows = int(rows.shape[0]), int(rows.shape[1]), int(order.shape[0])
        pitch_in = int(rows.stride(0)) if n_src > 1 else L
        if out is None:
            out = torch.empty((n_rows, L), dtype=torch.uint8, device=self.device)
        if out.dim() != 2 or out.dtype != torch.uint8 or int(out.shape[0]) != n_rows or int(out.shape[1]) < L or (n_rows and out.stride(1) != 1):
            raise McomError("qual_gather_rows: out must be a uint8 matrix of %d rows of at least %d contiguous bytes" % (n_rows, L))
        pitch_out = int(out.stride(0)) if n_rows > 1 else max(L, int(out.shape[1]))
        flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._check(self.lib.mcom_qual_gather_rows(self._h, rows.data_ptr() if n_src else None, n_src, L, pitch_in, order.data_ptr() if n_rows else None, n_rows,
                                                   out.data_ptr() if n_rows else None, pitch_out, self._p(flag)))
        return out[:, :L], int(flag.item())

    def qual_transform(self, rows, spec, in_place: bool = False):
        """mcom_qual_transform.  rows: uint8 device matrix [n, L] with contiguous rows (any row stride >= L, any
        address); spec: a QualLossySpec or the canonical text of one (`ill8`, `thr:T:LO:HI`, `pblock:P`).  Returns (the transformed
        matrix, the report as a dict of exact integers: changed, sum_abs, sum_sq, max_abs).  The matrix is a copy unless in_place: then
        rows itself is rewritten (the bytes between its rows stay) and returned.  McomError, with rows and nothing else touched, for a
        spec the transform refuses (a byte map that is not idempotent)."""
        torch = _torch()
        if not isinstance(spec, QualLossySpec):
            from .pipeline import qual_lossy_spec
            spec = qual_lossy_spec(spec)
        if rows.dim() != 2 or rows.dtype != torch.uint8 or (rows.shape[0] and rows.stride(1) != 1):
            raise McomError("qual_transform: a uint8 matrix with contiguous rows")
        n, L = int(rows.shape[0]), int(rows.shape[1])
        if not in_place:
            rows = rows.contiguous().clone()
        pitch = int(rows.stride(0)) if n > 1 else L
        rep = QualLossyReport()
        self._check(self.lib.mcom_qual_transform(self._h, rows.data_ptr() if n else None, n, L, pitch, C.byref(spec), C.byref(rep)))
        return rows, rep.as_dict()

    @staticmethod
    def qual_pblock_tile_rows() -> int:
        """Test hook (mcom_test_qual_pblock_tile_rows): the rows of one tile of the P-block kernel"""
        return int(load_library().mcom_test_qual_pblock_tile_rows())

    # -- test hooks of the one-launch scans and the read-back of their totals (include/mcom_test.h)
    @staticmethod
    def scan_constants() -> dict:
        """mcom_test_scan_constants: threads of a workgroup, elements per thread by width, words of the ring of totals, tracked entries"""
        v = [C.c_uint32() for _ in range(5)]
        load_library().mcom_test_scan_constants(*[C.byref(x) for x in v])
        return dict(zip(("threads", "per_u32", "per_u64", "ring_words", "tracked"), (int(x.value) for x in v)))

    def n_cu(self) -> int:
        """mcom_test_n_cu: the compute units the context sizes its grids by"""
        return int(self.lib.mcom_test_n_cu(self._h))

    def scan_async(self, src, dst, n: int):
        """mcom_test_scan_u32 (int32 tensors) / mcom_scan_u64 (int64 tensors) of the first n elements of src into dst -- views at any
        element offset of a larger buffer, or the same view twice.  Does not wait for the stream."""
        torch = _torch()
        assert src.dtype == dst.dtype and src.dtype in (torch.int32, torch.int64) and int(src.shape[0]) >= n and int(dst.shape[0]) >= n
        f = self.lib.mcom_test_scan_u32 if src.dtype == torch.int32 else self.lib.mcom_scan_u64
        self._check(f(self._h, self._p(src), self._p(dst), int(n)))

    def scan_script(self, steps, d_in, d_out, n_totals: int = 0, copy_bytes: int = 0, fill: int = 0xA5):
        """mcom_test_scan_script.  steps: SCAN_STEP_DTYPE records; d_in, d_out: device tensors (the two buffers).  Returns (the library's
        error code, h_totals uint64 [n_totals], h_copy uint8 [copy_bytes]); both host arrays start out as bytes of `fill`."""
        steps = np.ascontiguousarray(steps, dtype=SCAN_STEP_DTYPE)
        tot = np.full(max(n_totals, 1), fill * 0x0101010101010101, dtype=np.uint64)
        cp = np.full(max(copy_bytes, 1), fill, dtype=np.uint8)
        rc = self.lib.mcom_test_scan_script(self._h, steps.ctypes.data, int(steps.shape[0]),
                                            self._p(d_in), d_in.numel() * d_in.element_size(), self._p(d_out), d_out.numel() * d_out.element_size(),
                                            tot.ctypes.data, n_totals, cp.ctypes.data, copy_bytes)
        return int(rc), tot[:n_totals], cp[:copy_bytes]

    def dump_read_order(self, lists, mem, half: int = 0):
        """mcom_dump_read_order.  lists: int32 device vector, the read ids of the eight lists in the decoder's order;
        mem: int64 device vector, the members in dump order (read id in the upper half).  half == 0: the read id of every entry; half > 0:
        the ids of the entries that are reads of the first file (id < half), in their order.  Returns an int32 device vector of `rows` ids."""
        torch = _torch()
        nl, nm = int(lists.shape[0]), int(mem.shape[0])
        order = torch.empty(max(int(half) if half else nl + nm, 1), dtype=torch.int32, device=self.device)
        rows = C.c_uint64()
        self._check(self.lib.mcom_dump_read_order(self._h, self._p(lists, torch.int32) if nl else None, nl, self._p(mem, torch.int64) if nm else None, nm, int(half), self._p(order), C.byref(rows)))
        return order[:min(int(rows.value), int(order.shape[0]))]

    def fastq_qualities(self, text, L: int, first_record: int = 0, out=None):
        """mcom_decode_line_index + mcom_fastq_quality_rows.  text: uint8 device tensor holding whole four-line records (every line ends
        with a newline).  Returns (rows uint8 [first_record + n_records, L], flag bits of MCOM_FASTQ_F_*, the first flagged record or
        None); rows of flagged records hold nothing valid.  out: a uint8 device matrix with contiguous rows to gather into."""
        torch = _torch()
        start, _ = self.decode_line_index(text)
        n_rec = (int(start.shape[0]) - 1) // 4
        if out is None:
            out = torch.zeros((max(first_record + n_rec, 1), L), dtype=torch.uint8, device=self.device)
        pitch = int(out.stride(0)) if int(out.shape[0]) > 1 else max(L, int(out.shape[1]))
        if out.dtype != torch.uint8 or out.stride(1) != 1 or int(out.shape[0]) < first_record + n_rec or int(out.shape[1]) < L:
            raise McomError("fastq_qualities: out must hold %d rows of %d bytes" % (first_record + n_rec, L))
        flag = torch.tensor([0, -1], dtype=torch.int32, device=self.device)
        self._check(self.lib.mcom_fastq_quality_rows(self._h, self._p(text, torch.uint8) if n_rec else None, int(text.shape[0]), self._p(start), first_record, n_rec, L,
                                                     out.data_ptr(), pitch, self._p(flag)))
        f = flag.cpu().numpy().view(np.uint32)
        return out[:first_record + n_rec, :L], int(f[0]), (None if f[1] == 0xFFFFFFFF else int(f[1]))

    def fastq_emit(self, reads, quals, first: int = 0):
        """mcom_fastq_emit.  reads, quals: uint8 device matrices [count, >= L] with contiguous rows (row strides at will): the rows of
        records first .. first + count - 1.  Returns the records `@<i+1>`, read, `+`, qualities as one uint8 device tensor."""
        torch = _torch()
        count, L = int(quals.shape[0]), int(quals.shape[1])
        if int(reads.shape[0]) != count or int(reads.shape[1]) != L or (count and (reads.stride(1) != 1 or quals.stride(1) != 1)):
            raise McomError("fastq_emit: reads and qualities of one shape, rows contiguous")
        rp = int(reads.stride(0)) if count > 1 else L
        qp = int(quals.stride(0)) if count > 1 else L
        nb = C.c_uint64()
        self._check(self.lib.mcom_fastq_emit(self._h, None, rp, None, qp, first, count, L, None, C.byref(nb)))
        out = torch.empty(max(int(nb.value), 1), dtype=torch.uint8, device=self.device)
        self._check(self.lib.mcom_fastq_emit(self._h, reads.data_ptr() if count else None, rp, quals.data_ptr() if count else None, qp, first, count, L, self._p(out), C.byref(nb)))
        return out[:nb.value]

    def qual_test_hist(self, rows):
        """Test hook (mcom_test_qual_hist): (alphabet map as 32 bytes, A, counts int64 [A, min(A, 8), 8, A] on the device) of the uint8
        device matrix `rows` (at least one row), through the launches of mcom_qual_encode."""
        torch = _torch()
        self.lib.mcom_test_qual_hist.restype = C.c_int
        self.lib.mcom_test_qual_hist.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]
        n, L = int(rows.shape[0]), int(rows.shape[1])
        pitch = int(rows.stride(0)) if n > 1 else L
        hmap = C.create_string_buffer(32); A = C.c_uint32()
        self._check(self.lib.mcom_test_qual_hist(self._h, rows.data_ptr(), n, L, pitch, hmap, C.byref(A), None))
        a = int(A.value); q = min(a, 8)
        counts = torch.empty(a * q * 8 * a, dtype=torch.int64, device=self.device)
        self._check(self.lib.mcom_test_qual_hist(self._h, rows.data_ptr(), n, L, pitch, hmap, C.byref(A), self._p(counts)))
        return hmap.raw, a, counts.view(a, q, 8, a)

    # ---- read names and '+' lines (csrc/names.hip) ----
    def name_encode(self, text, n_records: int, out=None):
        """mcom_name_encode.  text: uint8 device tensor holding the name text of n_records records (two lines each, any address).
        Returns the `.mcn` member as a uint8 device tensor; McomError names the first record with a line above
        255 bytes.  out: a uint8 device tensor to write the member into."""
        torch = _torch()
        n = int(text.shape[0])
        cap = int(out.shape[0]) if out is not None else int(self.lib.mcom_name_bound(n))
        if out is None:
            out = torch.empty(cap, dtype=torch.uint8, device=self.device)
        got, bad = C.c_uint64(), C.c_uint64()
        self._check(self.lib.mcom_name_encode(self._h, self._p(text, torch.uint8) if n else None, n, int(n_records), self._p(out), cap, C.byref(got), C.byref(bad)))
        return out[:got.value]

    def name_decode(self, member, out=None):
        """mcom_name_decode.  member: uint8 device tensor.  Returns (the name text as a uint8 device tensor, the offset of every record
        in it as an int64 device tensor of n_records + 1 entries); McomError for every member section 3.10 refuses.  out: a uint8
        device tensor to decode into (its length is the room offered)."""
        torch = _torch()
        n_in = int(member.shape[0])
        head = bytes(member[:96].cpu().numpy())
        n, t = C.c_uint64(), C.c_uint64()
        if self.lib.mcom_name_info(head if head else None, n_in, C.byref(n), C.byref(t)):
            raise McomError("name_decode: not a .mcn member")
        n, t = int(n.value), int(t.value)
        if out is None:
            out = torch.empty(max(t, 1), dtype=torch.uint8, device=self.device)
        off = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        gt, gn = C.c_uint64(), C.c_uint64()
        self._check(self.lib.mcom_name_decode(self._h, self._p(member, torch.uint8), n_in, self._p(out, torch.uint8), int(out.shape[0]), C.byref(gt), C.byref(gn), self._p(off)))
        return out[:t], off

    def name_encode_mate(self, text, n_records: int, mate, out=None):
        """mcom_name_encode_mate.  text, mate: uint8 device tensors, the name texts of the second and the first
        file of a pair (n_records records each; both are read up to their last byte and no further).  Returns the `.mcn` member: kind 2,
        coded against the mate, where that is strictly smaller than name_encode's member, and that member otherwise."""
        torch = _torch()
        n, nm = int(text.shape[0]), int(mate.shape[0])
        cap = int(out.shape[0]) if out is not None else int(self.lib.mcom_name_bound(n))
        if out is None:
            out = torch.empty(cap, dtype=torch.uint8, device=self.device)
        got, bad = C.c_uint64(), C.c_uint64()
        self._check(self.lib.mcom_name_encode_mate(self._h, self._p(text, torch.uint8) if n else None, n, int(n_records), self._p(mate, torch.uint8) if nm else None, nm,
                                                   self._p(out), cap, C.byref(got), C.byref(bad)))
        return out[:got.value]

    def name_decode_mate(self, member, mate, out=None):
        """mcom_name_decode_mate.  member, mate: uint8 device tensors.  Returns the name text as a uint8 device tensor; a kind-2 member is
        decoded against the mate and refused (McomError) when the mate is not the text it was coded against; kinds 0 and 1 as name_decode.
        out: a uint8 device tensor to decode into (its length is the room offered)."""
        torch = _torch()
        n_in, nm = int(member.shape[0]), int(mate.shape[0])
        head = bytes(member[:96].cpu().numpy())
        n, t = C.c_uint64(), C.c_uint64()
        if self.lib.mcom_name_info_mate(head if head else None, n_in, C.byref(n), C.byref(t)):
            raise McomError("name_decode_mate: not a .mcn member")
        t = int(t.value)
        if out is None:
            out = torch.empty(max(t, 1), dtype=torch.uint8, device=self.device)
        gt, gn = C.c_uint64(), C.c_uint64()
        self._check(self.lib.mcom_name_decode_mate(self._h, self._p(member, torch.uint8), n_in, self._p(mate, torch.uint8) if nm else None, nm, self._p(out, torch.uint8),
                                                   int(out.shape[0]), C.byref(gt), C.byref(gn)))
        return out[:t]

    def name_compare(self, text_a, off_a, text_b, off_b):
        """mcom_name_compare.  Two name texts (uint8 device tensors) with their record offsets (int64 device tensors of n + 1 entries).
        Returns (the number of records that differ, the lowest of them or None)."""
        torch = _torch()
        n = int(off_a.shape[0]) - 1
        if int(off_b.shape[0]) - 1 != n or off_a.dtype != torch.int64 or off_b.dtype != torch.int64:
            raise McomError("name_compare: two int64 offset arrays of one length")
        d, f = C.c_uint64(), C.c_uint64()
        self._check(self.lib.mcom_name_compare(self._h, self._p(text_a, torch.uint8), self._p(off_a), int(text_a.shape[0]), self._p(text_b, torch.uint8), self._p(off_b),
                                               int(text_b.shape[0]), n, C.byref(d), C.byref(f)))
        return int(d.value), (None if f.value == 0xFFFFFFFFFFFFFFFF else int(f.value))

    def fastq_names(self, text, first_record: int = 0):
        """mcom_decode_line_index + mcom_fastq_name_text.  text: uint8 device tensor holding whole four-line records (every line ends
        with a newline).  Returns (the name text uint8, record offsets int64 [n_records + 1], flag bits of MCOM_FASTQ_F_*, the first
        flagged record or None); a flagged record takes no room in the name text."""
        torch = _torch()
        start, _ = self.decode_line_index(text)
        n_rec = (int(start.shape[0]) - 1) // 4
        off = torch.zeros(n_rec + 1, dtype=torch.int64, device=self.device)
        flag = torch.tensor([0, -1], dtype=torch.int32, device=self.device)
        nb = C.c_uint64()
        self._check(self.lib.mcom_fastq_name_text(self._h, self._p(text, torch.uint8) if n_rec else None, int(text.shape[0]), self._p(start), first_record, n_rec, None, 0,
                                                  C.byref(nb), self._p(off), self._p(flag)))
        out = torch.empty(max(int(nb.value), 1), dtype=torch.uint8, device=self.device)
        flag = torch.tensor([0, -1], dtype=torch.int32, device=self.device)
        self._check(self.lib.mcom_fastq_name_text(self._h, self._p(text, torch.uint8) if n_rec else None, int(text.shape[0]), self._p(start), first_record, n_rec, self._p(out),
                                                  int(out.shape[0]), C.byref(nb), self._p(off), self._p(flag)))
        f = flag.cpu().numpy().view(np.uint32)
        return out[:nb.value], off, int(f[0]), (None if f[1] == 0xFFFFFFFF else int(f[1]))

    def fastq_emit_named(self, reads, quals, names, rec_off, first: int = 0):
        """mcom_fastq_emit_named.  reads, quals: uint8 device matrices [count, >= L] with contiguous rows: the rows of records first ..
        first + count - 1.  names, rec_off: a name text and the offsets of ALL its records (what name_decode returns).  Returns the
        records `@<name>`, read, `+<text>`, qualities as one uint8 device tensor."""
        torch = _torch()
        count, L = int(quals.shape[0]), int(quals.shape[1])
        if int(reads.shape[0]) != count or int(reads.shape[1]) != L or (count and (reads.stride(1) != 1 or quals.stride(1) != 1)):
            raise McomError("fastq_emit_named: reads and qualities of one shape, rows contiguous")
        if rec_off.dtype != torch.int64 or first < 0 or first + count + 1 > int(rec_off.shape[0]):
            raise McomError("fastq_emit_named: %d records from %d need %d int64 offsets" % (count, first, first + count + 1))
        rp = int(reads.stride(0)) if count > 1 else L
        qp = int(quals.stride(0)) if count > 1 else L
        off = rec_off[first:]
        nb = C.c_uint64()
        self._check(self.lib.mcom_fastq_emit_named(self._h, None, rp, None, qp, None, int(names.shape[0]), self._p(off), count, L, None, C.byref(nb)))
        out = torch.empty(max(int(nb.value), 1), dtype=torch.uint8, device=self.device)
        self._check(self.lib.mcom_fastq_emit_named(self._h, reads.data_ptr() if count else None, rp, quals.data_ptr() if count else None, qp, self._p(names, torch.uint8),
                                                   int(names.shape[0]), self._p(off), count, L, self._p(out), C.byref(nb)))
        return out[:nb.value]

    # ---- the digest of a FASTQ file (csrc/digest.hip) ----
    def fastq_record_hashes(self, text, lines_per_record: int = 4, first_record: int = 0, hS=None, hQ=None, hN=None, with_qual: bool = True, with_names: bool = True):
        """mcom_decode_line_index + mcom_fastq_record_hashes.  text: uint8 device tensor holding whole records of lines_per_record (4 or 1)
        lines.  hS, hQ, hN: int64 device tensors [n_total, 2] that cover all records of the file and are written at first_record .. (fresh
        ones of first_record + n_records rows otherwise; hQ / hN are left out with with_qual / with_names False and with lines_per_record
        1).  Returns (hS, hQ, hN, flag bits of MCOM_FASTQ_F_*, the first flagged record or None); a flagged record's rows are not written."""
        torch = _torch()
        start, _ = self.decode_line_index(text)
        n_rec = (int(start.shape[0]) - 1) // int(lines_per_record)
        four = int(lines_per_record) == 4
        fresh = lambda: torch.zeros((max(first_record + n_rec, 1), 2), dtype=torch.int64, device=self.device)  # noqa: E731
        if hS is None:
            hS = fresh()
        if hQ is None and four and with_qual:
            hQ = fresh()
        if hN is None and four and with_names:
            hN = fresh()
        n_total = int(hS.shape[0])
        for t in (hS, hQ, hN):
            if t is not None and (t.dtype != torch.int64 or t.dim() != 2 or int(t.shape[1]) != 2 or int(t.shape[0]) != n_total or not t.is_contiguous()):
                raise McomError("fastq_record_hashes: the hash arrays are contiguous int64 [n_total, 2] of one length")
        if first_record + n_rec > n_total:
            raise McomError("fastq_record_hashes: %d records from %d do not fit %d rows" % (n_rec, first_record, n_total))
        flag = torch.tensor([0, -1], dtype=torch.int32, device=self.device)
        self._check(self.lib.mcom_fastq_record_hashes(self._h, self._p(text, torch.uint8) if n_rec else None, int(text.shape[0]), self._p(start), int(first_record), n_rec,
                                                      int(lines_per_record), n_total, self._p(hS), self._p(hQ), self._p(hN), self._p(flag)))
        f = flag.cpu().numpy().view(np.uint32)
        return hS, hQ, hN, int(f[0]), (None if f[1] == 0xFFFFFFFF else int(f[1]))

    def digest_reduce(self, hS1, hQ1=None, hN1=None, hS2=None, hQ2=None, hN2=None, n=None):
        """mcom_digest_reduce over int64 device tensors [>= n, 2] (n: all rows of hS1 by default).  Returns the sixteen sums as Python
        integers: word 2 * key + seed, keys in the order seq.ordered.1, qual.ordered.1, name.ordered.1, the three of file 2, seq.multiset,
        rec.multiset; the sums of arrays not given are 0."""
        torch = _torch()
        n = int(hS1.shape[0]) if n is None else int(n)
        for t in (hS1, hQ1, hN1, hS2, hQ2, hN2):
            if t is not None and (t.dtype != torch.int64 or t.dim() != 2 or int(t.shape[1]) != 2 or int(t.shape[0]) < n or not t.is_contiguous()):
                raise McomError("digest_reduce: the hash arrays are contiguous int64 [>= n, 2]")
        sums = (C.c_uint64 * 16)()
        self._check(self.lib.mcom_digest_reduce(self._h, self._p(hS1) if n else None, self._p(hQ1), self._p(hN1), self._p(hS2), self._p(hQ2), self._p(hN2), n, sums))
        return [int(v) for v in sums]

    # ---- the odd reads of a -V archive against the contigs (csrc/odd_align.hip) ----
    _ODD_GUARD = 0xA5A5A5A5A5A5A5A5 - (1 << 64)                # 0xA5 in every byte of an int64 word

    def _odd_guarded(self, words: int, canary: int, cols: int = 0):
        """an int64 device buffer of `words` zeroed words (rows of `cols` when given) with canary // 8 words of 0xA5 bytes on either side:
        (the whole buffer, the zeroed view inside it)"""
        torch = _torch()
        if canary % 8:
            raise McomError("a canary around 64-bit words is a multiple of 8 bytes")
        cw, n = canary // 8, words * max(cols, 1)
        buf = torch.full((n + 2 * cw,), self._ODD_GUARD, dtype=torch.int64, device=self.device)
        buf[cw:cw + n] = 0
        return buf, buf[cw:cw + n]

    def _odd_guard_check(self, buf, inner_words: int, canary: int, what: str):
        cw = canary // 8
        if cw and not (bool((buf[:cw] == self._ODD_GUARD).all()) and bool((buf[cw + inner_words:] == self._ODD_GUARD).all())):
            raise McomError(what + " wrote outside its output")

    def odd_text(self, refs, canary: int = 0):
        """mcom_odd_text_append over refs, a list of (ref.bin image: uint8 device vector, bases taken from it): T as an int64 device vector of
        (|T| + 31) // 32 + 1 words (2 bits per base, the last word zero), and |T|.  canary: that many bytes of 0xA5 (a multiple of 8) are
        placed around T and checked after the calls."""
        total = sum(int(b) for _, b in refs)
        words = (total + 31) // 32 + 1
        buf, t = self._odd_guarded(words, canary)
        at = 0
        for img, bases in refs:
            self._check(self.lib.mcom_odd_text_append(self._h, self._p(t), words, at, self._p(img, _torch().uint8) if int(img.shape[0]) else None, int(img.shape[0]), int(bases)))
            at += int(bases)
        self.sync()
        self._odd_guard_check(buf, words, canary, "odd_text_append")
        return t.clone(), total

    def _odd_args(self, t, t_bases, odd, off):
        torch = _torch()
        n_odd = int(off.shape[0]) - 1
        if t.dtype != torch.int64 or int(t.shape[0]) < (int(t_bases) + 31) // 32 + 1 or off.dtype != torch.int64 or n_odd < 0 or odd.dtype != torch.uint8:
            raise McomError("odd_align: t int64 of (|T| + 31) // 32 + 1 words, odd uint8, off int64 [n_odd + 1]")
        return n_odd

    def odd_index_build(self, t, t_bases: int):
        """mcom_odd_index_build: the handle of the sorted seed grid of T (release it with odd_index_free)."""
        torch = _torch()
        if t.dtype != torch.int64 or int(t.shape[0]) < (int(t_bases) + 31) // 32 + 1:
            raise McomError("odd_index_build: t int64 of (|T| + 31) // 32 + 1 words")
        h = C.c_void_p()
        self._check(self.lib.mcom_odd_index_build(self._h, self._p(t), int(t_bases), C.byref(h)))
        return h

    def odd_index_free(self, idx):
        self.lib.mcom_odd_index_free(self._h, idx)

    def odd_index_entries(self, idx, canary: int = 0):
        """the sorted grid as an int64 tensor [n, 2] (key, position): a copy, made between canaries when asked for"""
        n = int(self.lib.mcom_odd_index_size(idx))
        buf, out = self._odd_guarded(n, canary, cols=2)
        if n:
            self._check(self.lib.mcom_odd_index_copy(self._h, idx, self._p(out)))
        self._odd_guard_check(buf, 2 * n, canary, "odd_index_copy")
        return out.clone().reshape(n, 2)

    def odd_align(self, idx, t, t_bases: int, odd, off, canary: int = 0):
        """mcom_odd_align.  odd: the full odd text (uint8 device vector), off: int64 [n_odd + 1].  Returns the hit words, int64 [n_odd]
        (-1: not aligned; else d << 48 | strand << 40 | p).  canary: that many bytes of 0xA5 (a multiple of 8) are placed around the hit
        words -- exactly n_odd of them, none for no record -- and checked after the call."""
        n_odd = self._odd_args(t, t_bases, odd, off)
        buf, hits = self._odd_guarded(n_odd, canary)
        self._check(self.lib.mcom_odd_align(self._h, idx, self._p(t), int(t_bases), self._p(odd), self._p(off), n_odd, self._p(hits) if n_odd else None))
        self._odd_guard_check(buf, n_odd, canary, "odd_align")
        return hits.clone()

    def odd_align_encode(self, hits, t, t_bases: int, odd, off, canary: int = 0):
        """mcom_odd_align_encode: (member, residual) as uint8 device vectors; member is empty when no record is aligned.  canary: that many
        bytes of 0xA5 are placed around both outputs and checked after the call."""
        torch = _torch()
        n_odd = self._odd_args(t, t_bases, odd, off)
        ml, rl = C.c_uint64(), C.c_uint64()
        args = (self._p(hits, torch.int64) if n_odd else None, self._p(odd), self._p(off), n_odd, self._p(t), int(t_bases))
        self._check(self.lib.mcom_odd_align_encode(self._h, *args, None, 0, C.byref(ml), None, 0, C.byref(rl)))
        m, r = int(ml.value), int(rl.value)
        mem = torch.full((m + 2 * canary + 1,), 0xA5, dtype=torch.uint8, device=self.device)
        res = torch.full((r + 2 * canary + 1,), 0xA5, dtype=torch.uint8, device=self.device)
        self._check(self.lib.mcom_odd_align_encode(self._h, *args, C.c_void_p(mem.data_ptr() + canary), m, C.byref(ml), C.c_void_p(res.data_ptr() + canary), r, C.byref(rl)))
        for buf, n in ((mem, m), (res, r)):
            if canary and not (bool((buf[:canary] == 0xA5).all()) and bool((buf[canary + n:] == 0xA5).all())):
                raise McomError("odd_align_encode wrote outside its output")
        return mem[canary:canary + m].clone(), res[canary:canary + r].clone()

    def odd_align_decode(self, member, t, t_bases: int, residual, off, canary: int = 0):
        """mcom_odd_align_decode of an untrusted member.  Returns (the full odd text or None, flags, the refusal's words or None)."""
        torch = _torch()
        n_odd = int(off.shape[0]) - 1
        if t.dtype != torch.int64 or int(t.shape[0]) < (int(t_bases) + 31) // 32 + 1 or off.dtype != torch.int64 or n_odd < 0:
            raise McomError("odd_align_decode: t int64 of (|T| + 31) // 32 + 1 words, off int64 [n_odd + 1]")
        odd_bytes = int(off[-1].item())
        out = torch.full((odd_bytes + 2 * canary + 1,), 0xA5, dtype=torch.uint8, device=self.device)
        flags = C.c_uint32()
        rc = self.lib.mcom_odd_align_decode(self._h, self._p(member, torch.uint8), int(member.shape[0]), self._p(t), int(t_bases),
                                            self._p(residual, torch.uint8) if int(residual.shape[0]) else None, int(residual.shape[0]), self._p(off), n_odd, odd_bytes,
                                            C.c_void_p(out.data_ptr() + canary), C.byref(flags))
        if canary and not (bool((out[:canary] == 0xA5).all()) and bool((out[canary + odd_bytes:] == 0xA5).all())):
            raise McomError("odd_align_decode wrote outside its output")
        if rc:
            if not flags.value:
                self._check(rc)
            return None, int(flags.value), self.lib.mcom_last_error(self._h).decode()
        return out[canary:canary + odd_bytes].clone(), 0, None

    # ---- reads of differing lengths (csrc/ragged.hip) ----
    def fastq_lengths(self, text, first_record: int = 0, lens=None, hist=None):
        """mcom_decode_line_index + mcom_fastq_lengths.  text: uint8 device tensor holding whole four-line records.  lens: a uint8 device
        vector of at least first_record + n_records entries to write into (a fresh one otherwise); hist: the int64 device vector of 256
        counters that runs across the pieces of a file (a cleared one otherwise).  Returns (lens, hist, flag bits of MCOM_FASTQ_F_*, the
        first flagged record or None); the entry of a flagged record holds nothing valid."""
        torch = _torch()
        start, _ = self.decode_line_index(text)
        n_rec = (int(start.shape[0]) - 1) // 4
        if lens is None:
            lens = torch.zeros(max(first_record + n_rec, 1), dtype=torch.uint8, device=self.device)
        if hist is None:
            hist = torch.zeros(256, dtype=torch.int64, device=self.device)
        if lens.dtype != torch.uint8 or int(lens.shape[0]) < first_record + n_rec or hist.dtype != torch.int64 or int(hist.shape[0]) != 256:
            raise McomError("fastq_lengths: lens must hold %d bytes, hist 256 int64 counters" % (first_record + n_rec))
        flag = torch.tensor([0, -1], dtype=torch.int32, device=self.device)
        self._check(self.lib.mcom_fastq_lengths(self._h, self._p(text, torch.uint8) if n_rec else None, int(text.shape[0]), self._p(start), first_record, n_rec,
                                                self._p(lens), self._p(hist), self._p(flag)))
        f = flag.cpu().numpy().view(np.uint32)
        return lens, hist, int(f[0]), (None if f[1] == 0xFFFFFFFF else int(f[1]))

    def ragged_index(self, lens, L: int):
        """mcom_ragged_index.  lens: uint8 device vector, byte r = length of record r - 1.  Returns (slots int64 [n]: the rank among the
        even records, or bit 63 | the offset into the odd text -- negative as int64 --, n_even, n_odd, odd_bytes)."""
        torch = _torch()
        n = int(lens.shape[0])
        slot = torch.zeros(max(n, 1), dtype=torch.int64, device=self.device)
        ne, no, ob = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.mcom_ragged_index(self._h, self._p(lens, torch.uint8) if n else None, n, int(L), self._p(slot), C.byref(ne), C.byref(no), C.byref(ob)))
        return slot[:n], int(ne.value), int(no.value), int(ob.value)

    def fastq_ragged_rows(self, text, which: int, L: int, lens, slot, rows, odd, first_record: int = 0):
        """mcom_decode_line_index + mcom_fastq_ragged_rows.  text: uint8 device tensor holding whole four-line records, records
        first_record .. of the file; which: 1 the sequence lines, 3 the quality lines; lens, slot: the tables of ALL records (fastq_lengths,
        ragged_index); rows: uint8 device matrix [n_even, >= L] with contiguous rows, odd: uint8 device vector of odd_bytes -- both are
        written into.  Returns (flag bits of MCOM_FASTQ_F_*, the first flagged record or None)."""
        torch = _torch()
        start, _ = self.decode_line_index(text)
        n_rec = (int(start.shape[0]) - 1) // 4
        n_total = int(lens.shape[0])
        if lens.dtype != torch.uint8 or slot.dtype != torch.int64 or int(slot.shape[0]) != n_total or rows.dtype != torch.uint8 or odd.dtype != torch.uint8 or rows.dim() != 2 or \
                (int(rows.shape[0]) and (rows.stride(1) != 1 or int(rows.shape[1]) < L)):
            raise McomError("fastq_ragged_rows: lens uint8 and slot int64 of one length, rows a uint8 matrix of at least L columns, odd uint8")
        cap_rows, odd_cap = int(rows.shape[0]), int(odd.shape[0])
        pitch = int(rows.stride(0)) if cap_rows > 1 else max(L, int(rows.shape[1]) if cap_rows else L)
        flag = torch.tensor([0, -1], dtype=torch.int32, device=self.device)
        self._check(self.lib.mcom_fastq_ragged_rows(self._h, self._p(text, torch.uint8) if n_rec else None, int(text.shape[0]), self._p(start), first_record, n_rec, int(which), int(L),
                                                    self._p(lens) if n_total else None, self._p(slot) if n_total else None, n_total, rows.data_ptr() if cap_rows else None, pitch, cap_rows,
                                                    odd.data_ptr() if odd_cap else None, odd_cap, self._p(flag)))
        f = flag.cpu().numpy().view(np.uint32)
        return int(f[0]), (None if f[1] == 0xFFFFFFFF else int(f[1]))

    def fastq_emit_ragged(self, L: int, lens, slot, reads, odd_seq, quals=None, odd_qual=None, names=None, rec_off=None, first: int = 0, count=None):
        """mcom_fastq_emit_ragged.  lens, slot: the tables of all n records; reads (and quals): uint8 device matrices [n_even, >= L] with
        contiguous rows; odd_seq (and odd_qual): the odd texts; names, rec_off: a name text and the int64 offsets of all its records (what
        name_decode returns).  Returns records first .. first + count - 1 (to the last one by default) as one uint8 device tensor: four
        lines each with quals, else the read and a newline."""
        torch = _torch()
        n = int(lens.shape[0])
        count = n - first if count is None else int(count)
        S = RaggedSrc()
        n_even = int(reads.shape[0])
        for t in (reads, quals):
            if t is not None and (t.dtype != torch.uint8 or t.dim() != 2 or int(t.shape[0]) != n_even or (n_even and (t.stride(1) != 1 or int(t.shape[1]) < L))):
                raise McomError("fastq_emit_ragged: reads and qualities uint8 matrices of one row count and at least L columns, rows contiguous")
        if (quals is None) != (odd_qual is None) or (odd_qual is not None and int(odd_qual.shape[0]) != int(odd_seq.shape[0])) or (names is None) != (rec_off is None):
            raise McomError("fastq_emit_ragged: quality rows and odd quality text come together and match the reads', names and offsets come together")
        if lens.dtype != torch.uint8 or slot.dtype != torch.int64 or int(slot.shape[0]) != n or (rec_off is not None and (rec_off.dtype != torch.int64 or int(rec_off.shape[0]) != n + 1)):
            raise McomError("fastq_emit_ragged: lens uint8 [n], slot int64 [n], rec_off int64 [n + 1]")
        keep = [t.contiguous() if t is not None else None for t in (odd_seq, odd_qual, names, rec_off, lens, slot)]
        S.d_reads = reads.data_ptr() if n_even else None
        S.read_pitch = int(reads.stride(0)) if n_even > 1 else max(L, int(reads.shape[1]))
        nothing = torch.zeros(16, dtype=torch.uint8, device=self.device)      # an empty table still says "with qualities" / "with names"
        S.d_quals = (quals.data_ptr() if n_even else nothing.data_ptr()) if quals is not None else None
        S.qual_pitch = (int(quals.stride(0)) if n_even > 1 else max(L, int(quals.shape[1]))) if quals is not None else 0
        S.n_even = n_even
        S.odd_bytes = int(keep[0].shape[0])
        S.d_odd_seq = keep[0].data_ptr() if S.odd_bytes else None
        S.d_odd_qual = keep[1].data_ptr() if (quals is not None and S.odd_bytes) else None
        S.d_slot = keep[5].data_ptr() if n else None
        S.d_len = keep[4].data_ptr() if n else None
        S.n = n
        S.d_names = (keep[2].data_ptr() if int(keep[2].shape[0]) else nothing.data_ptr()) if names is not None else None
        S.names_bytes = int(keep[2].shape[0]) if names is not None else 0
        S.d_rec_off = keep[3].data_ptr() if rec_off is not None else None
        S.L = int(L)
        nb = C.c_uint64()
        self._check(self.lib.mcom_fastq_emit_ragged(self._h, C.byref(S), int(first), count, None, 0, C.byref(nb)))
        out = torch.empty(max(int(nb.value), 1), dtype=torch.uint8, device=self.device)
        self._check(self.lib.mcom_fastq_emit_ragged(self._h, C.byref(S), int(first), count, self._p(out), int(out.shape[0]), C.byref(nb)))
        return out[:nb.value]

    # ---- the block-sorting coder (csrc/bwt.hip) ----
    def bwt_encode(self, raw, out=None):
        """mcom_bwt_encode.  raw: uint8 device tensor.  Returns the `.bwt` member as a uint8 device tensor.
        out: a uint8 device tensor to write the member into (its length is the room offered) instead of a fresh one."""
        torch = _torch()
        n = int(raw.shape[0])
        cap = int(out.shape[0]) if out is not None else int(self.lib.mcom_bwt_bound(n))
        if out is None:
            out = torch.empty(cap, dtype=torch.uint8, device=self.device)
        got = C.c_uint64()
        self._check(self.lib.mcom_bwt_encode(self._h, self._p(raw, torch.uint8) if n else None, n, self._p(out), cap, C.byref(got)))
        return out[:got.value]

    def bwt_decode(self, member, out=None):
        """mcom_bwt_decode.  member: uint8 device tensor.  Returns the raw bytes as a uint8 device tensor; McomError for every member
        section 3.8 refuses.  out: a uint8 device tensor to decode into (its length is the room offered) instead of a fresh one of
        the length the header states (below 4 GiB)."""
        torch = _torch()
        n = int(member.shape[0])
        if out is not None:
            cap = int(out.shape[0])
        else:
            # the room comes from the header only once the header describes this member to the byte (the host twin's own check)
            from .pipeline import load_host_library
            head = bytes(member[:40].cpu().numpy()) if n >= 40 else b""
            raw_len = C.c_uint64()
            if len(head) != 40 or load_host_library().mcomh_bwt_raw_len(head, n, C.byref(raw_len)):
                raise McomError("bwt_decode: the header does not describe this member")
            cap = int(raw_len.value)
            out = torch.empty(max(cap, 1), dtype=torch.uint8, device=self.device)
        got = C.c_uint64()
        self._check(self.lib.mcom_bwt_decode(self._h, self._p(member, torch.uint8) if n else None, n, self._p(out), cap, C.byref(got)))
        return out[:got.value]

    def bwt_test_forward(self, raw):
        """Test hook (mcom_test_bwt_forward): (transformed bytes uint8 [n], index rows int64 [anchors], rounds of prefix doubling) for
        the uint8 device tensor `raw` (at least one byte), through the launches of mcom_bwt_encode."""
        torch = _torch()
        self.lib.mcom_test_bwt_forward.restype = C.c_int
        self.lib.mcom_test_bwt_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        n = int(raw.shape[0])
        n_anc = sum(-(-min(1 << 20, n - a) // 4096) for a in range(0, n, 1 << 20))
        tr = torch.empty(n, dtype=torch.uint8, device=self.device)
        idx = torch.zeros(max(n_anc, 1), dtype=torch.int32, device=self.device)
        rounds = C.c_int()
        self._check(self.lib.mcom_test_bwt_forward(self._h, self._p(raw, torch.uint8), n, self._p(tr), self._p(idx), C.byref(rounds)))
        return tr, idx[:n_anc].to(torch.int64) & 0xFFFFFFFF, int(rounds.value)

    def bwt_test_mtf(self, src, decode: bool = False):
        """Test hook (mcom_test_bwt_mtf): the move-to-front ranks of the uint8 device tensor `src` (decode: the bytes of ranks), the
        list starting as 0 .. 255 every 2^20 bytes, through the launches of the codec."""
        torch = _torch()
        self.lib.mcom_test_bwt_mtf.restype = C.c_int
        self.lib.mcom_test_bwt_mtf.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int]
        src = src.contiguous().clone()                      # (a fresh allocation: 4-byte aligned)
        dst = torch.empty_like(src)
        self._check(self.lib.mcom_test_bwt_mtf(self._h, self._p(src, torch.uint8), int(src.shape[0]), self._p(dst), 1 if decode else 0))
        return dst

    # -- verification (csrc/verify.hip)
    def _verify_table(self, t, L: int):
        """(rows, pitch, n) or (rows, pitch, n, mates): uint8 device tensors whose first byte is row 0 (a slice at any offset of a
        larger buffer will do), rows `pitch` bytes apart; a tensor may be None when n == 0."""
        torch = _torch()
        rows, pitch, n = t[0], int(t[1]), int(t[2])
        mates = t[3] if len(t) > 3 else None
        for x in (rows, mates):
            if x is not None and n and (x.dtype != torch.uint8 or x.numel() < (n - 1) * pitch + L):
                raise McomError("a table must be a uint8 tensor that holds (n - 1) * pitch + L bytes from row 0 on")
        return VerifyTable(self._p(rows).value if n else None, self._p(mates).value if (mates is not None and n) else None, pitch, n)

    @staticmethod
    def _verify_dict(r: VerifyReport) -> dict:
        return {"identical": bool(r.identical), "n_a": int(r.n_a), "n_b": int(r.n_b), "missing": int(r.missing), "extra": int(r.extra),
                "differing": int(r.differing), "first_diff": None if r.first_diff == 2 ** 64 - 1 else int(r.first_diff),
                "exact_runs": int(r.exact_runs), "missing_examples": [int(v) for v in r.missing_ex[: r.n_missing_ex]],
                "extra_examples": [int(v) for v in r.extra_ex[: r.n_extra_ex]]}

    def verify_multiset(self, a, b, L: int) -> dict:
        """mcom_verify_multiset: are the records of table a and table b the same multiset?  a, b: see _verify_table."""
        ta, tb, r = self._verify_table(a, L), self._verify_table(b, L), VerifyReport()
        self._check(self.lib.mcom_verify_multiset(self._h, C.byref(ta), C.byref(tb), L, C.byref(r)))
        return self._verify_dict(r)

    def verify_multiset_parts(self, a, b, L: int) -> dict:
        """mcom_verify_multiset_parts: a, b = (parts, pitch, n) with parts a list of 1 .. 4 uint8 device tensors whose first byte is row 0 of
        that part (rows `pitch` apart in all parts of a side); a record is row i of every part, one after the other."""
        torch = _torch()

        def side(t):
            parts, pitch, n = list(t[0]), int(t[1]), int(t[2])
            if not 1 <= len(parts) <= 4:
                raise McomError("verify_multiset_parts: 1 .. 4 parts")
            for x in parts:
                if n and (x is None or x.dtype != torch.uint8 or x.numel() < (n - 1) * pitch + L):
                    raise McomError("a part must be a uint8 tensor that holds (n - 1) * pitch + L bytes from row 0 on")
            v = VerifyParts()
            for q, x in enumerate(parts):
                v.d_part[q] = x.data_ptr() if n else None
            v.n_parts, v.pitch, v.n = len(parts), pitch, n
            return v
        ta, tb, r = side(a), side(b), VerifyReport()
        self._check(self.lib.mcom_verify_multiset_parts(self._h, C.byref(ta), C.byref(tb), L, C.byref(r)))
        return self._verify_dict(r)

    def verify_ordered(self, a, b, L: int) -> dict:
        """mcom_verify_ordered: record i of table a against record i of table b."""
        ta, tb, r = self._verify_table(a, L), self._verify_table(b, L), VerifyReport()
        self._check(self.lib.mcom_verify_ordered(self._h, C.byref(ta), C.byref(tb), L, C.byref(r)))
        return self._verify_dict(r)

    def set_verify_hash_bits(self, bits: int):
        """Test hook (mcom_set_verify_hash_bits): mcom_verify_multiset keeps the low `bits` bits of its hashes (64 or negative: all)."""
        self._check(self.lib.mcom_set_verify_hash_bits(self._h, int(bits)))

    def rans_test_hist(self, raw):
        """Test hook (mcom_test_rans_hist): the counts of k_rans_hist for the uint8 device tensor `raw` (at least one byte), launched as
        mcom_rans_encode launches it.  Returns (o0 int64 [4, 256], o1 int64 [7, 256, 256]) on the device."""
        torch = _torch()
        self.lib.mcom_test_rans_hist.restype = C.c_int; self.lib.mcom_test_rans_hist.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        counts = torch.empty(4 * 256 + 7 * 65536, dtype=torch.int64, device=self.device)
        self._check(self.lib.mcom_test_rans_hist(self._h, self._p(raw, torch.uint8), int(raw.shape[0]), self._p(counts)))
        return counts[:1024].view(4, 256), counts[1024:].view(7, 256, 256)

    def rans_test_seg_crc(self, raw, seg_log2: int = 11):
        """Test hook (mcom_test_rans_seg_crc): the CRC-32 of every segment of 2^seg_log2 bytes of `raw`, as k_rans_crc makes them for
        the codec calls.  Returns int64 [n_seg] on the device (values below 2^32)."""
        torch = _torch()
        self.lib.mcom_test_rans_seg_crc.restype = C.c_int
        self.lib.mcom_test_rans_seg_crc.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
        n = int(raw.shape[0])
        crc = torch.empty(max(1, -(-n // (1 << seg_log2))), dtype=torch.int32, device=self.device)
        self._check(self.lib.mcom_test_rans_seg_crc(self._h, self._p(raw, torch.uint8), n, seg_log2, self._p(crc)))
        return crc.to(torch.int64) & 0xFFFFFFFF


class Index:
    """Device-resident contig-minimizer index (mcom_idx)."""

    def __init__(self, ctx: Context, rec, k: int, b: int = 14):
        self.ctx = ctx
        self.n = int(rec.shape[0])
        h = C.c_void_p()
        ctx._check(ctx.lib.mcom_idx_build(ctx._h, ctx._p(rec), self.n, k, b, C.byref(h)))
        self._h = h

    def get(self, x):
        torch = _torch()
        n = int(x.shape[0])
        start = torch.empty(n, dtype=torch.int32, device=self.ctx.device)
        count = torch.empty(n, dtype=torch.int32, device=self.ctx.device)
        self.ctx._check(self.ctx.lib.mcom_idx_get(self.ctx._h, self._h, self.ctx._p(x, torch.int64), n, self.ctx._p(start), self.ctx._p(count)))
        return start, count

    def records(self):
        out = self.ctx.empty_records(max(self.n, 1))
        n = C.c_size_t()
        self.ctx._check(self.ctx.lib.mcom_idx_records(self.ctx._h, self._h, self.ctx._p(out), C.byref(n)))
        return out[: self.n]

    def close(self):
        if getattr(self, "_h", None):
            self.ctx.lib.mcom_idx_destroy(self.ctx._h, self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Dicts:
    """Device-resident Stage-2 dictionaries (mcom_dicts)."""

    def __init__(self, ctx: Context, sgbits, L: int, ininumdict: int = 0):
        torch = _torch()
        self.ctx = ctx
        self.n_sg = int(sgbits.shape[0])
        h = C.c_void_p()
        ctx._check(ctx.lib.mcom_dicts_build(ctx._h, ctx._p(sgbits, torch.int64), self.n_sg, L, ininumdict, C.byref(h)))
        self._h = h
        nd = C.c_int()
        nk = (C.c_uint32 * 16)(); mb = (C.c_uint32 * 16)()
        ctx._check(ctx.lib.mcom_dicts_info(self._h, C.byref(nd), nk, mb))
        self.nd = nd.value
        self.numkeys = [int(nk[i]) for i in range(self.nd)]
        self.maxbin = [int(mb[i]) for i in range(self.nd)]

    def lookup(self, dict_idx: int, keys):
        torch = _torch()
        n = int(keys.shape[0])
        start = torch.empty(n, dtype=torch.int32, device=self.ctx.device)
        count = torch.empty(n, dtype=torch.int32, device=self.ctx.device)
        self.ctx._check(self.ctx.lib.mcom_dicts_lookup(self.ctx._h, self._h, dict_idx, self.ctx._p(keys, torch.int64), n,
                                                       self.ctx._p(start), self.ctx._p(count)))
        return start, count

    def ids(self, dict_idx: int):
        torch = _torch()
        out = torch.empty(max(self.n_sg, 1), dtype=torch.int32, device=self.ctx.device)
        self.ctx._check(self.ctx.lib.mcom_dicts_ids(self.ctx._h, self._h, dict_idx, self.ctx._p(out)))
        return out[: self.n_sg]

    def close(self):
        if getattr(self, "_h", None):
            self.ctx.lib.mcom_dicts_free(self.ctx._h, self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dict_layout(L: int, ininumdict: int = 0):
    """mcom_dict_layout (host only): (start[], end[]) of the dictionary keys."""
    lib = load_library()
    st = (C.c_int * 16)(); en = (C.c_int * 16)()
    nd = lib.mcom_dict_layout(L, ininumdict, st, en)
    if nd < 0:
        raise McomError("mcom_dict_layout failed")
    return [st[i] for i in range(nd)], [en[i] for i in range(nd)]


def pack_nt4(reads: np.ndarray) -> np.ndarray:
    """Host statement of the packed-row format of include/mcom.h for ACGT-only rows (tests, host driver)."""
    n, L = reads.shape
    W = words_per_read(L)
    code = ((reads >> 1) ^ (reads >> 2)) & 3
    out = np.zeros((n, W), dtype=np.uint64)
    for i in range(L):
        out[:, i // 32] |= code[:, i].astype(np.uint64) << np.uint64(2 * (i % 32))
    return out


def pack_contigs(refs) -> tuple:
    """Packs contig strings (bytes, ACGT) as mcom_realign_pass wants them: returns (cbits u64, coff u64, clen u32)."""
    coff = np.zeros(len(refs), dtype=np.uint64)
    clen = np.array([len(r) for r in refs], dtype=np.uint32)
    words = [(2 * int(l) + 63) // 64 + 1 for l in clen]          # one padding word after every contig
    total = int(sum(words)) + 1
    cbits = np.zeros(total, dtype=np.uint64)
    o = 0
    for i, r in enumerate(refs):
        coff[i] = o
        a = np.frombuffer(r, dtype=np.uint8)
        code = (((a >> 1) ^ (a >> 2)) & 3).astype(np.uint64)
        sh = (2 * (np.arange(len(a)) % 32)).astype(np.uint64)
        np.bitwise_or.at(cbits, o + np.arange(len(a)) // 32, code << sh)
        o += words[i]
    return cbits, coff, clen


def records_to_numpy(rec) -> np.ndarray:
    """Device [n,2] int64 record tensor -> numpy structured (x, y) uint64."""
    a = rec.detach().cpu().numpy().view(np.uint64)
    out = np.empty(a.shape[0], dtype=MM_DTYPE)
    out["x"] = a[:, 0]; out["y"] = a[:, 1]
    return out
