"""ctypes binding of libmcom_host.so (include/mcom_host.h): the C++ host driver of the hot path."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .hip import McomError, QualAgreeReport, QualLossyReport, QualLossySpec, load_library

HERE = os.path.dirname(os.path.abspath(__file__))


class VerifyReport(C.Structure):
    """mcomh_verify_report of include/mcom_host.h"""
    _fields_ = [("identical", C.c_int), ("mode", C.c_int), ("n_input", C.c_uint64), ("n_archive", C.c_uint64), ("missing", C.c_uint64),
                ("extra", C.c_uint64), ("differing", C.c_uint64), ("first_diff", C.c_uint64), ("exact_runs", C.c_uint64),
                ("missing_ex", C.c_uint64 * 8), ("extra_ex", C.c_uint64 * 8), ("n_missing_ex", C.c_uint32), ("n_extra_ex", C.c_uint32),
                ("times_ms", C.c_double * 8)]


class Digest(C.Structure):
    """mcomh_digest of include/mcom_host.h"""
    _fields_ = [("files", C.c_uint32), ("present", C.c_uint32), ("n", C.c_uint64), ("sums", C.c_uint64 * 16)]


class DigestReport(C.Structure):
    """mcomh_digest_report of include/mcom_host.h"""
    _fields_ = [("identical", C.c_int32), ("first_diff", C.c_int32), ("compared", C.c_uint32), ("differing", C.c_uint32), ("files", C.c_uint32), ("reserved", C.c_uint32),
                ("n_stored", C.c_uint64), ("n_output", C.c_uint64), ("message", C.c_char * 256)]


DIGEST_KEYS = ("seq.ordered.1", "qual.ordered.1", "name.ordered.1", "seq.ordered.2", "qual.ordered.2", "name.ordered.2", "seq.multiset", "rec.multiset")


class Params(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("k", "e", "m", "w", "cbthr", "max_rounds", "step", "maxthr", "numdict", "host_threads", "maxsearch", "window_scan",
                                         "full_consensus", "full_sketch", "overlap_screen", "host_dump", "stream_sets", "stage2_join", "read_batches")]


def host_lib_path() -> str:
    return os.path.join(HERE, "lib", "libmcom_host.so")


_lib = None


def load_host_library():
    global _lib
    if _lib is not None:
        return _lib
    load_library()                      # libmcom_hip.so first: fails loudly when it has not been built
    p = host_lib_path()
    if not os.path.exists(p):
        raise McomError(f"{p} is missing: run __graft_entry__.build()")
    L = C.CDLL(p)
    vp, sz, i32, cp = C.c_void_p, C.c_size_t, C.c_int, C.c_char_p
    L.mcomh_create.restype = i32
    L.mcomh_create.argtypes = [C.POINTER(vp), i32, vp, vp, vp, sz, sz, i32, C.POINTER(Params)]
    L.mcomh_create_streamed.restype = i32
    L.mcomh_create_streamed.argtypes = [C.POINTER(vp), i32, vp, vp, sz, i32, C.POINTER(Params)]
    L.mcomh_set_records.restype = i32; L.mcomh_set_records.argtypes = [vp, vp, vp]
    L.mcomh_create_packed.restype = i32
    L.mcomh_create_packed.argtypes = [C.POINTER(vp), i32, vp, vp, sz, i32, C.POINTER(Params)]
    L.mcomh_destroy.restype = None; L.mcomh_destroy.argtypes = [vp]
    L.mcomh_last_error.restype = cp; L.mcomh_last_error.argtypes = [vp]
    for f in ("mcomh_kt_for_reads", "mcomh_kt_for_bucket", "mcomh_combine_cluster", "mcomh_update_single", "mcomh_pre_process"):
        getattr(L, f).restype = i32; getattr(L, f).argtypes = [vp]
    L.mcomh_realign_hash.restype = i32; L.mcomh_realign_hash.argtypes = [vp, i32, C.POINTER(C.c_long)]
    L.mcomh_dump_stages.restype = i32; L.mcomh_dump_stages.argtypes = [vp, cp]
    L.mcomh_cluster_dump.restype = i32; L.mcomh_cluster_dump.argtypes = [vp, cp]
    L.mcomh_decompress.restype = i32; L.mcomh_decompress.argtypes = [cp, cp, C.POINTER(C.c_uint64)]
    L.mcomh_cluster_dump_order.restype = i32; L.mcomh_cluster_dump_order.argtypes = [vp, cp]
    L.mcomh_decompress_order.restype = i32; L.mcomh_decompress_order.argtypes = [cp, cp, C.POINTER(C.c_uint64)]
    L.mcomh_cluster_dump_pe.restype = i32; L.mcomh_cluster_dump_pe.argtypes = [vp, cp]
    L.mcomh_decompress_pe.restype = i32; L.mcomh_decompress_pe.argtypes = [cp, cp, cp, C.POINTER(C.c_uint64)]
    L.mcomh_decompress_gpu.restype = i32; L.mcomh_decompress_gpu.argtypes = [cp, cp, C.POINTER(C.c_uint64), i32]
    L.mcomh_decompress_order_gpu.restype = i32; L.mcomh_decompress_order_gpu.argtypes = [cp, cp, C.POINTER(C.c_uint64), i32]
    L.mcomh_decompress_pe_gpu.restype = i32; L.mcomh_decompress_pe_gpu.argtypes = [cp, cp, cp, C.POINTER(C.c_uint64), i32]
    L.mcomh_decompress_gpu_times.restype = None; L.mcomh_decompress_gpu_times.argtypes = [C.POINTER(C.c_double)]
    L.mcomh_verify_gpu.restype = i32; L.mcomh_verify_gpu.argtypes = [cp, i32, cp, cp, i32, C.POINTER(VerifyReport)]
    L.mcomh_fastq_pair_to_device.restype = i32
    L.mcomh_fastq_pair_to_device.argtypes = [cp, cp, i32, C.POINTER(i32), sz, C.POINTER(vp), C.POINTER(sz), C.c_char_p, sz]
    L.mcomh_n_contigs.restype = sz; L.mcomh_n_contigs.argtypes = [vp]
    L.mcomh_contig_ref.restype = vp; L.mcomh_contig_ref.argtypes = [vp, sz, C.POINTER(sz)]
    L.mcomh_contig_n.restype = sz; L.mcomh_contig_n.argtypes = [vp, sz]
    L.mcomh_contig_members.restype = vp; L.mcomh_contig_members.argtypes = [vp, sz]
    L.mcomh_list.restype = vp; L.mcomh_list.argtypes = [vp, cp, C.POINTER(sz)]
    L.mcomh_contig_set.restype = i32
    L.mcomh_contig_set.argtypes = [vp, C.POINTER(sz), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.mcomh_result_digest.restype = i32; L.mcomh_result_digest.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.mcomh_stat.restype = C.c_double; L.mcomh_stat.argtypes = [vp, cp]
    L.mcomh_prof_enable.restype = i32; L.mcomh_prof_enable.argtypes = [vp, i32]
    L.mcomh_prof_read.restype = i32; L.mcomh_prof_read.argtypes = [vp, cp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.mcomh_prof_kernels.restype = i32; L.mcomh_prof_kernels.argtypes = [vp, cp, C.c_char_p, sz, C.POINTER(sz)]
    L.mcomh_create_from_fastq.restype = i32; L.mcomh_create_from_fastq.argtypes = [C.POINTER(vp), i32, vp, cp, cp, C.POINTER(Params), C.c_char_p, sz]
    L.mcomh_fastq_read.restype = i32; L.mcomh_fastq_read.argtypes = [cp, C.POINTER(i32), vp, sz, C.POINTER(sz)]
    L.mcomh_fastq_to_device.restype = i32
    L.mcomh_fastq_to_device.argtypes = [cp, i32, C.POINTER(i32), sz, C.POINTER(vp), C.POINTER(sz), C.c_char_p, sz]
    L.mcomh_device_free.restype = None; L.mcomh_device_free.argtypes = [vp]
    u64 = C.c_uint64
    L.mcomh_rans_bound.restype = u64; L.mcomh_rans_bound.argtypes = [u64]
    L.mcomh_rans_estimate.restype = i32; L.mcomh_rans_estimate.argtypes = [vp, u64, C.POINTER(u64)]
    L.mcomh_rans_encode.restype = i32; L.mcomh_rans_encode.argtypes = [vp, u64, vp, u64, C.POINTER(u64), i32]
    L.mcomh_rans_decode.restype = i32; L.mcomh_rans_decode.argtypes = [vp, u64, vp, u64, C.POINTER(u64)]
    L.mcomh_bgzf_bound.restype = u64; L.mcomh_bgzf_bound.argtypes = [u64]
    L.mcomh_bgzf_encode.restype = i32; L.mcomh_bgzf_encode.argtypes = [vp, u64, vp, u64, C.POINTER(u64), i32]
    L.mcomh_bgzf_file.restype = i32; L.mcomh_bgzf_file.argtypes = [cp, cp, i32]
    L.mcomh_gzip_inflate_members.restype = i32; L.mcomh_gzip_inflate_members.argtypes = [vp, u64, vp, u64, vp, u64, vp, C.POINTER(u64), C.POINTER(u64)]
    L.mcomh_gzip_inflate.restype = i32; L.mcomh_gzip_inflate.argtypes = [vp, u64, vp, u64, C.POINTER(u64)]
    L.mcomh_gunzip_file.restype = i32; L.mcomh_gunzip_file.argtypes = [cp, cp, i32]
    L.mcomh_entropy_pack_file.restype = i32; L.mcomh_entropy_pack_file.argtypes = [cp, cp, i32]
    L.mcomh_entropy_unpack_file.restype = i32; L.mcomh_entropy_unpack_file.argtypes = [cp, cp, i32]
    L.mcomh_entropy_times.restype = None; L.mcomh_entropy_times.argtypes = [C.POINTER(C.c_double)]
    L.mcomh_bwt_bound.restype = u64; L.mcomh_bwt_bound.argtypes = [u64]
    L.mcomh_bwt_encode.restype = i32; L.mcomh_bwt_encode.argtypes = [vp, u64, vp, u64, C.POINTER(u64)]
    L.mcomh_bwt_decode.restype = i32; L.mcomh_bwt_decode.argtypes = [vp, u64, vp, u64, C.POINTER(u64)]
    L.mcomh_bwt_raw_len.restype = i32; L.mcomh_bwt_raw_len.argtypes = [vp, u64, C.POINTER(u64)]
    L.mcomh_bwt_stages.restype = i32; L.mcomh_bwt_stages.argtypes = [vp, u64, vp, vp, vp]
    L.mcomh_bwt_pack_file.restype = i32; L.mcomh_bwt_pack_file.argtypes = [cp, cp, i32]
    L.mcomh_bwt_unpack_file.restype = i32; L.mcomh_bwt_unpack_file.argtypes = [cp, cp, i32]
    u32 = C.c_uint32
    L.mcomh_qual_bound.restype = u64; L.mcomh_qual_bound.argtypes = [u64, u32]
    L.mcomh_qual_info.restype = i32; L.mcomh_qual_info.argtypes = [vp, u64, C.POINTER(u64), C.POINTER(u32)]
    L.mcomh_qual_estimate.restype = i32; L.mcomh_qual_estimate.argtypes = [vp, u64, u32, u64, C.POINTER(u64)]
    L.mcomh_qual_encode.restype = i32; L.mcomh_qual_encode.argtypes = [vp, u64, u32, u64, vp, u64, C.POINTER(u64), i32]
    L.mcomh_qual_decode.restype = i32; L.mcomh_qual_decode.argtypes = [vp, u64, vp, u64, u64, C.POINTER(u64), C.POINTER(u32)]
    L.mcomh_fastq_qualities_to_device.restype = i32
    L.mcomh_fastq_qualities_to_device.argtypes = [cp, i32, i32, sz, C.POINTER(vp), C.POINTER(sz), C.c_char_p, sz]
    L.mcomh_fastq_quality_member.restype = i32; L.mcomh_fastq_quality_member.argtypes = [cp, i32, i32, cp, C.POINTER(u64), C.c_char_p, sz]
    L.mcomh_device_copy.restype = i32; L.mcomh_device_copy.argtypes = [vp, vp, sz]
    L.mcomh_decompress_fastq.restype = i32; L.mcomh_decompress_fastq.argtypes = [cp, cp, C.POINTER(u64)]
    L.mcomh_decompress_fastq_gpu.restype = i32; L.mcomh_decompress_fastq_gpu.argtypes = [cp, cp, C.POINTER(u64), i32]
    L.mcomh_verify_quality_gpu.restype = i32; L.mcomh_verify_quality_gpu.argtypes = [cp, cp, i32, C.POINTER(VerifyReport)]
    L.mcomh_keep_read_order.restype = i32; L.mcomh_keep_read_order.argtypes = [vp, i32]
    L.mcomh_qual_gather_rows.restype = i32; L.mcomh_qual_gather_rows.argtypes = [vp, u64, u32, u64, vp, u64, vp, u64, C.POINTER(u32)]
    L.mcomh_fastq_quality_member_ordered.restype = i32; L.mcomh_fastq_quality_member_ordered.argtypes = [cp, i32, i32, cp, cp, C.POINTER(u64), C.c_char_p, sz]
    L.mcomh_qual_lossy_parse.restype = i32; L.mcomh_qual_lossy_parse.argtypes = [cp, C.POINTER(QualLossySpec)]
    L.mcomh_qual_lossy_print.restype = i32; L.mcomh_qual_lossy_print.argtypes = [C.POINTER(QualLossySpec), C.c_char_p, sz]
    L.mcomh_qual_transform.restype = i32; L.mcomh_qual_transform.argtypes = [vp, u64, u32, u64, C.POINTER(QualLossySpec), C.POINTER(QualLossyReport)]
    L.mcomh_qual_pack_file_lossy.restype = i32; L.mcomh_qual_pack_file_lossy.argtypes = [cp, cp, i32, i32, C.POINTER(QualLossySpec), C.POINTER(QualLossyReport)]
    L.mcomh_fastq_quality_member_lossy.restype = i32
    L.mcomh_fastq_quality_member_lossy.argtypes = [cp, i32, i32, cp, C.POINTER(QualLossySpec), cp, C.POINTER(u64), C.POINTER(QualLossyReport), C.c_char_p, sz]
    L.mcomh_qual_lossy_marker.restype = i32; L.mcomh_qual_lossy_marker.argtypes = [cp, C.POINTER(QualLossySpec), C.c_char_p, sz]
    L.mcomh_agree_mask.restype = i32; L.mcomh_agree_mask.argtypes = [cp, i32, cp, i32, C.POINTER(u64), C.POINTER(i32), C.POINTER(u64)]
    L.mcomh_qual_agree.restype = i32; L.mcomh_qual_agree.argtypes = [vp, u64, u32, u64, vp, u64, u64, u32, C.POINTER(QualAgreeReport)]
    L.mcomh_fastq_quality_member_agree.restype = i32
    L.mcomh_fastq_quality_member_agree.argtypes = [cp, i32, i32, cp, cp, u64, u32, C.POINTER(QualLossySpec), cp, C.POINTER(u64), C.POINTER(QualAgreeReport), C.POINTER(QualLossyReport), C.c_char_p, sz]
    L.mcomh_qual_agree_marker.restype = i32; L.mcomh_qual_agree_marker.argtypes = [cp, C.POINTER(u32), C.POINTER(u32)]
    L.mcomh_decompress_fastq_reordered.restype = i32; L.mcomh_decompress_fastq_reordered.argtypes = [cp, cp, C.POINTER(u64)]
    L.mcomh_decompress_fastq_reordered_gpu.restype = i32; L.mcomh_decompress_fastq_reordered_gpu.argtypes = [cp, cp, C.POINTER(u64), i32]
    L.mcomh_decompress_fastq_pe.restype = i32; L.mcomh_decompress_fastq_pe.argtypes = [cp, cp, cp, C.POINTER(u64)]
    L.mcomh_decompress_fastq_pe_gpu.restype = i32; L.mcomh_decompress_fastq_pe_gpu.argtypes = [cp, cp, cp, C.POINTER(u64), i32]
    L.mcomh_verify_records_gpu.restype = i32; L.mcomh_verify_records_gpu.argtypes = [cp, i32, cp, cp, i32, C.POINTER(VerifyReport)]
    L.mcomh_name_bound.restype = u64; L.mcomh_name_bound.argtypes = [u64]
    L.mcomh_name_info.restype = i32; L.mcomh_name_info.argtypes = [vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.mcomh_name_encode.restype = i32; L.mcomh_name_encode.argtypes = [vp, u64, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.mcomh_name_decode.restype = i32; L.mcomh_name_decode.argtypes = [vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.mcomh_fastq_names_to_device.restype = i32; L.mcomh_fastq_names_to_device.argtypes = [cp, i32, sz, C.POINTER(vp), C.POINTER(u64), C.POINTER(sz), C.c_char_p, sz]
    L.mcomh_fastq_name_member.restype = i32; L.mcomh_fastq_name_member.argtypes = [cp, i32, cp, C.POINTER(u64), C.c_char_p, sz]
    L.mcomh_verify_names_gpu.restype = i32; L.mcomh_verify_names_gpu.argtypes = [cp, cp, i32, C.POINTER(VerifyReport)]
    L.mcomh_name_pack_file.restype = i32; L.mcomh_name_pack_file.argtypes = [cp, cp, i32]
    L.mcomh_name_unpack_file.restype = i32; L.mcomh_name_unpack_file.argtypes = [cp, cp, i32]
    L.mcomh_name_info_mate.restype = i32; L.mcomh_name_info_mate.argtypes = [vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.mcomh_name_encode_mate.restype = i32; L.mcomh_name_encode_mate.argtypes = [vp, u64, u64, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.mcomh_name_decode_mate.restype = i32; L.mcomh_name_decode_mate.argtypes = [vp, u64, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.mcomh_name_pack_file_mate.restype = i32; L.mcomh_name_pack_file_mate.argtypes = [cp, cp, cp, i32]
    L.mcomh_name_unpack_file_mate.restype = i32; L.mcomh_name_unpack_file_mate.argtypes = [cp, cp, cp, i32]
    L.mcomh_cluster_dump_order_pe.restype = i32; L.mcomh_cluster_dump_order_pe.argtypes = [vp, cp]
    for f in ("mcomh_decompress_order_pe", "mcomh_decompress_fastq_order_pe"):
        getattr(L, f).restype = i32; getattr(L, f).argtypes = [cp, cp, cp, C.POINTER(u64)]
        getattr(L, f + "_gpu").restype = i32; getattr(L, f + "_gpu").argtypes = [cp, cp, cp, C.POINTER(u64), i32]
    L.mcomh_verify_order_pe_reads_gpu.restype = i32; L.mcomh_verify_order_pe_reads_gpu.argtypes = [cp, cp, cp, i32, C.POINTER(VerifyReport)]
    L.mcomh_verify_order_pe_gpu.restype = i32; L.mcomh_verify_order_pe_gpu.argtypes = [cp, cp, cp, i32, C.POINTER(VerifyReport)]
    L.mcomh_verify_order_pe_parts_gpu.restype = i32; L.mcomh_verify_order_pe_parts_gpu.argtypes = [cp, cp, cp, i32, C.POINTER(VerifyReport), C.POINTER(i32)]
    L.mcomh_verify_quality_member_gpu.restype = i32; L.mcomh_verify_quality_member_gpu.argtypes = [cp, cp, cp, i32, C.POINTER(VerifyReport)]
    L.mcomh_verify_names_member_gpu.restype = i32; L.mcomh_verify_names_member_gpu.argtypes = [cp, cp, cp, cp, i32, C.POINTER(VerifyReport)]
    L.mcomh_fastq_name_member_mate.restype = i32; L.mcomh_fastq_name_member_mate.argtypes = [cp, cp, i32, cp, C.POINTER(u64), C.c_char_p, sz]
    L.mcomh_fastq_lengths_file.restype = i32; L.mcomh_fastq_lengths_file.argtypes = [cp, i32, sz, cp, C.POINTER(u64), C.POINTER(i32), C.POINTER(u64), C.c_char_p, sz]
    L.mcomh_fastq_ragged_files.restype = i32; L.mcomh_fastq_ragged_files.argtypes = [cp, i32, i32, i32, cp, sz, cp, cp, C.POINTER(u64), C.c_char_p, sz]
    L.mcomh_fastq_to_device_ragged.restype = i32; L.mcomh_fastq_to_device_ragged.argtypes = [cp, i32, i32, cp, sz, C.POINTER(vp), C.POINTER(sz), cp, C.c_char_p, sz]
    L.mcomh_fastq_quality_member_ragged.restype = i32; L.mcomh_fastq_quality_member_ragged.argtypes = [cp, i32, i32, cp, cp, cp, C.POINTER(u64), C.c_char_p, sz]
    L.mcomh_fastq_emit_ragged.restype = i32; L.mcomh_fastq_emit_ragged.argtypes = [vp, u64, u64, vp, u64, C.POINTER(u64)]
    L.mcomh_verify_ragged_gpu.restype = i32; L.mcomh_verify_ragged_gpu.argtypes = [cp, cp, i32, C.POINTER(VerifyReport), C.POINTER(i32)]
    L.mcomh_fastq_record_hashes.restype = i32; L.mcomh_fastq_record_hashes.argtypes = [vp, u64, vp, u64, u64, i32, u64, vp, vp, vp, vp]
    L.mcomh_digest_reduce.restype = i32; L.mcomh_digest_reduce.argtypes = [vp, vp, vp, vp, vp, vp, u64, vp]
    L.mcomh_fastq_digest_files.restype = i32; L.mcomh_fastq_digest_files.argtypes = [cp, cp, i32, i32, i32, sz, cp, C.POINTER(u64), C.c_char_p, sz]
    L.mcomh_digest_print.restype = i32; L.mcomh_digest_print.argtypes = [C.POINTER(Digest), C.c_char_p, sz, C.POINTER(sz)]
    L.mcomh_digest_parse.restype = i32; L.mcomh_digest_parse.argtypes = [C.c_char_p, sz, C.POINTER(Digest), C.c_char_p, sz]
    L.mcomh_digest_check.restype = i32; L.mcomh_digest_check.argtypes = [cp, cp, cp, i32, C.POINTER(DigestReport)]
    for f in ("mcomh_decompress_order_range", "mcomh_decompress_fastq_range"):
        getattr(L, f).restype = i32; getattr(L, f).argtypes = [cp, cp, u64, u64, C.POINTER(u64), i32]
    L.mcomh_decompress_order_pe_range.restype = i32; L.mcomh_decompress_order_pe_range.argtypes = [cp, cp, cp, u64, u64, C.POINTER(u64), i32, i32]
    L.mcomh_qual_decode_rows.restype = i32; L.mcomh_qual_decode_rows.argtypes = [vp, u64, u64, u64, vp, u64, C.POINTER(u64), C.POINTER(u32)]
    L.mcomh_odd_text_append.restype = None; L.mcomh_odd_text_append.argtypes = [vp, u64, vp, u64, u64]
    L.mcomh_odd_index_build.restype = i32; L.mcomh_odd_index_build.argtypes = [vp, u64, C.POINTER(vp)]
    L.mcomh_odd_index_free.restype = None; L.mcomh_odd_index_free.argtypes = [vp]
    L.mcomh_odd_index_size.restype = u64; L.mcomh_odd_index_size.argtypes = [vp]
    L.mcomh_odd_align.restype = i32; L.mcomh_odd_align.argtypes = [vp, vp, u64, vp, vp, u64, vp]
    L.mcomh_odd_align_encode.restype = i32; L.mcomh_odd_align_encode.argtypes = [vp, vp, vp, u64, vp, u64, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64)]
    L.mcomh_odd_align_decode.restype = i32; L.mcomh_odd_align_decode.argtypes = [vp, u64, vp, u64, vp, u64, vp, u64, vp, C.POINTER(u32)]
    L.mcomh_odd_align_refusal.restype = C.c_char_p; L.mcomh_odd_align_refusal.argtypes = [u32]
    L.mcomh_odd_align_folder.restype = i32; L.mcomh_odd_align_folder.argtypes = [cp, i32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.c_char_p, sz]
    _lib = L
    return L


HOST_ABI_SYMBOLS = ["mcomh_create", "mcomh_create_streamed", "mcomh_create_packed", "mcomh_create_from_fastq", "mcomh_set_records", "mcomh_destroy", "mcomh_last_error", "mcomh_kt_for_reads", "mcomh_kt_for_bucket",
                    "mcomh_combine_cluster", "mcomh_update_single", "mcomh_realign_hash", "mcomh_stage2", "mcomh_pre_process",
                    "mcomh_dump_stages", "mcomh_cluster_dump", "mcomh_decompress", "mcomh_n_contigs", "mcomh_contig_ref", "mcomh_contig_n", "mcomh_contig_members",
                    "mcomh_list", "mcomh_stat", "mcomh_prof_enable", "mcomh_prof_read", "mcomh_prof_kernels", "mcomh_fastq_read", "mcomh_fastq_to_device",
                    "mcomh_device_free", "mcomh_cluster_dump_order", "mcomh_decompress_order",
                    "mcomh_cluster_dump_pe", "mcomh_decompress_pe", "mcomh_fastq_pair_to_device",
                    "mcomh_decompress_gpu", "mcomh_decompress_order_gpu", "mcomh_decompress_pe_gpu", "mcomh_decompress_gpu_times", "mcomh_verify_gpu",
                    "mcomh_contig_set", "mcomh_result_digest",
                    # the built-in entropy stage (host/mcom_entropy.cpp)
                    "mcomh_rans_bound", "mcomh_rans_estimate", "mcomh_rans_encode", "mcomh_rans_decode", "mcomh_entropy_pack_file",
                    "mcomh_entropy_unpack_file", "mcomh_entropy_times",
                    # the block-sorting coder (host/mcom_bwt.cpp)
                    "mcomh_bwt_bound", "mcomh_bwt_encode", "mcomh_bwt_decode", "mcomh_bwt_raw_len", "mcomh_bwt_stages", "mcomh_bwt_pack_file",
                    "mcomh_bwt_unpack_file",
                    # quality values (host/mcom_qual.cpp)
                    "mcomh_qual_bound", "mcomh_qual_info", "mcomh_qual_estimate", "mcomh_qual_encode", "mcomh_qual_decode",
                    "mcomh_qual_pack_file", "mcomh_qual_unpack_file", "mcomh_fastq_quality_member", "mcomh_device_copy",
                    "mcomh_fastq_qualities_to_device", "mcomh_decompress_fastq", "mcomh_decompress_fastq_gpu", "mcomh_verify_quality_gpu",
                    # quality values in the archive's own order (`minicom -q`)
                    "mcomh_keep_read_order", "mcomh_qual_gather_rows", "mcomh_fastq_quality_member_ordered", "mcomh_decompress_fastq_reordered",
                    "mcomh_decompress_fastq_reordered_gpu", "mcomh_decompress_fastq_pe", "mcomh_decompress_fastq_pe_gpu", "mcomh_verify_records_gpu",
                    # read names and '+' lines (host/mcom_names.cpp)
                    "mcomh_name_bound", "mcomh_name_info", "mcomh_name_encode", "mcomh_name_decode", "mcomh_name_pack_file",
                    "mcomh_name_unpack_file", "mcomh_fastq_names_to_device", "mcomh_fastq_name_member", "mcomh_verify_names_gpu",
                    # names coded against a mate file's names (section 3.12)
                    "mcomh_name_info_mate", "mcomh_name_encode_mate", "mcomh_name_decode_mate", "mcomh_name_pack_file_mate",
                    "mcomh_name_unpack_file_mate", "mcomh_fastq_name_member_mate",
                    # a pair kept in input order (section 3.12)
                    "mcomh_cluster_dump_order_pe", "mcomh_decompress_order_pe", "mcomh_decompress_order_pe_gpu", "mcomh_decompress_fastq_order_pe",
                    "mcomh_decompress_fastq_order_pe_gpu", "mcomh_verify_order_pe_reads_gpu", "mcomh_verify_order_pe_parts_gpu", "mcomh_verify_order_pe_gpu",
                    "mcomh_verify_quality_member_gpu", "mcomh_verify_names_member_gpu",
                    # lossy quality values (`minicom -b`, host/mcom_qual_lossy.cpp)
                    "mcomh_qual_lossy_parse", "mcomh_qual_lossy_print", "mcomh_qual_transform", "mcomh_qual_pack_file_lossy", "mcomh_fastq_quality_member_lossy",
                    "mcomh_qual_lossy_marker",
                    # consensus-guided lossy quality values (`minicom -a`, host/mcom_agree.cpp)
                    "mcomh_agree_mask", "mcomh_qual_agree", "mcomh_fastq_quality_member_agree", "mcomh_qual_agree_marker",
                    # BGZF output (`minicom -d -z`, host/mcom_bgzf.cpp)
                    "mcomh_bgzf_bound", "mcomh_bgzf_encode", "mcomh_bgzf_file",
                    # BGZF input inflated on the GPU (host/mcom_gzip_gpu.cpp)
                    "mcomh_gzip_inflate_members", "mcomh_gzip_inflate", "mcomh_gunzip_file",
                    # reads of differing lengths (`minicom -p -V`, host/mcom_ragged.cpp)
                    "mcomh_fastq_lengths_file", "mcomh_fastq_ragged_files", "mcomh_fastq_to_device_ragged", "mcomh_fastq_quality_member_ragged",
                    "mcomh_fastq_emit_ragged", "mcomh_verify_ragged_gpu",
                    # self-checking archives (`minicom -K`, host/mcom_digest.cpp)
                    "mcomh_fastq_record_hashes", "mcomh_digest_reduce", "mcomh_fastq_digest_files", "mcomh_digest_print", "mcomh_digest_parse", "mcomh_digest_check",
                    # a record range of a -p archive (`minicom -d -R`)
                    "mcomh_decompress_order_range", "mcomh_decompress_fastq_range", "mcomh_decompress_order_pe_range", "mcomh_qual_decode_rows",
                    # the odd reads of a -V archive against the contigs (`minicom -p -V -A`, host/mcom_odd_align.cpp)
                    "mcomh_odd_text_append", "mcomh_odd_index_build", "mcomh_odd_index_free", "mcomh_odd_index_size", "mcomh_odd_align", "mcomh_odd_align_encode",
                    "mcomh_odd_align_decode", "mcomh_odd_align_refusal", "mcomh_odd_align_folder",
                    # multi-GPU (bound in minicom_amd/distributed.py)
                    "mcomh_comm_unique_id", "mcomh_comm_create_rccl", "mcomh_comm_create_ops", "mcomh_comm_destroy", "mcomh_comm_rank",
                    "mcomh_comm_world", "mcomh_comm_last_error", "mcomh_comm_alltoallv", "mcomh_comm_allgatherv", "mcomh_comm_allreduce_u64",
                    "mcomh_comm_stats", "mcomh_comm_seconds", "mcomh_create_dist", "mcomh_pool_trim"]


def decompress(folder: str, out_path: str, order: bool = False, device: int | None = None) -> int:
    """mcomh_decompress(_order): stream files -> one read per line (order=True: the -p file set, original order).
    Returns the number of reads.  device=None: the host decoder; an integer: the reads are rebuilt on that GPU
    (mcomh_decompress(_order)_gpu: the same bytes; an error, never the host decoder, when there is no such GPU)."""
    n = C.c_uint64()
    lib = load_host_library()
    if device is None:
        rc = (lib.mcomh_decompress_order if order else lib.mcomh_decompress)(folder.encode(), out_path.encode(), C.byref(n))
    else:
        rc = (lib.mcomh_decompress_order_gpu if order else lib.mcomh_decompress_gpu)(folder.encode(), out_path.encode(), C.byref(n), int(device))
    if rc:
        raise McomError(f"cannot decode the stream files in {folder}" + ("" if device is None else f" on GPU {device}"))
    return int(n.value)


def decompress_range(folder: str, out_path: str, first: int, count: int, device: int | None = None, fastq: bool = False, out_path2: str | None = None) -> int:
    """mcomh_decompress_order_range / _fastq_range / _order_pe_range: records first .. first + count - 1 (first
    from 0, the range clipped at the archive's end) of a -p archive, and nothing else: one read per line, with fastq=True four-line
    records; with out_path2 the same range of both files of a pair kept in input order.  Ranges that tile the archive concatenate to the
    full decode.  device=None: the host twin (the whole table in memory, then the slice); an integer: on that GPU, where only the window's
    rows are made.  Returns the number of records written.  McomError, and no file, for first > n and for a folder that is not a -p
    archive, or is one made with -q or -V."""
    if first < 0 or count < 0 or first >= 2 ** 64 or count >= 2 ** 64:
        raise McomError(f"decompress_range: records {first} .. + {count}")
    n = C.c_uint64()
    lib = load_host_library()
    dev = -1 if device is None else int(device)
    if out_path2 is not None:
        rc = lib.mcomh_decompress_order_pe_range(os.fsencode(folder), os.fsencode(out_path), os.fsencode(out_path2), int(first), int(count), C.byref(n), dev, 1 if fastq else 0)
    else:
        rc = (lib.mcomh_decompress_fastq_range if fastq else lib.mcomh_decompress_order_range)(os.fsencode(folder), os.fsencode(out_path), int(first), int(count), C.byref(n), dev)
    if rc:
        raise McomError(f"cannot decode records {first} .. + {count} of {folder}" + ("" if device is None else f" on GPU {device}") +
                        ": the range begins behind the last record, or the folder is not a complete, consistent -p archive (archives made with -q or -V are refused)")
    return int(n.value)


def verify(folder: str, fastq: str, fastq2: str | None = None, order: bool = False, device: int = 0) -> dict:
    """mcomh_verify_gpu: do the stream files in `folder` give back exactly the reads of `fastq` (and, for a paired-end archive, the
    mates of `fastq2`)?  Decided on GPU `device`, nothing is written.  order=True: a -p archive, line against line; otherwise the
    reads (pairs) as a multiset.  Returns the report; McomError when no comparison could be made (an archive the decoders refuse, an
    unreadable FASTQ or one of another read length, no such GPU, no room on the card) -- a difference is a verdict, not an error."""
    if fastq is None or folder is None:
        raise McomError("verify needs a folder and a FASTQ file")
    if order and fastq2 is not None:
        raise McomError("-p is a single-end option: no second FASTQ file")
    mode = 2 if fastq2 is not None else 1 if order else 0
    r = VerifyReport()
    rc = load_host_library().mcomh_verify_gpu(os.fsencode(folder), mode, os.fsencode(fastq), os.fsencode(fastq2) if fastq2 is not None else None,
                                              int(device), C.byref(r))
    if rc:
        raise McomError(f"cannot verify the stream files in {folder} against {fastq} on GPU {device}")
    t = r.times_ms
    return {"identical": bool(r.identical), "mode": ("default", "order", "paired")[r.mode], "n_input": int(r.n_input), "n_archive": int(r.n_archive),
            "missing": int(r.missing), "extra": int(r.extra), "differing": int(r.differing),
            "first_diff": None if r.first_diff == 2 ** 64 - 1 else int(r.first_diff), "exact_runs": int(r.exact_runs),
            "missing_examples": [int(v) for v in r.missing_ex[: r.n_missing_ex]], "extra_examples": [int(v) for v in r.extra_ex[: r.n_extra_ex]],
            "times_ms": {"ingest": t[0], "upload_index": t[1], "decode": t[2], "compare": t[3], "total": t[4], "read_files": t[5],
                         "compare_device": t[6], "decode_kernels": t[7]}}


def decompress_gpu_times() -> dict:
    """mcomh_decompress_gpu_times: where the last GPU decode of this process spent its time, in ms."""
    t = (C.c_double * 8)()
    load_host_library().mcomh_decompress_gpu_times(t)
    return {"read_files_ms": t[0], "upload_index_ms": t[1], "decode_wall_ms": t[2], "decode_kernels_ms": t[3],
            "download_write_ms": t[4], "write_ms": t[5], "total_ms": t[6]}


RANS_MODELS = ((0, 1), (1, 1), (1, 2), (1, 4), (2, 1), (2, 2), (2, 4))     # (model, stride) in the order of mcomh_rans_estimate


def rans_encode(data: bytes, model: int | None = None, stride: int = 1) -> bytes:
    """mcomh_rans_encode, the host twin of the GPU coder: raw bytes -> a `.rans` member.  model None: chosen by estimated size;
    0 stored, 1 order-0, 2 order-1 with `stride` 1, 2 or 4 force one."""
    lib = load_host_library()
    n = len(data)
    cap = 32 + n if model is None else int(lib.mcomh_rans_bound(n))
    out = C.create_string_buffer(cap)
    got = C.c_uint64()
    src = (C.c_char * n).from_buffer_copy(data) if n else None
    rc = lib.mcomh_rans_encode(src, n, out, cap, C.byref(got), 0 if model is None else 0x100 | (model << 4) | stride)
    if rc:
        raise McomError(f"rans_encode: error {rc}")
    return out.raw[:got.value]


def bgzf_encode(data: bytes, device: int | None = None, eof: bool = True) -> bytes:
    """The bytes of `data` as BGZF members of 65280 bytes of text each, closed with the empty member a file ends
    with unless eof=False.  device None: mcomh_bgzf_encode, the host twin; an integer: mcom_bgzf_encode on that GPU -- the same bytes."""
    n = len(data)
    if device is not None:
        import numpy as np
        import torch
        from .hip import Context
        raw = torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).to(f"cuda:{int(device)}") if n else torch.empty(0, dtype=torch.uint8, device=f"cuda:{int(device)}")
        return bytes(Context(int(device)).bgzf_encode(raw, eof=eof).cpu().numpy())
    lib = load_host_library()
    cap = int(lib.mcomh_bgzf_bound(n))
    out = C.create_string_buffer(cap)
    got = C.c_uint64()
    src = (C.c_char * n).from_buffer_copy(data) if n else None
    rc = lib.mcomh_bgzf_encode(src, n, out, cap, C.byref(got), 1 if eof else 0)
    if rc:
        raise McomError(f"bgzf_encode: error {rc}")
    return out.raw[:got.value]


def bgzf_file(in_path: str, out_path: str, device: int | None = None) -> None:
    """mcomh_bgzf_file: a file -> the BGZF file of its bytes (what `mcomz z` runs).  device None: the host twin; an integer: that GPU (an
    error, never the twin, when there is no such GPU).  No output file is left by a call that fails."""
    if load_host_library().mcomh_bgzf_file(os.fsencode(in_path), os.fsencode(out_path), -1 if device is None else int(device)):
        raise McomError(f"cannot write {in_path} as BGZF to {out_path}" + ("" if device is None else f" on GPU {device}"))


def gzip_walk(data: bytes):
    """mcom_gzip_walk over a BGZF buffer: (table, text_bytes, used, ok).  table: numpy array of hip.GZIP_MEMBER_DTYPE with the whole
    members in front of the first stop, text_bytes the sum of their ISIZEs, used the bytes they take; ok False when the walk stopped at
    a member without a `BC` field, with reserved flag bits or of a size that leaves the buffer."""
    import numpy as np
    from .hip import GZIP_MEMBER_DTYPE, load_library
    lib = load_library()
    n = len(data)
    src = (C.c_char * n).from_buffer_copy(data) if n else None
    cnt, text, used = C.c_uint64(), C.c_uint64(), C.c_uint64()
    lib.mcom_gzip_walk(src, n, None, 0, C.byref(cnt), C.byref(text), C.byref(used))
    tab = np.zeros(cnt.value, dtype=GZIP_MEMBER_DTYPE)
    rc = lib.mcom_gzip_walk(src, n, tab.ctypes.data if cnt.value else None, cnt.value, C.byref(cnt), C.byref(text), C.byref(used)) if cnt.value else \
        lib.mcom_gzip_walk(src, n, None, 0, C.byref(cnt), C.byref(text), C.byref(used))
    return tab[:cnt.value], int(text.value), int(used.value), rc == 0 and used.value == n


def gzip_inflate_members(data: bytes, table, out_bytes: int | None = None, device: int | None = None, fill: int = 0):
    """The members `table` (hip.GZIP_MEMBER_DTYPE) of `data` into a buffer of out_bytes (default: the end of the last slot) that starts
    out filled with `fill`: (buffer, statuses), both bytes.  device None: mcomh_gzip_inflate_members, the host twin; an integer:
    mcom_gzip_inflate on that GPU -- the same bytes in every slot of a member that is OK and the same statuses."""
    import numpy as np
    from .hip import GZIP_MEMBER_DTYPE
    tab = np.ascontiguousarray(table, dtype=GZIP_MEMBER_DTYPE)
    n, nin = int(tab.shape[0]), len(data)
    if out_bytes is None:
        out_bytes = int((tab["out_off"] + tab["isize"]).max()) if n else 0
    if device is not None:
        import torch
        from .hip import Context
        dev = f"cuda:{int(device)}"
        raw = torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).to(dev) if nin else torch.empty(0, dtype=torch.uint8, device=dev)
        out = torch.full((out_bytes,), fill, dtype=torch.uint8, device=dev)
        out, status = Context(int(device)).gzip_inflate(raw, tab, out=out)
        return bytes(out.cpu().numpy()), bytes(status.cpu().numpy())
    lib = load_host_library()
    src = (C.c_char * nin).from_buffer_copy(data) if nin else None
    out = (C.c_char * max(out_bytes, 1)).from_buffer_copy(bytes([fill]) * max(out_bytes, 1))
    status = C.create_string_buffer(max(n, 1))
    bad, first = C.c_uint64(), C.c_uint64()
    if lib.mcomh_gzip_inflate_members(src, nin, tab.ctypes.data if n else None, n, out, out_bytes, status, C.byref(bad), C.byref(first)):
        raise McomError("gzip_inflate: a member's payload or slot leaves its buffer, or slots overlap or are out of order")
    return out.raw[:out_bytes], status.raw[:n]


def gzip_inflate(data: bytes, device: int | None = None):
    """A BGZF buffer to (text, statuses): its members by mcom_gzip_walk, inflated by the host twin (device None) or by mcom_gzip_inflate
    on that GPU.  statuses: one MCOM_GZIP_* byte per member; the text of a member that is not OK is unspecified inside its own slot.
    McomError when the buffer is not BGZF members to its end."""
    tab, text, used, ok = gzip_walk(data)
    if not ok:
        raise McomError(f"gzip_inflate: no BGZF member at byte {used}")
    return gzip_inflate_members(data, tab, text, device)


def gunzip_file(in_path: str, out_path: str, device: int | None = None) -> None:
    """mcomh_gunzip_file: a BGZF file -> its text (what `mcomz u` runs).  device None: the host twin; an integer: that GPU (an error, never
    the twin, when there is no such GPU).  No output file is left when a member is refused or the file is not BGZF to its end."""
    if load_host_library().mcomh_gunzip_file(os.fsencode(in_path), os.fsencode(out_path), -1 if device is None else int(device)):
        raise McomError(f"cannot inflate {in_path} to {out_path}" + ("" if device is None else f" on GPU {device}"))


def rans_decode(member: bytes, cap: int | None = None) -> bytes:
    """mcomh_rans_decode: a `.rans` member -> the raw bytes; McomError for one that is truncated, malformed or fails its CRC-32."""
    lib = load_host_library()
    n = len(member)
    if cap is None:
        cap = int.from_bytes(member[8:16], "little") if n >= 16 else 0
        if cap > 1 << 40:
            raise McomError("rans_decode: the header asks for %d bytes" % cap)
    out = C.create_string_buffer(max(cap, 1))
    got = C.c_uint64()
    src = (C.c_char * n).from_buffer_copy(member) if n else None
    rc = lib.mcomh_rans_decode(src, n, out, cap, C.byref(got))
    if rc:
        raise McomError(f"rans_decode: error {rc}: not a complete, intact .rans member")
    return out.raw[:got.value]


def fastq_qualities(path: str, L: int, device: int = 0, piece_bytes: int = 0):
    """mcomh_fastq_qualities_to_device: the quality lines of a four-line FASTQ file (plain or .gz) as a uint8 device tensor [n, L].
    piece_bytes: the size of the two page-locked pieces the text goes up through (0 = 32 MiB; a request below 4 * (2 L + 64) bytes is
    raised to that -- 552 bytes at L = 37 -- so that a piece holds a few records; tests pass small sizes so that records straddle pieces).  McomError, naming the first bad record, for a file the kernel flags."""
    import torch
    lib = load_host_library()
    err = C.create_string_buffer(320)
    d, n = C.c_void_p(), C.c_size_t()
    if lib.mcomh_fastq_qualities_to_device(os.fsencode(path), int(device), int(L), int(piece_bytes), C.byref(d), C.byref(n), err, 320):
        raise McomError(f"{path}: {err.value.decode() or 'cannot read the qualities'}")
    try:
        out = torch.empty((int(n.value), int(L)), dtype=torch.uint8, device=f"cuda:{int(device)}")
        if n.value:
            if lib.mcomh_device_copy(out.data_ptr(), d, int(n.value) * int(L)):
                raise McomError("fastq_qualities: copy failed")
    finally:
        lib.mcomh_device_free(d)
    return out


def qual_lossy_spec(spec) -> QualLossySpec:
    """mcomh_qual_lossy_parse: the canonical text of a lossy spec (`ill8`, `thr:T:LO:HI`, `pblock:P`) -> the
    structure the C calls take.  A QualLossySpec passes through (a general byte map is made with QualLossySpec.from_lut).  McomError for
    anything else: another spelling, leading zeros, trailing text, a thr that is not idempotent."""
    if isinstance(spec, QualLossySpec):
        return spec
    s = QualLossySpec()
    text = spec.encode() if isinstance(spec, str) else bytes(spec)
    if b"\0" in text or load_host_library().mcomh_qual_lossy_parse(text, C.byref(s)):
        raise McomError("not a lossy spec: %r (ill8, thr:T:LO:HI with 0 <= LO < T <= HI <= 93, pblock:P with 1 <= P <= 47; decimal, no leading zeros)" % (spec,))
    return s


def qual_lossy_text(spec) -> str:
    """mcomh_qual_lossy_print: the canonical text of a spec (what qual_lossy.txt holds in front of its newline)"""
    out = C.create_string_buffer(32)
    if load_host_library().mcomh_qual_lossy_print(C.byref(qual_lossy_spec(spec)), out, 32):
        raise McomError("qual_lossy_text: a general byte map has no text")
    return out.value.decode()


def qual_transform(rows, spec, device: int | None = None):
    """The lossy transform of a quality matrix: rows, a uint8 matrix [n, L] with contiguous rows (any row stride
    >= L), is left alone; returns (the transformed matrix [n, L], the report {"changed", "sum_abs", "sum_sq", "max_abs"}).  device=None:
    mcomh_qual_transform, the host twin; an integer: mcom_qual_transform on that GPU -- the same bytes and the same report.  McomError
    for a spec the transform refuses."""
    s = qual_lossy_spec(spec)
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.dtype != np.uint8 or (rows.size and rows.strides[1] != 1):
        raise McomError("qual_transform: a uint8 matrix with contiguous rows")
    n, L = rows.shape
    if device is not None:
        import torch
        from .hip import Context
        out, rep = Context(int(device)).qual_transform(torch.from_numpy(np.ascontiguousarray(rows)).to(f"cuda:{int(device)}"), s)
        return out.cpu().numpy(), rep
    out = np.array(rows, dtype=np.uint8, order="C")
    r = QualLossyReport()
    if load_host_library().mcomh_qual_transform(out.ctypes.data if n else None, n, L, L, C.byref(s), C.byref(r)):
        raise McomError("qual_transform: rows of %d bytes, or a spec the transform refuses (a byte map that is not idempotent)" % L)
    return out, r.as_dict()


def qual_lossy_marker(folder: str):
    """mcomh_qual_lossy_marker: the canonical spec text of FOLDER/qual_lossy.txt, None without the file; McomError when the file holds
    anything but a canonical spec and a newline."""
    s = QualLossySpec(); out = C.create_string_buffer(40)
    rc = load_host_library().mcomh_qual_lossy_marker(os.fsencode(folder), C.byref(s), out, 40)
    if rc < 0:
        raise McomError(f"{folder}/qual_lossy.txt does not hold a lossy spec and a newline")
    return out.value.decode() if rc else None


# ---- consensus-guided lossy quality values (`minicom -a Q[:C]`, host/mcom_agree.cpp) ----
def agree_mask(folder: str, C_min: int = 3, device: int | None = None, out_path: str | None = None):
    """mcomh_agree_mask: the agreement mask of the stream files in `folder` (a default-mode or a -p archive): a uint8 matrix [n, ceil(L / 8)],
    row j beside row j of the decoder's image, column i in bit i & 7 of byte i >> 3.  Returns (mask, L, bits_set).  device=None: the host
    decoders' member loops; an integer: mcom_agree_coverage and mcom_agree_mask on that GPU -- the same bytes.  out_path: where the
    mask file is left (otherwise a temporary file that is removed).  McomError for a folder the matching decoder refuses, a paired-end
    default-mode archive, a ragged one, or C_min outside 1 .. 255; no file is left then."""
    import tempfile
    own = out_path is None
    if own:
        fd, out_path = tempfile.mkstemp(suffix=".mask"); os.close(fd); os.remove(out_path)
    n, L, bits = C.c_uint64(), C.c_int32(), C.c_uint64()
    try:
        if load_host_library().mcomh_agree_mask(os.fsencode(folder), int(C_min), os.fsencode(out_path), -1 if device is None else int(device), C.byref(n), C.byref(L), C.byref(bits)):
            raise McomError(f"{folder}: no agreement mask (not a complete, consistent default-mode or -p archive, or a coverage outside 1 .. 255)")
        mb = (int(L.value) + 7) // 8
        mask = np.fromfile(out_path, dtype=np.uint8).reshape(int(n.value), mb)
    finally:
        if own and os.path.exists(out_path):
            os.remove(out_path)
    return mask, int(L.value), int(bits.value)


def qual_agree(rows, mask, Q: int, first_mask_row: int = 0, device: int | None = None):
    """The agreement transform: rows uint8 [n, L] is left alone; returns (the matrix with 33 + Q wherever bit i of
    mask row first_mask_row + r is set, the report {"changed", "sum_abs", "sum_sq", "max_abs", "mask_bits"}).  mask: uint8 [m, >= ceil(L / 8)].
    device=None: mcomh_qual_agree, the host twin; an integer: mcom_qual_agree on that GPU -- the same bytes and the same report."""
    rows = np.asarray(rows); mask = np.ascontiguousarray(mask, dtype=np.uint8)
    if rows.ndim != 2 or rows.dtype != np.uint8 or mask.ndim != 2 or first_mask_row < 0 or first_mask_row + rows.shape[0] > mask.shape[0]:
        raise McomError("qual_agree: a uint8 matrix of rows and a mask with a row for each of them")
    n, L = rows.shape
    if device is not None:
        import torch
        from .hip import Context
        dev = f"cuda:{int(device)}"
        out, rep = Context(int(device)).qual_agree(torch.from_numpy(np.ascontiguousarray(rows)).to(dev), torch.from_numpy(mask).to(dev), int(Q), first_mask_row=int(first_mask_row))
        return out.cpu().numpy(), rep
    out = np.array(rows, dtype=np.uint8, order="C")
    r = QualAgreeReport()
    if load_host_library().mcomh_qual_agree(out.ctypes.data if n else None, n, L, L, mask.ctypes.data if mask.size else None, mask.shape[1], int(first_mask_row), int(Q), C.byref(r)):
        raise McomError("qual_agree: Q 0 .. 93, rows of 1 .. 256 bytes and mask rows of at least ceil(L / 8) bytes")
    return out, r.as_dict()


def qual_agree_marker(folder: str):
    """mcomh_qual_agree_marker: (Q, C) of FOLDER/qual_agree.txt, None without the file; McomError when it holds anything but `Q C` and a newline."""
    q, c = C.c_uint32(), C.c_uint32()
    rc = load_host_library().mcomh_qual_agree_marker(os.fsencode(folder), C.byref(q), C.byref(c))
    if rc < 0:
        raise McomError(f"{folder}/qual_agree.txt does not hold `Q C` (0 .. 93, 1 .. 255) and a newline")
    return (int(q.value), int(c.value)) if rc else None


def fastq_quality_member_agree(fastq: str, L: int, out_path: str, mask_path: str, Q: int, first_mask_row: int = 0, device: int | None = None, order_path: str | None = None, lossy=None):
    """mcomh_fastq_quality_member_agree: fastq_quality_member with the agreement transform behind the gather and in front of the lossy
    transform (when one is given).  Returns (records, agreement report, lossy report or None)."""
    err = C.create_string_buffer(320)
    n = C.c_uint64(); ar = QualAgreeReport(); lr = QualLossyReport()
    s = qual_lossy_spec(lossy) if lossy is not None else None
    if load_host_library().mcomh_fastq_quality_member_agree(os.fsencode(fastq), int(L), -1 if device is None else int(device), None if order_path is None else os.fsencode(order_path),
                                                            os.fsencode(mask_path), int(first_mask_row), int(Q), C.byref(s) if s is not None else None, os.fsencode(out_path), C.byref(n),
                                                            C.byref(ar), C.byref(lr), err, 320):
        raise McomError(f"{fastq}: {err.value.decode() or 'cannot code the qualities'}")
    return int(n.value), ar.as_dict(), (lr.as_dict() if s is not None else None)


def fastq_quality_member(fastq: str, L: int, out_path: str, device: int | None = None, order_path: str | None = None, lossy=None):
    """mcomh_fastq_quality_member: the quality lines of a four-line FASTQ file -> the `.mcq` member file out_path; returns the number of
    records.  device=None: the host twin (same record rules, same member); an integer: gathered and coded on that GPU.
    order_path (mcomh_fastq_quality_member_ordered): a read_order.bin; row j of the member is then record order[j]
    of the file.  McomError, and no member, when it is not a permutation of the records.
    lossy (mcomh_fastq_quality_member_lossy): a lossy spec; the rows go through the transform in front of the coder
    and the call returns (records, report) instead."""
    err = C.create_string_buffer(320)
    n = C.c_uint64()
    if lossy is not None:
        s = qual_lossy_spec(lossy); r = QualLossyReport()
        if load_host_library().mcomh_fastq_quality_member_lossy(os.fsencode(fastq), int(L), -1 if device is None else int(device), None if order_path is None else os.fsencode(order_path),
                                                                C.byref(s), os.fsencode(out_path), C.byref(n), C.byref(r), err, 320):
            raise McomError(f"{fastq}: {err.value.decode() or 'cannot code the qualities'}")
        return int(n.value), r.as_dict()
    if order_path is not None:
        if load_host_library().mcomh_fastq_quality_member_ordered(os.fsencode(fastq), int(L), -1 if device is None else int(device), os.fsencode(order_path), os.fsencode(out_path),
                                                                  C.byref(n), err, 320):
            raise McomError(f"{fastq}: {err.value.decode() or 'cannot code the qualities'}")
        return int(n.value)
    if load_host_library().mcomh_fastq_quality_member(os.fsencode(fastq), int(L), -1 if device is None else int(device), os.fsencode(out_path), C.byref(n), err, 320):
        raise McomError(f"{fastq}: {err.value.decode() or 'cannot code the qualities'}")
    return int(n.value)


# ---- reads of differing lengths (`minicom -p -V`, host/mcom_ragged.cpp) ----
def fastq_lengths(fastq: str, out_path: str, device: int | None = None, piece_bytes: int = 0):
    """mcomh_fastq_lengths_file: one pass over a four-line FASTQ file (plain or .gz) whose reads may differ in length.  Every record is
    checked, out_path gets len.bin (one byte, length - 1, per record).  Returns (n, L, n_odd): the records, the modal sequence length
    (ties: the larger), the records of another length.  device=None: the host twin; an integer: on that GPU, the text going up in
    pieces of piece_bytes (0: 32 MiB).  McomError names the first bad record."""
    err = C.create_string_buffer(320)
    n, L, n_odd = C.c_uint64(), C.c_int32(), C.c_uint64()
    if load_host_library().mcomh_fastq_lengths_file(os.fsencode(fastq), -1 if device is None else int(device), int(piece_bytes), os.fsencode(out_path), C.byref(n), C.byref(L),
                                                    C.byref(n_odd), err, 320):
        raise McomError(f"{fastq}: {err.value.decode() or 'cannot take the lengths'}")
    return int(n.value), int(L.value), int(n_odd.value)


def fastq_ragged_files(fastq: str, which: int, L: int, len_path: str, out_rows: str, out_odd: str, device: int | None = None, piece_bytes: int = 0) -> int:
    """mcomh_fastq_ragged_files: line `which` (1: sequence, 3: quality) of every record, split by the lengths in len_path: the lines of L
    bytes as raw rows to out_rows, the others back to back to out_odd.  Returns n_even.  device as for fastq_lengths."""
    err = C.create_string_buffer(320)
    ne = C.c_uint64()
    if load_host_library().mcomh_fastq_ragged_files(os.fsencode(fastq), int(which), int(L), -1 if device is None else int(device), os.fsencode(len_path), int(piece_bytes),
                                                    os.fsencode(out_rows), os.fsencode(out_odd), C.byref(ne), err, 320):
        raise McomError(f"{fastq}: {err.value.decode() or 'cannot split the file'}")
    return int(ne.value)


def fastq_quality_member_ragged(fastq: str, L: int, len_path: str, out_mcq: str, out_odd_qual: str, device: int | None = None) -> int:
    """mcomh_fastq_quality_member_ragged: qual.mcq over the records of L bases and the quality lines of the others (odd.qual).  Returns the
    rows of the member."""
    err = C.create_string_buffer(320)
    ne = C.c_uint64()
    if load_host_library().mcomh_fastq_quality_member_ragged(os.fsencode(fastq), int(L), -1 if device is None else int(device), os.fsencode(len_path), os.fsencode(out_mcq),
                                                             os.fsencode(out_odd_qual), C.byref(ne), err, 320):
        raise McomError(f"{fastq}: {err.value.decode() or 'cannot code the qualities'}")
    return int(ne.value)


# ---- self-checking archives (`minicom -K`, host/mcom_digest.cpp) ----
def fastq_digest(path: str, path2: str | None = None, lines_per_record: int = 4, with_qual: bool = True, device: int | None = None, piece_bytes: int = 0, out_path: str | None = None) -> str:
    """mcomh_fastq_digest_files: the text of digest.txt for one FASTQ file (plain or .gz), or for a pair.  lines_per_record 1: a file of one
    read per line (sequence keys only); with_qual=False leaves the quality keys out.  device=None: the host twin; an integer: on that GPU,
    the text going up in pieces of piece_bytes (0: 32 MiB).  out_path: the file is kept there as well.  McomError names the first record
    that is none, or says that the two files differ in their record counts; no file is left behind then."""
    import tempfile
    err = C.create_string_buffer(400)
    n = C.c_uint64()
    with tempfile.TemporaryDirectory() as td:
        out = out_path if out_path is not None else os.path.join(td, "digest.txt")
        if load_host_library().mcomh_fastq_digest_files(os.fsencode(path), None if path2 is None else os.fsencode(path2), int(lines_per_record), 1 if with_qual else 0,
                                                        -1 if device is None else int(device), int(piece_bytes), os.fsencode(out), C.byref(n), err, 400):
            raise McomError(err.value.decode() or f"{path}: cannot take the digest")
        with open(out, "rb") as f:
            return f.read().decode()


def digest_parse(text) -> dict:
    """mcomh_digest_parse: {"files", "n", key: (word of seed 1, word of seed 2)} of a digest.txt; McomError with the reason for anything
    not written exactly as mcomh_digest_print writes it."""
    b = text.encode() if isinstance(text, str) else bytes(text)
    d = Digest()
    why = C.create_string_buffer(128)
    if load_host_library().mcomh_digest_parse(b, len(b), C.byref(d), why, 128):
        raise McomError("not a digest: " + why.value.decode())
    out = {"files": int(d.files), "n": int(d.n)}
    for k, name in enumerate(DIGEST_KEYS):
        if d.present >> k & 1:
            out[name] = (int(d.sums[2 * k]), int(d.sums[2 * k + 1]))
    return out


def digest_check(folder: str, out1: str, out2: str | None = None, device: int | None = None) -> dict:
    """mcomh_digest_check: the decoder's output files against folder/digest.txt.  Returns {"identical", "compared": [keys], "differing":
    [keys], "first_diff": a key, "n" or None, "n_stored", "n_output"}; McomError when the check is refused."""
    r = DigestReport()
    if load_host_library().mcomh_digest_check(os.fsencode(folder), os.fsencode(out1), None if out2 is None else os.fsencode(out2), -1 if device is None else int(device), C.byref(r)):
        raise McomError("digest check refused: " + (r.message.decode() or "error"))
    keys = lambda bits: [name for k, name in enumerate(DIGEST_KEYS) if bits >> k & 1]  # noqa: E731
    return {"identical": bool(r.identical), "compared": keys(r.compared), "differing": keys(r.differing),
            "first_diff": None if r.first_diff == -1 else "n" if r.first_diff == -2 else DIGEST_KEYS[r.first_diff], "n_stored": int(r.n_stored), "n_output": int(r.n_output)}


def fastq_record_hashes_host(text: bytes, lines_per_record: int = 4, first_record: int = 0, n_total: int | None = None, with_qual: bool = True, with_names: bool = True):
    """mcomh_fastq_record_hashes over a text of whole records (the line index is made here).  Returns (hS, hQ, hN, flag bits, first flagged
    record or None): uint64 arrays [n_total, 2] (None where not asked for, or with lines_per_record 1)."""
    buf = np.frombuffer(bytes(text), dtype=np.uint8)
    nl = np.flatnonzero(buf == 10)
    start = np.concatenate([[0], nl + 1]).astype(np.uint64)
    n_rec = (len(start) - 1) // lines_per_record
    n_total = first_record + n_rec if n_total is None else int(n_total)
    four = lines_per_record == 4
    hS = np.zeros((max(n_total, 1), 2), dtype=np.uint64)
    hQ = np.zeros((max(n_total, 1), 2), dtype=np.uint64) if four and with_qual else None
    hN = np.zeros((max(n_total, 1), 2), dtype=np.uint64) if four and with_names else None
    flag = np.array([0, 0xFFFFFFFF], dtype=np.uint32)
    if load_host_library().mcomh_fastq_record_hashes(buf.ctypes.data if len(buf) else None, len(buf), start.ctypes.data, int(first_record), n_rec, int(lines_per_record), n_total,
                                                     hS.ctypes.data, None if hQ is None else hQ.ctypes.data, None if hN is None else hN.ctypes.data, flag.ctypes.data):
        raise McomError("fastq_record_hashes: bad arguments")
    return hS[:n_total], None if hQ is None else hQ[:n_total], None if hN is None else hN[:n_total], int(flag[0]), (None if flag[1] == 0xFFFFFFFF else int(flag[1]))


def digest_reduce_host(hS1, hQ1=None, hN1=None, hS2=None, hQ2=None, hN2=None):
    """mcomh_digest_reduce: the sixteen sums (word 2 * key + seed, keys in the order of DIGEST_KEYS) of uint64 arrays [n, 2]"""
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.uint64) for a in (hS1, hQ1, hN1, hS2, hQ2, hN2)]
    n = int(arrs[0].shape[0])
    sums = np.zeros(16, dtype=np.uint64)
    if load_host_library().mcomh_digest_reduce(*[None if a is None else a.ctypes.data for a in arrs], n, sums.ctypes.data):
        raise McomError("digest_reduce: bad arguments")
    return [int(v) for v in sums]


def ragged_index(len_bin: bytes, L: int):
    """The slots of the records of a len.bin in plain Python (what mcom_ragged_index computes on the device): (slots, n_even, n_odd,
    odd_bytes); a slot is the rank among the records of L bases, or bit 63 | the offset into the odd text."""
    slots, n_even, odd_bytes = [], 0, 0
    for b in len_bin:
        if b + 1 == L:
            slots.append(n_even); n_even += 1
        else:
            slots.append((1 << 63) | odd_bytes); odd_bytes += b + 1
    return slots, n_even, len(len_bin) - n_even, odd_bytes


def verify_ragged(folder: str, fastq: str, device: int = 0):
    """mcomh_verify_ragged_gpu: an archive made with -V against its FASTQ file, part by part.  Returns a dict part -> report for the parts
    that were compared: len, even_reads, even_quals, odd_seq, odd_qual."""
    reps = (VerifyReport * 5)(); present = (C.c_int32 * 5)()
    if load_host_library().mcomh_verify_ragged_gpu(os.fsencode(folder), os.fsencode(fastq), int(device), reps, present):
        raise McomError(f"{folder} could not be verified against {fastq}")
    out = {"identical": True}
    for k, tag in enumerate(("len", "even_reads", "even_quals", "odd_seq", "odd_qual")):
        if present[k]:
            r = reps[k]
            out[tag] = {"identical": bool(r.identical), "n_input": int(r.n_input), "n_archive": int(r.n_archive), "differing": int(r.differing),
                        "first_diff": None if r.first_diff == 2 ** 64 - 1 else int(r.first_diff)}
            out["identical"] = out["identical"] and out[tag]["identical"]
    return out


def decompress_fastq(folder: str, out_path: str, device: int | None = None) -> int:
    """mcomh_decompress_fastq(_gpu): the stream files of a -p -Q archive and its qual.mcq -> records `@<i+1>`, read, `+`, qualities.
    Returns the number of records.  device=None: the host route; an integer: reads and qualities rebuilt and the records laid out on
    that GPU (the same bytes; an error, never the host route, when there is no such GPU)."""
    n = C.c_uint64()
    lib = load_host_library()
    rc = lib.mcomh_decompress_fastq(os.fsencode(folder), os.fsencode(out_path), C.byref(n)) if device is None else \
        lib.mcomh_decompress_fastq_gpu(os.fsencode(folder), os.fsencode(out_path), C.byref(n), int(device))
    if rc:
        raise McomError(f"cannot decode {folder} to FASTQ" + ("" if device is None else f" on GPU {device}") + ": not a -p archive with qual.mcq, or a refused member")
    return int(n.value)


def read_order(order) -> np.ndarray:
    """A read order as a uint32 array: an array of row numbers as it is, or the bytes / the path of a read_order.bin (little-endian u32
    values); McomError for a file whose size is no multiple of 4."""
    if isinstance(order, (str, os.PathLike)):
        with open(order, "rb") as f:
            order = f.read()
    if isinstance(order, (bytes, bytearray, memoryview)):
        if len(order) % 4:
            raise McomError("read order: %d bytes are not a multiple of 4" % len(order))
        return np.frombuffer(bytes(order), dtype="<u4").astype(np.uint32)
    a = np.asarray(order)
    if a.ndim != 1 or a.dtype.kind not in "iu" or (a.size and (int(a.min()) < 0 or int(a.max()) >= 2 ** 32)):
        raise McomError("read order: a vector of row numbers below 2^32")
    return np.ascontiguousarray(a.astype(np.uint32))


def qual_gather(rows, order, device: int | None = None):
    """Quality rows put into a read order: row j of the result is rows[order[j]].  rows: uint8 matrix [n, L] (numpy);
    order: see read_order -- it must be a permutation of 0 .. n - 1, which the gather itself checks: McomError for another entry count, an
    entry >= n or a row named twice.  device=None: mcomh_qual_gather_rows on the host; an integer: mcom_qual_gather_rows on that GPU (an
    error, never the host twin, when there is none).  Returns a uint8 numpy matrix [n, L]."""
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.dtype != np.uint8 or (rows.shape[0] and rows.strides[1] != 1):
        raise McomError("qual_gather: a uint8 matrix with contiguous rows")
    o = read_order(order)
    n, L = int(rows.shape[0]), int(rows.shape[1])
    if int(o.shape[0]) != n:
        raise McomError("qual_gather: the order holds %d entries for %d rows" % (int(o.shape[0]), n))
    if device is None:
        pitch = int(rows.strides[0]) if n > 1 else L
        out = np.zeros((n, L), dtype=np.uint8)
        flag = C.c_uint32(0)
        if load_host_library().mcomh_qual_gather_rows(rows.ctypes.data if n else None, n, L, pitch, o.ctypes.data if n else None, n, out.ctypes.data if n else None, L, C.byref(flag)):
            raise McomError("qual_gather: rows of %d bytes at pitch %d" % (L, pitch))
        flags = int(flag.value)
    else:
        import torch
        from .hip import Context
        dev = f"cuda:{int(device)}"
        d_out, flags = Context(int(device)).qual_gather_rows(torch.from_numpy(np.ascontiguousarray(rows)).to(dev), torch.from_numpy(o.view(np.int32)).to(dev))
        out = d_out.cpu().numpy()
    if flags:
        raise McomError("qual_gather: the order is not a permutation of the rows:" + (" an entry beyond the last row" if flags & 1 else "") + (" a row named twice" if flags & 2 else ""))
    return out


def decompress_fastq_reordered(folder: str, out_path: str, device: int | None = None) -> int:
    """mcomh_decompress_fastq_reordered(_gpu): the stream files of a default-mode archive and its rqual.mcq (`minicom -q`) -> records
    `@<j+1>`, read, `+`, qualities in the archive's own order.  Returns the number of records; device as for decompress_fastq."""
    n = C.c_uint64()
    lib = load_host_library()
    rc = lib.mcomh_decompress_fastq_reordered(os.fsencode(folder), os.fsencode(out_path), C.byref(n)) if device is None else \
        lib.mcomh_decompress_fastq_reordered_gpu(os.fsencode(folder), os.fsencode(out_path), C.byref(n), int(device))
    if rc:
        raise McomError(f"cannot decode {folder} to FASTQ" + ("" if device is None else f" on GPU {device}") + ": not a default-mode archive with rqual.mcq, or a refused member")
    return int(n.value)


def decompress_fastq_pe(folder: str, out_path1: str, out_path2: str, device: int | None = None) -> int:
    """mcomh_decompress_fastq_pe(_gpu): the stream files of a paired-end archive with rqual_1.mcq and rqual_2.mcq (`minicom -1 -2 -q`) -> two
    FASTQ files, record j of one the mate of record j of the other, both named `@<j+1>`.  Returns the number of pairs."""
    n = C.c_uint64()
    lib = load_host_library()
    rc = lib.mcomh_decompress_fastq_pe(os.fsencode(folder), os.fsencode(out_path1), os.fsencode(out_path2), C.byref(n)) if device is None else \
        lib.mcomh_decompress_fastq_pe_gpu(os.fsencode(folder), os.fsencode(out_path1), os.fsencode(out_path2), C.byref(n), int(device))
    if rc:
        raise McomError(f"cannot decode {folder} to two FASTQ files" + ("" if device is None else f" on GPU {device}") + ": not a paired-end archive with rqual_1.mcq and rqual_2.mcq, or a refused member")
    return int(n.value)


def decompress_order_pe(folder: str, out_path1: str, out_path2: str, device: int | None = None, fastq: bool = False) -> int:
    """mcomh_decompress_order_pe(_gpu), with fastq=True mcomh_decompress_fastq_order_pe(_gpu): the stream files of a pair kept in input order
    (`minicom -1 -2 -p [-Q [-N]]`) -> the two files in input order: reads one per line, or four-line records (with
    name_1.mcn and name_2.mcn the two input files byte for byte).  Returns the number of pairs."""
    n = C.c_uint64()
    lib = load_host_library()
    name = "mcomh_decompress_fastq_order_pe" if fastq else "mcomh_decompress_order_pe"
    args = (os.fsencode(folder), os.fsencode(out_path1), os.fsencode(out_path2), C.byref(n))
    rc = getattr(lib, name)(*args) if device is None else getattr(lib, name + "_gpu")(*args, int(device))
    if rc:
        raise McomError(f"cannot decode {folder} to two files in input order" + ("" if device is None else f" on GPU {device}") + ": not a complete, consistent archive of a pair kept in input order")
    return int(n.value)


def verify_order_pe(folder: str, fastq1: str, fastq2: str, device: int = 0) -> dict:
    """mcomh_verify_order_pe_parts_gpu: a pair kept in input order against its two FASTQ files on GPU `device` -- the reads line against
    line over both files, and per file the quality lines and the names and `+` lines where the archive holds their members.  "identical" is
    true when every check made says so; "reads", "quality_1", "quality_2", "names_1", "names_2" are the checks made.  McomError when a
    check could not be made or the archive holds one member of two."""
    reps = (VerifyReport * 5)(); present = (C.c_int32 * 5)()
    if load_host_library().mcomh_verify_order_pe_parts_gpu(os.fsencode(folder), os.fsencode(fastq1), os.fsencode(fastq2), int(device), reps, present):
        raise McomError(f"cannot verify {folder} against {fastq1} and {fastq2} on GPU {device}")
    out = {"identical": True}
    for k, tag in enumerate(("reads", "quality_1", "quality_2", "names_1", "names_2")):
        if present[k]:
            r = reps[k]
            out[tag] = {"identical": bool(r.identical), "n_input": int(r.n_input), "n_archive": int(r.n_archive), "differing": int(r.differing),
                        "first_diff": None if r.first_diff == 2 ** 64 - 1 or not r.differing else int(r.first_diff)}
            out["identical"] = out["identical"] and out[tag]["identical"]
    return out


def verify_records(folder: str, fastq: str, fastq2: str | None = None, device: int = 0) -> dict:
    """mcomh_verify_records_gpu: does a `minicom -q` archive give back exactly the (read, quality) records of `fastq` -- with fastq2 the
    (read 1, read 2, quality 1, quality 2) pairs -- as a multiset, duplicates counted?  Decided on GPU `device`, nothing is written.
    McomError when no comparison could be made; a difference is a verdict, not an error."""
    r = VerifyReport()
    if load_host_library().mcomh_verify_records_gpu(os.fsencode(folder), 2 if fastq2 is not None else 0, os.fsencode(fastq), os.fsencode(fastq2) if fastq2 is not None else None,
                                                    int(device), C.byref(r)):
        raise McomError(f"cannot verify the records in {folder} against {fastq} on GPU {device}")
    t = r.times_ms
    return {"identical": bool(r.identical), "mode": ("default", "order", "paired")[r.mode], "n_input": int(r.n_input), "n_archive": int(r.n_archive),
            "missing": int(r.missing), "extra": int(r.extra), "exact_runs": int(r.exact_runs),
            "missing_examples": [int(v) for v in r.missing_ex[: r.n_missing_ex]], "extra_examples": [int(v) for v in r.extra_ex[: r.n_extra_ex]],
            "times_ms": {"ingest": t[0], "upload_index": t[1], "decode": t[2], "compare": t[3], "total": t[4]}}


def verify_quality(folder: str, fastq: str, device: int = 0) -> dict:
    """mcomh_verify_quality_gpu: does folder/qual.mcq give back exactly the quality lines of `fastq`, line against line?  Decided on GPU
    `device`, nothing is written.  McomError when no comparison could be made; a difference is a verdict, not an error."""
    r = VerifyReport()
    if load_host_library().mcomh_verify_quality_gpu(os.fsencode(folder), os.fsencode(fastq), int(device), C.byref(r)):
        raise McomError(f"cannot verify the qualities in {folder} against {fastq} on GPU {device}")
    return {"identical": bool(r.identical), "n_input": int(r.n_input), "n_archive": int(r.n_archive), "differing": int(r.differing),
            "first_diff": None if r.first_diff == 2 ** 64 - 1 else int(r.first_diff),
            "times_ms": {"ingest": r.times_ms[0], "decode": r.times_ms[2], "compare": r.times_ms[3], "total": r.times_ms[4]}}


QUAL_MODELS = ("stored", "order-0", "P", "PP", "PMP")     # the model ids of a `.mcq` member
QUAL_HINT_RANS = 0x180


def qual_hint(model) -> int:
    """MCOM_QUAL_HINT of include/mcom.h: None = choose, 0 .. 4 = that model id, "rans" = the embedded `.rans` member"""
    return 0 if model is None else QUAL_HINT_RANS if model == "rans" else 0x100 | int(model)


def qual_encode(rows, model=None) -> bytes:
    """mcomh_qual_encode, the host twin of the GPU coder: a uint8 matrix [n, L] (1 <= L <= 256; rows may be strided) -> a `.mcq`
    member.  model None: chosen by estimated size, and the embedded `.rans` member where that is smaller; 0 .. 4 or "rans" force one."""
    import numpy as np
    lib = load_host_library()
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.dtype != np.uint8 or (rows.shape[0] and rows.strides[1] != 1):
        raise McomError("qual_encode: a uint8 matrix with contiguous rows")
    n, L = int(rows.shape[0]), int(rows.shape[1])
    pitch = int(rows.strides[0]) if n > 1 else L
    cap = int(lib.mcomh_qual_bound(n, L))
    if not cap or pitch < L:
        raise McomError("qual_encode: rows of %d bytes" % L)
    out = C.create_string_buffer(cap)
    got = C.c_uint64()
    rc = lib.mcomh_qual_encode(rows.ctypes.data if n else None, n, L, pitch, out, cap, C.byref(got), qual_hint(model))
    if rc:
        raise McomError(f"qual_encode: error {rc}")
    return out.raw[:got.value]


def qual_info(member: bytes) -> tuple[int, int]:
    """mcomh_qual_info: (n_rows, L) a `.mcq` member's header states; McomError when the first 64 bytes are not such a header"""
    n, L = C.c_uint64(), C.c_uint32()
    head = bytes(member[:64])
    if load_host_library().mcomh_qual_info((C.c_char * len(head)).from_buffer_copy(head) if head else None, len(member), C.byref(n), C.byref(L)):
        raise McomError("qual_info: not a .mcq member")
    return int(n.value), int(L.value)


def qual_decode(member: bytes, pitch: int | None = None):
    """mcomh_qual_decode: a `.mcq` member -> the uint8 matrix [n, L] (a view of rows `pitch` apart when given); McomError for a member
    that is truncated, malformed or fails its CRC-32."""
    import numpy as np
    lib = load_host_library()
    member = bytes(member)
    n, L = qual_info(member)
    pitch = L if pitch is None else int(pitch)
    if pitch < L or n * pitch > 1 << 40:
        raise McomError("qual_decode: %d rows of %d bytes at pitch %d" % (n, L, pitch))
    buf = np.zeros(max(n * pitch, 1), dtype=np.uint8)
    gn, gL = C.c_uint64(), C.c_uint32()
    rc = lib.mcomh_qual_decode((C.c_char * len(member)).from_buffer_copy(member), len(member), buf.ctypes.data, pitch, n, C.byref(gn), C.byref(gL))
    if rc:
        raise McomError(f"qual_decode: error {rc}: not a complete, intact .mcq member")
    return buf[:n * pitch].reshape(n, pitch)[:, :L]


def qual_decode_rows(member: bytes, first: int, count: int, pitch: int | None = None, device: int | None = None):
    """Rows first .. first + count - 1 of a `.mcq` member (count clipped at the member's end) as a uint8 matrix [count, L] (DESIGN.md
    section 3.19): only the segments that hold them are decoded, and the member's CRC-32, which covers all rows, is NOT checked unless
    the range is the whole member.  device=None: mcomh_qual_decode_rows on the host; an integer: mcom_qual_decode_rows on that GPU (an
    error, never the host twin, when there is none).  McomError for a member whose header, tables, run lengths or touched segments are
    refused, and for first > n."""
    import numpy as np
    member = bytes(member)
    n, L = qual_info(member)
    first, count = int(first), int(count)
    if first < 0 or count < 0 or first > n:
        raise McomError("qual_decode_rows: rows %d .. + %d of %d" % (first, count, n))
    count = min(count, n - first)
    pitch = L if pitch is None else int(pitch)
    if pitch < L or count * pitch > 1 << 40:
        raise McomError("qual_decode_rows: %d rows of %d bytes at pitch %d" % (count, L, pitch))
    if device is not None:
        import torch
        from .hip import Context
        d_member = torch.from_numpy(np.frombuffer(member, dtype=np.uint8).copy()).to(f"cuda:{int(device)}")
        return Context(int(device)).qual_decode_rows(d_member, first, count, pitch=pitch).cpu().numpy()
    buf = np.zeros(max(count * pitch, 1), dtype=np.uint8)
    gn, gL = C.c_uint64(), C.c_uint32()
    rc = load_host_library().mcomh_qual_decode_rows((C.c_char * len(member)).from_buffer_copy(member), len(member), first, count, buf.ctypes.data, pitch, C.byref(gn), C.byref(gL))
    if rc:
        raise McomError(f"qual_decode_rows: error {rc}: a refused .mcq member")
    return buf[:count * pitch].reshape(count, pitch)[:, :L]


def qual_estimate(rows) -> list[int]:
    """mcomh_qual_estimate: the estimated coded size under every model id, in the order of QUAL_MODELS"""
    import numpy as np
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    est = (C.c_uint64 * 5)()
    if load_host_library().mcomh_qual_estimate(rows.ctypes.data if rows.size else None, rows.shape[0], rows.shape[1], rows.shape[1], est):
        raise McomError("qual_estimate: rows of %d bytes" % rows.shape[1])
    return [int(v) for v in est]


def name_text(names, plus=None) -> bytes:
    """The name text of records: per record its name (line 1 without '@'), a newline, the text of its third
    line (without '+'; plus=None: bare everywhere), a newline."""
    plus = [b""] * len(names) if plus is None else plus
    return b"".join(bytes(a) + b"\n" + bytes(b) + b"\n" for a, b in zip(names, plus))


def name_encode(text: bytes, n_records: int | None = None, device: int | None = None, mate: bytes | None = None) -> bytes:
    """A name text (name_text) -> a `.mcn` member.  device None: mcomh_name_encode, the host twin; an integer: mcom_name_encode on that
    GPU (the same bytes; an error, never the host twin, when there is none).  n_records None: half the number of lines.  McomError
    for a text that is not two complete lines per record; for a line above 255 bytes it names the record.
    mate: the name text of the mate file, record for record: mcom[h]_name_encode_mate -- the member is coded
    against it (kind 2) where that is strictly smaller, and is the member without a mate otherwise; McomError for a mate that is not two
    lines for each of the text's records."""
    text = bytes(text)
    n = text.count(b"\n") // 2 if n_records is None else int(n_records)
    if device is not None:
        import torch
        ctx = _device_context(device)
        dev = f"cuda:{int(device)}"
        up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else torch.empty(0, dtype=torch.uint8, device=dev)
        got = ctx.name_encode(up(text), n) if mate is None else ctx.name_encode_mate(up(text), n, up(bytes(mate)))
        return got.cpu().numpy().tobytes()
    lib = load_host_library()
    cap = int(lib.mcomh_name_bound(len(text)))
    out = C.create_string_buffer(cap)
    got, bad = C.c_uint64(), C.c_uint64()
    buf = (C.c_char * len(text)).from_buffer_copy(text) if text else None
    if mate is None:
        rc = lib.mcomh_name_encode(buf, len(text), n, out, cap, C.byref(got), C.byref(bad))
    else:
        mate = bytes(mate)
        rc = lib.mcomh_name_encode_mate(buf, len(text), n, (C.c_char * len(mate)).from_buffer_copy(mate) if mate else None, len(mate), out, cap, C.byref(got), C.byref(bad))
    if rc:
        if bad.value != 0xFFFFFFFFFFFFFFFF:
            raise McomError(f"name_encode: record {bad.value + 1} has a name or a '+' text above 255 bytes")
        raise McomError(f"name_encode: error {rc}: not the two lines of each of {n} records" + ("" if mate is None else ", in the text or in its mate"))
    return out.raw[:got.value]


def name_info(member: bytes, mate: bool = False) -> tuple[int, int]:
    """mcomh_name_info: (n_records, text_len) a `.mcn` member's header states; McomError when the first 96 bytes are not such a header.
    mate=True: mcomh_name_info_mate, for which a kind-2 header (section 3.12) is one too."""
    n, t = C.c_uint64(), C.c_uint64()
    head = bytes(member[:96])
    lib = load_host_library()
    if (lib.mcomh_name_info_mate if mate else lib.mcomh_name_info)((C.c_char * len(head)).from_buffer_copy(head) if head else None, len(member), C.byref(n), C.byref(t)):
        raise McomError("name_info: not a .mcn member")
    return int(n.value), int(t.value)


def name_decode(member: bytes, device: int | None = None, mate: bytes | None = None) -> bytes:
    """A `.mcn` member -> the name text, on the host twin or on that GPU; McomError for every member section 3.10 refuses.
    mate: the mate file's name text (mcom[h]_name_decode_mate): a kind-2 member is decoded against it and refused when it is not the
    text the member was coded against; kinds 0 and 1 decode as without it.  Without mate a kind-2 member is refused."""
    member = bytes(member)
    n, t = name_info(member, mate is not None)
    if device is not None:
        import torch
        ctx = _device_context(device)
        dev = f"cuda:{int(device)}"
        d_member = torch.frombuffer(bytearray(member), dtype=torch.uint8).to(dev)
        if mate is None:
            text, _ = ctx.name_decode(d_member)
        else:
            mate = bytes(mate)
            text = ctx.name_decode_mate(d_member, torch.frombuffer(bytearray(mate), dtype=torch.uint8).to(dev) if mate else torch.empty(0, dtype=torch.uint8, device=dev))
        return text.cpu().numpy().tobytes()
    out = C.create_string_buffer(max(t, 1))
    gt, gn = C.c_uint64(), C.c_uint64()
    buf = (C.c_char * len(member)).from_buffer_copy(member)
    if mate is None:
        rc = load_host_library().mcomh_name_decode(buf, len(member), out, t, C.byref(gt), C.byref(gn))
    else:
        mate = bytes(mate)
        rc = load_host_library().mcomh_name_decode_mate(buf, len(member), (C.c_char * len(mate)).from_buffer_copy(mate) if mate else None, len(mate), out, t, C.byref(gt), C.byref(gn))
    if rc:
        raise McomError(f"name_decode: error {rc}: not a complete, intact .mcn member" + ("" if mate is None else " of this mate"))
    return out.raw[:t]


def fastq_name_member(fastq: str, out_path: str, device: int | None = None, mate_path: str | None = None) -> int:
    """mcomh_fastq_name_member: the names and `+` texts of a four-line FASTQ file -> the `.mcn` member file out_path; returns the number
    of records.  device None: the host twin of the record rules and of the coder; an integer: that GPU (an error when there is none).
    McomError names the first record that has no `@` or `+` line or more than 255 bytes behind either; no file is left then.
    mate_path: `fastq` is the second file of a pair and mate_path the first (mcomh_fastq_name_member_mate): the member is coded against
    the first file's names where that is smaller; McomError when the two files differ in records."""
    n = C.c_uint64(); err = C.create_string_buffer(320)
    lib, dev = load_host_library(), -1 if device is None else int(device)
    if mate_path is None:
        rc = lib.mcomh_fastq_name_member(os.fsencode(fastq), dev, os.fsencode(out_path), C.byref(n), err, 320)
    else:
        rc = lib.mcomh_fastq_name_member_mate(os.fsencode(fastq), os.fsencode(mate_path), dev, os.fsencode(out_path), C.byref(n), err, 320)
    if rc:
        raise McomError(f"{fastq}: {err.value.decode() or 'cannot code the names'}")
    return int(n.value)


def fastq_names(path: str, device: int = 0, piece_bytes: int = 0) -> tuple[bytes, int]:
    """mcomh_fastq_names_to_device: (the name text of a four-line FASTQ file, the number of records), gathered on GPU `device` through
    pieces of piece_bytes (0 = 32 MiB) with the unfinished record of a piece carried in front of the next."""
    lib = load_host_library()
    d, nb, n = C.c_void_p(), C.c_uint64(), C.c_size_t()
    err = C.create_string_buffer(320)
    if lib.mcomh_fastq_names_to_device(os.fsencode(path), int(device), int(piece_bytes), C.byref(d), C.byref(nb), C.byref(n), err, 320):
        raise McomError(f"{path}: {err.value.decode() or 'cannot read the names'}")
    try:
        import torch
        out = torch.empty(max(int(nb.value), 1), dtype=torch.uint8, device=f"cuda:{int(device)}")
        if nb.value and lib.mcomh_device_copy(out.data_ptr(), d, int(nb.value)):
            raise McomError("fastq_names: copy failed")
        return out[:nb.value].cpu().numpy().tobytes(), int(n.value)
    finally:
        lib.mcomh_device_free(d)


def verify_names(folder: str, fastq: str, device: int = 0) -> dict:
    """mcomh_verify_names_gpu: does folder/name.mcn give back exactly the names and `+` texts of `fastq`, record against record?  Decided
    on GPU `device`, nothing is written.  McomError when no comparison could be made; a difference is a verdict, not an error."""
    r = VerifyReport()
    if load_host_library().mcomh_verify_names_gpu(os.fsencode(folder), os.fsencode(fastq), int(device), C.byref(r)):
        raise McomError(f"cannot verify the names in {folder} against {fastq} on GPU {device}")
    return {"identical": bool(r.identical), "n_input": int(r.n_input), "n_archive": int(r.n_archive), "differing": int(r.differing),
            "first_diff": None if r.first_diff == 2 ** 64 - 1 else int(r.first_diff)}


def name_file(in_path: str, out_path: str, pack: bool, device: int | None = None, mate_path: str | None = None) -> None:
    """mcomh_name_pack_file / _unpack_file: a file of name text -> a `.mcn` member file or back; device None: the host twin.
    mate_path: a file holding the mate's name text (mcomh_name_pack_file_mate / _unpack_file_mate)."""
    lib = load_host_library()
    dev = -1 if device is None else int(device)
    if mate_path is None:
        rc = (lib.mcomh_name_pack_file if pack else lib.mcomh_name_unpack_file)(os.fsencode(in_path), os.fsencode(out_path), dev)
    else:
        rc = (lib.mcomh_name_pack_file_mate if pack else lib.mcomh_name_unpack_file_mate)(os.fsencode(in_path), os.fsencode(mate_path), os.fsencode(out_path), dev)
    if rc:
        raise McomError(f"cannot {'pack' if pack else 'unpack'} {in_path}" + ("" if device is None else f" on GPU {device}"))


def rans_estimate(data: bytes) -> list[int]:
    """mcomh_rans_estimate: the estimated coded size of every candidate, in the order of RANS_MODELS."""
    est = (C.c_uint64 * 7)()
    n = len(data)
    load_host_library().mcomh_rans_estimate((C.c_char * n).from_buffer_copy(data) if n else None, n, est)
    return [int(v) for v in est]


def _device_context(device: int):
    from .hip import Context
    return Context(int(device))


def bwt_encode(data: bytes, device: int | None = None) -> bytes:
    """raw bytes -> a `.bwt` member.  device None: mcomh_bwt_encode, the host twin; an integer: mcom_bwt_encode
    on that GPU (the same bytes; an error, never the host twin, when there is none)."""
    if device is not None:
        import torch
        ctx = _device_context(device)
        raw = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(f"cuda:{int(device)}") if data else torch.empty(0, dtype=torch.uint8, device=f"cuda:{int(device)}")
        return ctx.bwt_encode(raw).cpu().numpy().tobytes()
    lib = load_host_library()
    n = len(data)
    cap = int(lib.mcomh_bwt_bound(n))
    out = C.create_string_buffer(cap)
    got = C.c_uint64()
    rc = lib.mcomh_bwt_encode((C.c_char * n).from_buffer_copy(data) if n else None, n, out, cap, C.byref(got))
    if rc:
        raise McomError(f"bwt_encode: error {rc}")
    return out.raw[:got.value]


def bwt_decode(member: bytes, device: int | None = None) -> bytes:
    """a `.bwt` member -> the raw bytes, on the host twin or on that GPU; McomError for every member section 3.8 refuses."""
    lib = load_host_library()
    n = len(member)
    src = (C.c_char * n).from_buffer_copy(member) if n else None
    raw_len = C.c_uint64()
    if lib.mcomh_bwt_raw_len(src, n, C.byref(raw_len)):
        raise McomError("bwt_decode: not a complete .bwt member")
    if device is not None:
        import torch
        ctx = _device_context(device)
        return ctx.bwt_decode(torch.frombuffer(bytearray(member), dtype=torch.uint8).to(f"cuda:{int(device)}")).cpu().numpy().tobytes()
    cap = int(raw_len.value)
    out = C.create_string_buffer(max(cap, 1))
    got = C.c_uint64()
    rc = lib.mcomh_bwt_decode(src, n, out, cap, C.byref(got))
    if rc:
        raise McomError(f"bwt_decode: error {rc}: not a complete, intact .bwt member")
    return out.raw[:got.value]


def bwt_stages(data: bytes):
    """mcomh_bwt_stages: (transformed bytes, index rows as a list, move-to-front ranks) of the host twin's encoder"""
    lib = load_host_library()
    n = len(data)
    n_anc = sum(-(-min(1 << 20, n - a) // 4096) for a in range(0, n, 1 << 20))
    tr, ix, rk = C.create_string_buffer(max(n, 1)), C.create_string_buffer(max(4 * n_anc, 1)), C.create_string_buffer(max(n, 1))
    if lib.mcomh_bwt_stages((C.c_char * n).from_buffer_copy(data) if n else None, n, tr, ix, rk):
        raise McomError("bwt_stages: error")
    return tr.raw[:n], [int.from_bytes(ix.raw[4 * k:4 * k + 4], "little") for k in range(n_anc)], rk.raw[:n]


def entropy_file(in_path: str, out_path: str, pack: bool, device: int | None = None, codec: str = "rans") -> dict:
    """mcomh_entropy_pack_file / _unpack_file (codec "bwt": mcomh_bwt_pack_file / _unpack_file): a file -> a member file or back.
    device None: the host twin; an integer: that GPU (an error, never the host twin, when there is none).  Returns mcomh_entropy_times
    as a dict."""
    lib = load_host_library()
    if codec not in ("rans", "bwt"):
        raise McomError("entropy_file: codec rans or bwt")
    if codec == "bwt":
        fn = lib.mcomh_bwt_pack_file if pack else lib.mcomh_bwt_unpack_file
    else:
        fn = lib.mcomh_entropy_pack_file if pack else lib.mcomh_entropy_unpack_file
    if fn(in_path.encode(), out_path.encode(), -1 if device is None else int(device)):
        raise McomError(("cannot pack %s" if pack else "%s is not a complete, intact ." + codec + " member") % in_path + ("" if device is None else f" (GPU {device})"))
    t = (C.c_double * 8)()
    lib.mcomh_entropy_times(t)
    return {"read_upload_ms": t[0], "codec_ms": t[1], "download_write_ms": t[2], "total_ms": t[3], "raw_bytes": int(t[4]), "coded_bytes": int(t[5])}


def pool_trim():
    """mcomh_pool_trim: pooled device blocks of closed pipelines go back to the runtime."""
    load_host_library().mcomh_pool_trim()


def decompress_pe(folder: str, out_path1: str, out_path2: str, device: int | None = None) -> int:
    """mcomh_decompress_pe: the paired-end file set -> two files, line i of both is a pair.  Returns the number of pairs.
    device: as for decompress()."""
    n = C.c_uint64()
    if device is None:
        rc = load_host_library().mcomh_decompress_pe(folder.encode(), out_path1.encode(), out_path2.encode(), C.byref(n))
    else:
        rc = load_host_library().mcomh_decompress_pe_gpu(folder.encode(), out_path1.encode(), out_path2.encode(), C.byref(n), int(device))
    if rc:
        raise McomError(f"cannot decode the paired-end stream files in {folder}" + ("" if device is None else f" on GPU {device}"))
    return int(n.value)


def read_fastq(path: str, L: int = 0) -> np.ndarray:
    """mcomh_fastq_read: the reads of a FASTQ/FASTA file (plain or .gz) as a numpy uint8 [n, L] array.  Host only."""
    lib = load_host_library()
    Lc, n = C.c_int(L), C.c_size_t()
    rc = lib.mcomh_fastq_read(path.encode(), C.byref(Lc), None, C.c_size_t(-1).value, C.byref(n))      # count + check
    if rc:
        raise McomError(f"{path}: not a FASTQ/FASTA file of equal-length reads ({rc})")
    out = np.empty((n.value, Lc.value), dtype=np.uint8)
    rc = lib.mcomh_fastq_read(path.encode(), C.byref(Lc), out.ctypes.data_as(C.c_void_p), n.value, C.byref(n))
    if rc:
        raise McomError(f"{path}: read failed ({rc})")
    return out


class Pipeline:
    """Stage 1 + Stage 2 of minicom on one GPU.  reads: numpy uint8 [n, L] (host) or a torch uint8 CUDA tensor [n, pitch]."""

    def __init__(self, reads, L: int | None = None, device: int = 0, stream=None, packed: bool = False, records=None, **params):
        """records (packed=True only): (x int64 [n], ylow int32 [n]) CUDA tensors, the minimizers the rows were sketched to with
        this pipeline's k on the rank that sent them: kt_for_reads then assembles the records instead of sketching again."""
        self.lib = load_host_library()
        p = Params(**{k: int(v) for k, v in params.items()})
        h = C.c_void_p()
        s = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(0)
        if packed:
            # int64 CUDA tensor [n, W] of packed rows (include/mcom.h format)
            assert reads.is_cuda and reads.is_contiguous() and L is not None and reads.shape[1] == (2 * L + 63) // 64
            n = int(reads.shape[0])
            self._keep = reads
            rc = self.lib.mcomh_create_packed(C.byref(h), device, s, C.c_void_p(reads.data_ptr()), n, L, C.byref(p))
        elif isinstance(reads, np.ndarray):
            reads = np.ascontiguousarray(reads, dtype=np.uint8)
            n, L = reads.shape
            self._keep = reads
            rc = self.lib.mcomh_create(C.byref(h), device, s, reads.ctypes.data_as(C.c_void_p), None, L, n, L, C.byref(p))
        else:
            assert reads.is_cuda and reads.is_contiguous() and L is not None
            n, pitch = reads.shape
            self._keep = reads
            rc = self.lib.mcomh_create(C.byref(h), device, s, None, C.c_void_p(reads.data_ptr()), pitch, n, L, C.byref(p))
        if rc:
            raise McomError(f"mcomh_create failed ({rc}): no usable GPU or bad arguments; there is no CPU fallback")
        self._h = h
        self.n, self.L = n, L
        if records is not None:
            assert packed, "records travel with packed rows"
            x, ylow = records
            import torch
            assert x.is_cuda and ylow.is_cuda and x.is_contiguous() and ylow.is_contiguous() and x.dtype == torch.int64 and ylow.dtype == torch.int32
            assert int(x.shape[0]) == n and int(ylow.shape[0]) == n
            self._keep = (self._keep, x, ylow)
            self._check(self.lib.mcomh_set_records(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(ylow.data_ptr())))

    @classmethod
    def from_host_streamed(cls, reads, device: int = 0, **params):
        """mcomh_create_streamed: reads = torch uint8 CPU tensor (ideally pinned) or numpy array [n, L], NOT copied on the
        host; kt_for_reads uploads it chunk by chunk beside the classification kernels.  Keep `reads` alive."""
        lib = load_host_library()
        n, L = int(reads.shape[0]), int(reads.shape[1])
        ptr = reads.ctypes.data if isinstance(reads, np.ndarray) else reads.data_ptr()
        self = cls.__new__(cls)
        self.lib = lib
        p = Params(**{k: int(v) for k, v in params.items()})
        h = C.c_void_p()
        rc = lib.mcomh_create_streamed(C.byref(h), device, C.c_void_p(0), C.c_void_p(ptr), n, L, C.byref(p))
        if rc:
            raise McomError(f"mcomh_create_streamed failed ({rc})")
        self._h, self._keep = h, reads
        self.n, self.L = n, L
        return self

    @classmethod
    def from_fastq(cls, path: str, L: int = 0, device: int = 0, chunk_reads: int = 0, path2: str | None = None, **params):
        """FASTQ/FASTA (plain or .gz) -> HBM through two pinned chunks (mcomh_fastq_to_device) -> pipeline.
        path2: the mates' file (paired end): its reads follow those of the first file."""
        lib = load_host_library()
        err = C.create_string_buffer(256)
        self = cls.__new__(cls)
        self.lib = lib
        p = Params(**{k: int(v) for k, v in params.items()})
        h = C.c_void_p()
        rc = lib.mcomh_create_from_fastq(C.byref(h), device, C.c_void_p(0), path.encode(), path2.encode() if path2 else None, C.byref(p), err, 256)
        if rc:
            raise McomError(f"{path}: {err.value.decode() or rc}")
        self._h, self._dev_reads, self._keep = h, None, None
        self.n, self.L = int(lib.mcomh_stat(h, b"n")), int(lib.mcomh_stat(h, b"L"))
        if L and L != self.L:
            self.close()
            raise McomError(f"{path}: reads of {self.L} bases, {L} expected")
        return self

    @classmethod
    def from_fastq_ragged(cls, path: str, L: int, len_path: str, odd_seq_path: str, device: int = 0, piece_bytes: int = 0, **params):
        """A FASTQ file whose reads differ in length -> pipeline over its reads of L bases: the text is parsed on
        the card by the lengths in len_path (fastq_lengths wrote it and returned L), the reads of L bases go to HBM in input order
        (mcomh_fastq_to_device_ragged), the bases of the others to odd_seq_path."""
        lib = load_host_library()
        err = C.create_string_buffer(320)
        d, n = C.c_void_p(), C.c_size_t()
        if lib.mcomh_fastq_to_device_ragged(os.fsencode(path), int(device), int(L), os.fsencode(len_path), int(piece_bytes), C.byref(d), C.byref(n), os.fsencode(odd_seq_path), err, 320):
            raise McomError(f"{path}: {err.value.decode() or 'cannot read the file'}")
        self = cls.__new__(cls)
        self.lib = lib
        p = Params(**{k: int(v) for k, v in params.items()})
        h = C.c_void_p()
        if lib.mcomh_create(C.byref(h), device, C.c_void_p(0), None, d, int(L), n.value, int(L), C.byref(p)):
            lib.mcomh_device_free(d)
            raise McomError("mcomh_create failed: no usable GPU or bad arguments; there is no CPU fallback")
        self._h, self._dev_reads, self._keep = h, d, None
        self.n, self.L = int(n.value), int(L)
        return self

    def _check(self, rc):
        if rc:
            raise McomError(f"mcom host error {rc}: {self.lib.mcomh_last_error(self._h).decode()}")

    def close(self):
        if getattr(self, "_h", None):
            self.lib.mcomh_destroy(self._h)
            self._h = None
        if getattr(self, "_dev_reads", None):
            self.lib.mcomh_device_free(self._dev_reads)
            self._dev_reads = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def kt_for_reads(self): self._check(self.lib.mcomh_kt_for_reads(self._h))
    def kt_for_bucket(self): self._check(self.lib.mcomh_kt_for_bucket(self._h))
    def combine_cluster(self): self._check(self.lib.mcomh_combine_cluster(self._h))
    def update_single(self): self._check(self.lib.mcomh_update_single(self._h))
    def pre_process(self): self._check(self.lib.mcomh_pre_process(self._h))
    def stage2(self): self._check(self.lib.mcomh_stage2(self._h))

    def realign_hash(self, thr: int) -> int:
        cr = C.c_long()
        self._check(self.lib.mcomh_realign_hash(self._h, thr, C.byref(cr)))
        return cr.value

    def dump_stages(self, path: str): self._check(self.lib.mcomh_dump_stages(self._h, path.encode()))

    def keep_read_order(self, on: bool = True):
        """mcomh_keep_read_order: while on, cluster_dump (default or paired) also writes folder/read_order.bin."""
        self._check(self.lib.mcomh_keep_read_order(self._h, 1 if on else 0))

    def cluster_dump(self, folder: str, order: bool = False, paired: bool = False):
        """Writes the reference's pre-bsc stream files (cluster_dump at one thread) into an existing directory;
        order=True: the order-preserving file set of minicom -p; paired=True: the paired-end file set (rows [0, n/2) are
        the first file, rows [n/2, n) their mates)."""
        fn = self.lib.mcomh_cluster_dump_pe if paired else self.lib.mcomh_cluster_dump_order if order else self.lib.mcomh_cluster_dump
        self._check(fn(self._h, folder.encode()))

    def cluster_dump_order_pe(self, folder: str):
        """mcomh_cluster_dump_order_pe: a pipeline made of two files, dumped in input order -- the order-preserving file set of the 2 n rows
        and pe_order.txt."""
        self._check(self.lib.mcomh_cluster_dump_order_pe(self._h, folder.encode()))

    def prof_enable(self, on: bool = True): self._check(self.lib.mcomh_prof_enable(self._h, 1 if on else 0))

    def prof_read(self, name: str):
        """(device milliseconds, launches) of one kernel class, measured with HIP events on the launch stream."""
        ms = C.c_double(); n = C.c_uint64()
        self._check(self.lib.mcomh_prof_read(self._h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def prof_kernels(self, name: str = "*") -> dict:
        """{kernel name: launches} of one kernel class ("*": every kernel of the library) while the profiler was on -- the
        compiler's spelling of each instantiation, which is the name rocprofv3 prints"""
        need = C.c_size_t()
        self._check(self.lib.mcomh_prof_kernels(self._h, name.encode(), None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value + 1)
        self._check(self.lib.mcomh_prof_kernels(self._h, name.encode(), buf, need.value + 1, None))
        out = {}
        for ln in buf.value.decode().splitlines():
            k, _, c = ln.rpartition("\t")
            out[k] = int(c)
        return out

    def stat(self, name: str) -> float:
        return float(self.lib.mcomh_stat(self._h, name.encode()))

    def id_list(self, name: str) -> np.ndarray:
        n = C.c_size_t()
        ptr = self.lib.mcomh_list(self._h, name.encode(), C.byref(n))
        if not n.value:
            return np.zeros(0, dtype=np.uint32)
        return np.frombuffer((C.c_char * (4 * n.value)).from_address(ptr), dtype=np.uint32).copy()

    def contig_set(self):
        """(ref uint8 [chars], ref_off uint64 [n + 1], mem uint64 [members], mem_off uint64 [n + 1]): the whole contig set as
        flat numpy arrays (copies), mcomh_contig_set."""
        n = C.c_size_t(); ref, ro, mem, mo = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self.lib.mcomh_contig_set(self._h, C.byref(n), C.byref(ref), C.byref(ro), C.byref(mem), C.byref(mo)))
        nc = n.value

        def arr(ptr, dtype, count):
            if not count:
                return np.zeros(0, dtype=dtype)
            return np.frombuffer((C.c_char * (np.dtype(dtype).itemsize * count)).from_address(ptr.value), dtype=dtype).copy()
        roff = arr(ro, np.uint64, nc + 1) if nc else np.zeros(1, np.uint64)
        moff = arr(mo, np.uint64, nc + 1) if nc else np.zeros(1, np.uint64)
        return arr(ref, np.uint8, int(roff[-1])), roff, arr(mem, np.uint64, int(moff[-1])), moff

    def result_digest(self):
        """mcomh_result_digest: eight numbers that two runs over the same reads must share."""
        out = (C.c_uint64 * 8)()
        self._check(self.lib.mcomh_result_digest(self._h, out))
        return [int(v) for v in out]

    def contigs(self):
        out = []
        for i in range(self.lib.mcomh_n_contigs(self._h)):
            n = self.lib.mcomh_contig_n(self._h, i)
            mem = np.frombuffer((C.c_char * (8 * n)).from_address(self.lib.mcomh_contig_members(self._h, i)), dtype=np.uint64).copy() if n else np.zeros(0, np.uint64)
            ln = C.c_size_t()
            ptr = self.lib.mcomh_contig_ref(self._h, i, C.byref(ln))
            out.append((C.string_at(ptr, ln.value), mem))
        return out


# ---- the odd reads of a -V archive against the contigs (`minicom -p -V -A`, host/mcom_odd_align.cpp) ----
def odd_align_folder(folder: str, device: int | None = None):
    """mcomh_odd_align_folder over the UNGROUPED stream files of `folder` (ref.bin.*, beg_pos.bin.*, info.txt, len.bin, odd.seq): odd.aln is
    written and odd.seq rewritten to the reads that were not found in the contigs.  device=None: the plain C++ twins; an integer: the
    kernels of csrc/odd_align.hip on that GPU -- the same bytes.  Returns (n_odd, n_aligned, residual_bytes); nothing is written when no
    read is aligned."""
    n, a, r = C.c_uint64(), C.c_uint64(), C.c_uint64()
    err = C.create_string_buffer(256)
    if load_host_library().mcomh_odd_align_folder(os.fsencode(folder), -1 if device is None else int(device), C.byref(n), C.byref(a), C.byref(r), err, 256):
        raise McomError(f"{folder}: odd reads not aligned: {err.value.decode(errors='replace')}")
    return int(n.value), int(a.value), int(r.value)


def _np_ptr(a):
    return C.c_void_p(a.ctypes.data) if a.size else C.c_void_p(0)


def odd_text_host(refs):
    """mcomh_odd_text_append over refs, a list of (ref.bin image as bytes, bases taken): (T as uint64 words, the last one zero; |T|)."""
    L = load_host_library()
    total = sum(int(b) for _, b in refs)
    t = np.zeros((total + 31) // 32 + 1, dtype=np.uint64)
    at = 0
    for img, bases in refs:
        a = np.frombuffer(bytes(img), dtype=np.uint8)
        L.mcomh_odd_text_append(_np_ptr(t), at, _np_ptr(a), a.size, int(bases))
        at += int(bases)
    return t, total


def odd_align_host(t, t_bases: int, odd: bytes, off):
    """mcomh_odd_index_build + mcomh_odd_align: the hit words (uint64 [n_odd]) of the records odd[off[j]:off[j + 1]]."""
    L = load_host_library()
    off = np.ascontiguousarray(off, dtype=np.uint64)
    text = np.frombuffer(bytes(odd), dtype=np.uint8)
    hits = np.zeros(max(off.size - 1, 1), dtype=np.uint64)
    idx = C.c_void_p()
    if L.mcomh_odd_index_build(_np_ptr(t), int(t_bases), C.byref(idx)):
        raise McomError("odd_align: no seed index (a text of 2^40 bases or more?)")
    try:
        if L.mcomh_odd_align(idx, _np_ptr(t), int(t_bases), _np_ptr(text), _np_ptr(off), off.size - 1, _np_ptr(hits)):
            raise McomError("odd_align: record offsets that do not ascend by 0 .. 256")
    finally:
        L.mcomh_odd_index_free(idx)
    return hits[:off.size - 1]


def odd_align_encode_host(hits, t, t_bases: int, odd: bytes, off):
    """mcomh_odd_align_encode: (member bytes -- empty when no record is aligned --, residual bytes), in buffers of exact size."""
    L = load_host_library()
    off = np.ascontiguousarray(off, dtype=np.uint64); hits = np.ascontiguousarray(hits, dtype=np.uint64)
    text = np.frombuffer(bytes(odd), dtype=np.uint8)
    ml, rl = C.c_uint64(), C.c_uint64()
    args = (_np_ptr(hits), _np_ptr(text), _np_ptr(off), off.size - 1, _np_ptr(t), int(t_bases))
    if L.mcomh_odd_align_encode(*args, None, 0, C.byref(ml), None, 0, C.byref(rl)):
        raise McomError("odd_align_encode: a hit word that its read and the text do not bear out, or a text outside ACGTN")
    mem = np.zeros(int(ml.value), dtype=np.uint8); res = np.zeros(int(rl.value), dtype=np.uint8)
    if L.mcomh_odd_align_encode(*args, _np_ptr(mem), mem.size, C.byref(ml), _np_ptr(res), res.size, C.byref(rl)):
        raise McomError("odd_align_encode failed")
    return mem.tobytes(), res.tobytes()


def odd_align_decode_host(member: bytes, t, t_bases: int, residual: bytes, off):
    """mcomh_odd_align_decode of an untrusted member: (the full odd text or None, flags, the refusal's words or None)."""
    L = load_host_library()
    off = np.ascontiguousarray(off, dtype=np.uint64)
    mem = np.frombuffer(bytes(member), dtype=np.uint8); res = np.frombuffer(bytes(residual), dtype=np.uint8)
    out = np.zeros(int(off[-1]), dtype=np.uint8)
    flags = C.c_uint32()
    if L.mcomh_odd_align_decode(_np_ptr(mem), mem.size, _np_ptr(t), int(t_bases), _np_ptr(res), res.size, _np_ptr(off), off.size - 1, _np_ptr(out), C.byref(flags)):
        if not flags.value:                                  # the caller's own arguments, not the member
            raise McomError("odd_align_decode: a null pointer, or record offsets that do not ascend by 0 .. 256")
        return None, int(flags.value), L.mcomh_odd_align_refusal(flags.value).decode()
    return out.tobytes(), 0, None
