// minicom_amd/host/mcom_ragged.hpp -- what the decoders share of the ragged archive (host/mcom_ragged.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <functional>
#include <string>
#include <vector>

// The side members of a ragged archive, read from `folder` and checked against one another and against the core's n_even reads of L:
// the bytes of len.bin equal to L - 1 number n_even, the other lengths sum to the size of odd.seq (and of odd.qual, which is there
// exactly when want_qual says qual.mcq is).  slot: as mcom_ragged_index makes them.
struct McomRaggedParts {
	std::vector<uint8_t> len, odd_seq, odd_qual;
	std::vector<uint64_t> slot;
	uint64_t n = 0, n_even = 0;
};
// Line `which` (1 sequence, 3 quality) of every record of a FASTQ file, split on GPU `device` by the lengths in len_path: the even rows in
// HBM as [n_even][L] (*d_rows, release with mcomh_device_free), the odd text on the host.  What mcomh_fastq_to_device_ragged and the
// verifier run.  -1 with a message in err.
int mcom_ragged_split_to_device(const char *path, int device, int which, int L, const char *len_path, uint8_t **d_rows, std::vector<uint8_t> &odd, uint64_t *n_even, char *err,
                                size_t err_cap);
// is it a ragged archive at all (does folder/len.bin exist)?
bool mcom_ragged_present(const char *folder);
// false with `why` set: the parts disagree.  rebuild_odd false (the GPU decoder, for a folder with odd.aln): P.odd_seq is the residual as the folder
// holds it -- empty when odd.seq is missing -- and its size is not set against the lengths: the caller rebuilds the text and does that
bool mcom_ragged_load(const char *folder, int L, uint64_t n_even, bool want_qual, McomRaggedParts &P, std::string &why, bool rebuild_odd = true);
// `minicom -V -A` (host/mcom_odd_align.cpp): does folder/odd.aln exist?  ... and the full odd text into P.odd_seq
// from odd.aln, the contigs of the folder's ref.bin.* and the residual odd.seq (P.len is loaded); false with `why` set: refused
bool mcom_odd_align_present(const char *folder);
bool mcom_odd_align_rebuild(const char *folder, int L, McomRaggedParts &P, std::string &why);

#ifndef MCOM_ENTROPY_HOST_ONLY
#include "../../include/mcom.h"
// The piece loop of the FASTQ passes (plain or gzip text through zlib's reader, the unfinished record of a piece carried in front of the
// next one; a BGZF file of four-line records inflated on the card) for a pass that lives elsewhere: every record
// of the file at `path` goes through `pass` on the caller's context, `records` whole records of lines_per_record (4 or 1) lines from
// record `first` of the file with their text and line index; d_flag: the four flag words, cleared in front of the line index (words 0
// and 1: the pass's own, word 2: the index's).  pass returns 0 to go on; again(): the pass forgets what it has seen, the file starts again
// from its beginning.  *n = the records of the file.  -1 with a message in err (the pass words its own).
typedef std::function<int(const uint8_t *d_text, uint64_t bytes, uint64_t records, const uint64_t *d_line_start, uint64_t first, uint32_t *d_flag)> McomPiecePass;
int mcom_fastq_for_each_piece(const char *path, mcom_ctx *ctx, int device, int lines_per_record, size_t piece_bytes, const McomPiecePass &pass, const std::function<bool()> &again,
                              uint64_t *n, char *err, size_t err_cap);
#endif
