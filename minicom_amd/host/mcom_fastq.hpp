// minicom_amd/host/mcom_fastq.hpp -- the single-pass FASTQ parser, shared between mcom_fastq.cpp and the pipeline driver.
#pragma once
#include <stddef.h>
#include <stdint.h>
// ---- the single-pass route (round 4): pread in chunks, check, pack and send in one sweep; rows go to provisional places ----
struct McomFastqStream;
// rows a plain four-line FASTQ file can hold at most (room for the provisional places), *L = its read length (in: 0 or the length it
// must have); 0 = not that layout
size_t mcom_fastq_stream_cap(const char *path, int *L);
// 1 = done: d_packed / d_nmask (room for cap_rows rows each) hold every read at its piece's provisional place; 0 = not this layout after
// all; < 0 = error
int mcom_fastq_stream_packed(const char *path, int L, int device, void *copy_stream, uint64_t *d_packed, uint64_t *d_nmask, size_t cap_rows, McomFastqStream **out);
size_t mcom_fastq_stream_total(const McomFastqStream *st);
int mcom_fastq_stream_len(const McomFastqStream *st);
// the pieces: provisional first row and number of rows of each (arrays of the returned size; NULL: just the size)
size_t mcom_fastq_stream_pieces(const McomFastqStream *st, size_t *prov, size_t *count);
void mcom_fastq_stream_free(McomFastqStream *st);
// mcom_qual_gpu.cpp: FOLDER/qual_lossy.txt, when there, applied to the n x L quality rows at d_rows on GPU `device` by
// mcom_qual_transform -- what a verifier does to the FASTQ file's rows before it compares.  0 = no marker, or applied; -1 = a marker that
// is not a spec, or a device error (the message is printed)
int mcom_qual_lossy_apply_marker(const char *folder, int device, uint8_t *d_rows, size_t n, int L);
// the same for FOLDER/qual_agree.txt (`minicom -a`): the agreement mask rebuilt from the folder's stream files on the
// device, its rows [first_mask_row, first_mask_row + n) laid over the rows by mcom_qual_agree.  Before the call above: agreement first.
int mcom_qual_agree_apply_marker(const char *folder, int device, uint8_t *d_rows, size_t n, int L, uint64_t first_mask_row);
