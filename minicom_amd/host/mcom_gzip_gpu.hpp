// minicom_amd/host/mcom_gzip_gpu.hpp -- the piece loop that the FASTQ passes over a BGZF file share (host/mcom_gzip_gpu.cpp, DESIGN.md
// section 3.15): whole members go up compressed, are inflated on the card behind the unfinished record of the piece before, and the
// whole records of each piece are handed to the pass with their line index.
#pragma once
#include "../../include/mcom.h"
#include <functional>
#include <stddef.h>
#include <stdint.h>

// One piece on the card: d_text[0 .. bytes) holds `records` whole four-line records, d_line_start the 4 * records + 1 line starts of
// mcom_decode_line_index.  false: the pass gives the file up (a record it flags, no room).
typedef std::function<bool(const uint8_t *d_text, uint64_t bytes, uint64_t records, const uint64_t *d_line_start)> mcom_gz_piece_fn;

// true: the file at `path` was BGZF to its end and every record of it went through `piece` on the context's GPU.  false: the caller
// starts the file again from its beginning through zlib, and nothing `piece` did so far counts -- the file's first member carries no `BC`
// field, a later one does not, the walk leaves the file, the device refuses a member, the file ends inside a record, a piece holds no
// whole record, or `piece` said so.  The zlib route then words whatever is wrong with the file.
// piece_bytes: the text of the members of one piece (one member at least, however small).
bool mcom_gz_device_route(const char *path, mcom_ctx *ctx, size_t piece_bytes, const mcom_gz_piece_fn &piece);

// members inflated on the device by the last call (0: it returned false); what mcomh_test_gz_device_members reports
void mcom_gz_note_device_members(long n);
