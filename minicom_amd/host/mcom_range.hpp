// minicom_amd/host/mcom_range.hpp -- the two routes the range decoders (`minicom -d -R`) choose between.
// Internal to libmcom_host.
#pragma once
#include <cstdint>

// records [first, first + count) of a -p archive on GPU `device` (mcom_decompress_gpu.cpp): one read per line or -- fastq -- four-line
// records; pair: the same range of both files of a pair kept in input order.  The folder has passed the refusals that need no decoding
// (mcom_decompress.cpp); first > n is refused here, where n is known.  -1 and no output file when the range is refused.
int mcom_range_gpu(const char *folder, const char *out_path1, const char *out_path2, uint64_t first, uint64_t count, uint64_t *n_written, int device, bool pair, bool fastq);
