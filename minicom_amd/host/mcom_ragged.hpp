// minicom_amd/host/mcom_ragged.hpp -- what the decoders share of the ragged archive (host/mcom_ragged.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
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
// false with `why` set: the parts disagree
bool mcom_ragged_load(const char *folder, int L, uint64_t n_even, bool want_qual, McomRaggedParts &P, std::string &why);
