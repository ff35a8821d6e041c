// minicom_amd/csrc/digest_model.hpp -- the digest of a FASTQ file that `minicom -K` stores and `minicom -d` checks (DESIGN.md section
// 3.18), for host and device: the kernels of csrc/digest.hip and their plain C++ twin (host/mcom_digest.cpp) compute over these
// functions and nothing else, so they agree bit for bit.
//
// A LINE is the bytes b[0 .. m) of a FASTQ line without its newline and without the leading '@' / '+' of lines 1 and 3, m = 0 .. 256.
// All arithmetic is mod 2^64, and everything is computed once per seed K, so every value is a pair of words.
//   word w_j      the little-endian u64 of bytes [8j, 8j + 8), zero-padded, j = 0 .. ceil(m / 8) - 1
//   H(line)     = mix((sum_j mix(w_j ^ mix(K + j))) + m)
//   C(x, y)     = mix(x + mix(y + K))
//   hS = H(sequence), hQ = H(qualities), hN = C(H(name), H(plus text))
//   ordered     = sum_i mix(h_i + (i + 1) K)           multiset = sum_i mix(r_i)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MCOM_DG_HD __host__ __device__ inline
#else
#define MCOM_DG_HD inline
#endif

namespace mcom_digest_model {

enum { LINE_BYTES = 256, NAME_BYTES = 255 };
// the sixteen words of a digest: word 2 * key + seed
enum { SEQ_ORDERED_1 = 0, QUAL_ORDERED_1 = 1, NAME_ORDERED_1 = 2, SEQ_ORDERED_2 = 3, QUAL_ORDERED_2 = 4, NAME_ORDERED_2 = 5, SEQ_MULTISET = 6, REC_MULTISET = 7, N_KEYS = 8, N_SUMS = 16 };

MCOM_DG_HD uint64_t seed(int s) { return s ? 0xC2B2AE3D27D4EB4Full : 0x9E3779B97F4A7C15ull; }
MCOM_DG_HD uint64_t mix(uint64_t x)
{
	x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
	x ^= x >> 27; x *= 0x94D049BB133111EBull;
	x ^= x >> 31;
	return x;
}
// what word j of a line adds to the line's sum
MCOM_DG_HD uint64_t word_term(uint64_t w, uint64_t j, uint64_t K) { return mix(w ^ mix(K + j)); }
// H from the sum of the terms of a line of m bytes
MCOM_DG_HD uint64_t line_hash(uint64_t sum, uint64_t m) { return mix(sum + m); }
MCOM_DG_HD uint64_t combine(uint64_t x, uint64_t y, uint64_t K) { return mix(x + mix(y + K)); }
// the terms of the two reductions for record i (from 0)
MCOM_DG_HD uint64_t ordered_term(uint64_t h, uint64_t i, uint64_t K) { return mix(h + (i + 1) * K); }
MCOM_DG_HD uint64_t multiset_term(uint64_t r) { return mix(r); }

}  // namespace mcom_digest_model
