// minicom_amd/csrc/odd_align_model.hpp -- the odd reads of a -V archive coded against the contigs (`minicom -p -V -A`):
// the one statement of the rule and of the member odd.aln, shared by the kernels (csrc/odd_align.hip) and their plain C++ twins
// (host/mcom_odd_align.cpp).
//
// T, the reference text, is the bases of ref.bin.0, ref.bin.1, ... back to back, of every set as many as its contigs hold; it is kept as
// ref.bin keeps it, 2 bits per base (A C G T = 0 1 2 3), base i in bits 2 (i & 31) of little-endian 64-bit word i >> 5, with one word of
// zeros behind the last one.  The grid holds every q with q % G == 0 and q + K <= |T| under the key oa_key(T, q): the K bases from q,
// base j in bits 2 j.  A read of l >= K + G - 1 bases is laid on T in both orientations; every offset o whose K-mer holds no N and has
// at most M grid places q gives the candidates p = q - o with 0 <= p and p + l <= |T|; d(s, p) counts the places where the oriented read
// and T[p, p + l) differ (an N differs always).  The hit is the smallest d << 48 | s << 40 | p among the candidates with d <= E(l).
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define OA_HD __host__ __device__ inline
#else
#define OA_HD inline
#endif

enum { OA_K = 24, OA_G = 8, OA_M = 16, OA_MIN_LEN = OA_K + OA_G - 1, OA_MAX_LEN = 256, OA_HEADER = 64 };
#define OA_KEY_MASK 0xFFFFFFFFFFFFull
#define OA_MAX_T (1ull << 40)                                // |T| below this: p has 40 bits of the hit word
#define OA_NONE 0xFFFFFFFFFFFFFFFFull                        // the hit word of a read that is not aligned
#define OA_MAGIC "MCOMOAL1"

// why a member is refused, one bit per reason; oa_refusal() words the lowest one
enum {
	OA_F_HEADER = 1,      // too short for a header, another magic, constants other than 24 / 8 / 16
	OA_F_COUNT = 2,       // counts that disagree with the header, with len.bin or with the residual's size
	OA_F_SHORT = 4,       // an aligned read shorter than 31 bases
	OA_F_WINDOW = 8,      // p + l > |T|
	OA_F_BUDGET = 16,     // d above E(l)
	OA_F_OFFSET = 32,     // a mismatch offset outside the read
	OA_F_BASE = 64,       // a mismatch base outside ACGTN
	OA_F_SAME = 128,      // a mismatch that equals the window's base
	OA_F_CRC = 256        // the rebuilt text has another CRC-32 than the header states
};
inline const char *oa_refusal(uint32_t flags)
{
	if (flags & OA_F_HEADER) return "odd.aln: no header of this version (magic, K = 24, G = 8, M = 16)";
	if (flags & OA_F_COUNT) return "odd.aln: its counts disagree with its header, with len.bin or with the size of odd.seq";
	if (flags & OA_F_SHORT) return "odd.aln: an aligned read is shorter than 31 bases";
	if (flags & OA_F_WINDOW) return "odd.aln: a read's window leaves the contigs";
	if (flags & OA_F_BUDGET) return "odd.aln: a read has more mismatches than its length allows";
	if (flags & OA_F_OFFSET) return "odd.aln: a mismatch lies outside its read";
	if (flags & OA_F_BASE) return "odd.aln: a mismatch base outside ACGTN";
	if (flags & OA_F_SAME) return "odd.aln: a mismatch repeats the contig's base";
	if (flags & OA_F_CRC) return "odd.aln: the rebuilt odd text fails its CRC-32";
	return "odd.aln: accepted";
}

OA_HD uint32_t oa_budget(uint32_t l) { return (l - OA_K) / 8; }          // E(l), for l >= K
OA_HD uint64_t oa_hit(uint32_t d, uint32_t s, uint64_t p) { return (uint64_t)d << 48 | (uint64_t)s << 40 | p; }
OA_HD uint32_t oa_hit_d(uint64_t h) { return (uint32_t)(h >> 48); }
OA_HD uint32_t oa_hit_s(uint64_t h) { return (uint32_t)(h >> 40) & 1u; }
OA_HD uint64_t oa_hit_p(uint64_t h) { return h & (OA_MAX_T - 1); }
// A C G T -> 0 .. 3, N -> 4, anything else -> 5
OA_HD uint32_t oa_code(uint8_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : c == 'N' ? 4u : 5u; }
OA_HD uint8_t oa_char(uint32_t code) { return code == 0 ? 'A' : code == 1 ? 'C' : code == 2 ? 'G' : code == 3 ? 'T' : 'N'; }
OA_HD uint32_t oa_comp(uint32_t code) { return code < 4 ? 3u - code : code; }
// words of a packed text of n bases, the word of zeros behind it included
OA_HD uint64_t oa_words(uint64_t n_bases) { return (n_bases + 31) / 32 + 1; }
// the 32 bases from base `at` of a packed text (at / 32 + 1 must be a word of it: the padding word makes it so for every at <= n)
OA_HD uint64_t oa_window(const uint64_t *w, uint64_t at)
{
	const uint64_t i = at >> 5; const uint32_t sh = 2u * (uint32_t)(at & 31);
	return sh ? (w[i] >> sh) | (w[i + 1] << (64 - sh)) : w[i];
}
OA_HD uint32_t oa_base(const uint64_t *w, uint64_t at) { return (uint32_t)(w[at >> 5] >> (2u * (uint32_t)(at & 31))) & 3u; }
OA_HD uint64_t oa_key(const uint64_t *w, uint64_t at) { return oa_window(w, at) & OA_KEY_MASK; }
// grid entries of a text of n bases
OA_HD uint64_t oa_grid_size(uint64_t n_bases) { return n_bases < OA_K ? 0 : (n_bases - OA_K) / OA_G + 1; }
// the places where two windows of 32 bases differ, one bit (2 j) per base
OA_HD uint64_t oa_diff32(uint64_t a, uint64_t b) { const uint64_t x = a ^ b; return (x | (x >> 1)) & 0x5555555555555555ull; }

// ---- the member: header, then planar arrays (all little endian)
//  0 "MCOMOAL1"   8 K   12 G   16 M   20 CRC-32 of the full odd text   24 n_odd   32 n_aligned   40 |T|   48 n_mismatch   56 residual bytes
// 64 aligned bits (one per odd record), strand bits (one per aligned record), 5 planes of n_aligned bytes of p, n_aligned bytes of d,
//    n_mismatch offsets (per read ascending: the first as it is, the others minus the one before minus 1), n_mismatch bases
struct OaLayout { uint64_t n_odd, n_aligned, n_mm, aligned, strand, p, d, mm_off, mm_base, total; };
OA_HD OaLayout oa_layout(uint64_t n_odd, uint64_t n_aligned, uint64_t n_mm)
{
	OaLayout Y;
	Y.n_odd = n_odd; Y.n_aligned = n_aligned; Y.n_mm = n_mm;
	Y.aligned = OA_HEADER;
	Y.strand = Y.aligned + (n_odd + 7) / 8;
	Y.p = Y.strand + (n_aligned + 7) / 8;
	Y.d = Y.p + 5 * n_aligned;
	Y.mm_off = Y.d + n_aligned;
	Y.mm_base = Y.mm_off + n_mm;
	Y.total = Y.mm_base + n_mm;
	return Y;
}
struct OaHeader { uint32_t K, G, M, crc; uint64_t n_odd, n_aligned, t_bases, n_mm, residual; };
inline uint64_t oa_get(const uint8_t *p, int bytes) { uint64_t v = 0; for (int i = 0; i < bytes; ++i) v |= (uint64_t)p[i] << (8 * i); return v; }
inline void oa_put(uint8_t *p, int bytes, uint64_t v) { for (int i = 0; i < bytes; ++i) p[i] = (uint8_t)(v >> (8 * i)); }
inline void oa_header_put(uint8_t *m, const OaHeader &H)
{
	for (int i = 0; i < 8; ++i) m[i] = (uint8_t)OA_MAGIC[i];
	oa_put(m + 8, 4, H.K); oa_put(m + 12, 4, H.G); oa_put(m + 16, 4, H.M); oa_put(m + 20, 4, H.crc);
	oa_put(m + 24, 8, H.n_odd); oa_put(m + 32, 8, H.n_aligned); oa_put(m + 40, 8, H.t_bases); oa_put(m + 48, 8, H.n_mm); oa_put(m + 56, 8, H.residual);
}
// the header of an untrusted member against what the caller knows (the odd records of len.bin, |T|, the residual's size): flags, 0 = go on
inline uint32_t oa_header_check(const uint8_t *m, uint64_t len, uint64_t n_odd, uint64_t odd_bytes, uint64_t t_bases, uint64_t residual, OaHeader &H)
{
	if (len < OA_HEADER) return OA_F_HEADER;
	for (int i = 0; i < 8; ++i) if (m[i] != (uint8_t)OA_MAGIC[i]) return OA_F_HEADER;
	H.K = (uint32_t)oa_get(m + 8, 4); H.G = (uint32_t)oa_get(m + 12, 4); H.M = (uint32_t)oa_get(m + 16, 4); H.crc = (uint32_t)oa_get(m + 20, 4);
	H.n_odd = oa_get(m + 24, 8); H.n_aligned = oa_get(m + 32, 8); H.t_bases = oa_get(m + 40, 8); H.n_mm = oa_get(m + 48, 8); H.residual = oa_get(m + 56, 8);
	if (H.K != OA_K || H.G != OA_G || H.M != OA_M) return OA_F_HEADER;
	if (H.n_odd != n_odd || H.n_aligned > n_odd || H.n_aligned == 0 || H.t_bases != t_bases || H.residual != residual || H.residual > odd_bytes ||
	    H.n_mm > H.n_aligned * (uint64_t)oa_budget(OA_MAX_LEN)) return OA_F_COUNT;
	if (oa_layout(H.n_odd, H.n_aligned, H.n_mm).total != len) return OA_F_COUNT;
	return 0;
}

// ---- one read: what the encoder, the decoder and their twins do per record, stated once
// base j of the read laid on T at p in orientation s, as T has it there: the window's base under the READ's position j
OA_HD uint32_t oa_window_code(const uint64_t *t, uint32_t l, uint32_t s, uint64_t p, uint32_t j)
{
	const uint32_t c = oa_base(t, p + (s ? l - 1 - j : j));
	return s ? 3u - c : c;
}
// the places where the read (l characters in ACGTN) differs from its window; mm_off / mm_base (may be NULL: counted only) get them in the
// member's coding.  The caller has checked p + l <= |T|.
OA_HD uint32_t oa_encode_read(const uint64_t *t, const uint8_t *read, uint32_t l, uint32_t s, uint64_t p, uint8_t *mm_off, uint8_t *mm_base)
{
	uint32_t n = 0, prev = 0;
	for (uint32_t j = 0; j < l; ++j) {
		if (oa_code(read[j]) == oa_window_code(t, l, s, p, j)) continue;
		if (mm_off) { mm_off[n] = (uint8_t)(n ? j - prev - 1 : j); mm_base[n] = read[j]; }
		prev = j; ++n;
	}
	return n;
}
// the read back into out[0, l): the window in the read's orientation with the d mismatches laid over it.  Returns the flags of what is
// wrong with it; nothing but out[0, l) is written, and nothing at all for a read whose length, window or d is refused.
OA_HD uint32_t oa_decode_read(const uint64_t *t, uint64_t t_bases, uint32_t l, uint32_t s, uint64_t p, uint32_t d, const uint8_t *mm_off, const uint8_t *mm_base, uint8_t *out)
{
	if (l < OA_MIN_LEN) return OA_F_SHORT;
	if (p > t_bases || l > t_bases - p) return OA_F_WINDOW;
	if (d > oa_budget(l)) return OA_F_BUDGET;
	for (uint32_t j = 0; j < l; ++j) out[j] = oa_char(oa_window_code(t, l, s, p, j));
	uint32_t at = 0, flags = 0;
	for (uint32_t k = 0; k < d; ++k) {
		at = k ? at + 1 + mm_off[k] : mm_off[0];
		if (at >= l) return flags | OA_F_OFFSET;
		const uint8_t b = mm_base[k];
		if (oa_code(b) > 4) flags |= OA_F_BASE;
		else if (out[at] == b) flags |= OA_F_SAME;
		else out[at] = b;
	}
	return flags;
}
