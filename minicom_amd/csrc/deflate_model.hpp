// minicom_amd/csrc/deflate_model.hpp -- BGZF output (`minicom -d -z`): the ONE statement of everything that
// decides a byte of a member.  csrc/bgzf.hip (the kernels) and host/mcom_bgzf.cpp (the host twin) both compile it, so the two cannot
// drift apart: the 4-byte hash, the candidate and match rules, the length and distance symbols, the length-limited code construction
// with its total order on ties, the run-length coding of the code lengths, the HLIT / HDIST / HCLEN trimming, the dynamic-or-stored
// decision and the CRC-32 combine step.
//
// The parse of one block of n <= 65280 bytes (members decode alone, nothing outside the block is looked at):
//   positions are taken in tiles of 256.  Position p has at most two candidates: p - 1, and the largest q BELOW THE START OF p's
//   TILE with hash4(q) == hash4(p) and p - q <= 32768 (a table of 2^13 slots that holds, after each tile, the largest position per
//   slot: a maximum is order-free, so atomicMax in LDS and a plain loop agree).  The longer match wins, up to 258 and never past the
//   block's end; a tie goes to distance 1.  A match is used from length 4, or from 3 at distance 1.  The block is then parsed
//   greedily from position 0: at p the match if there is one (then p += length), the literal otherwise (p += 1).
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define MCOM_DM_HD __host__ __device__
#else
#define MCOM_DM_HD
#endif

namespace mcom_deflate {

enum { BLOCK = 65280, TILE = 256, HASH_BITS = 13, HASH_SLOTS = 1 << HASH_BITS, WINDOW = 32768, MAX_MATCH = 258,
       N_LL = 286, N_D = 30, N_CL = 19, EOB = 256, LL_BITS = 15, CL_BITS = 7,
       HEADER_BYTES = 18, TRAILER_BYTES = 8, STORED_BYTES = 5, MEMBER_EXTRA = HEADER_BYTES + STORED_BYTES + TRAILER_BYTES, EOF_BYTES = 28,
       TEXT_WORDS = BLOCK / 8 + 2,                       // a block as little-endian 64-bit words, zero behind its end
       CRC_CHUNK = 264,                                  // bytes per chunk CRC (33 words: lanes 264 bytes apart fall into different LDS banks)
       MAX_TOKENS = BLOCK + 1,                           // every byte a literal, and the end-of-block symbol
       TOK_MATCH = (int)0x80000000 };

MCOM_DM_HD inline uint64_t bound(uint64_t n) { return n + (uint64_t)MEMBER_EXTRA * ((n + BLOCK - 1) / BLOCK) + EOF_BYTES; }

// the empty member every BGZF file ends with
MCOM_DM_HD inline uint8_t eof_byte(uint32_t i)
{
	return i == 0 ? 0x1f : i == 1 ? 0x8b : i == 2 ? 0x08 : i == 3 ? 0x04 : i == 9 ? 0xff : i == 10 ? 0x06 : i == 12 ? 0x42 : i == 13 ? 0x43 :
	       i == 14 ? 0x02 : i == 16 ? 0x1b : i == 18 ? 0x03 : 0x00;
}
// the 18 bytes in front of a member of `size` bytes in all
MCOM_DM_HD inline uint8_t header_byte(uint32_t i, uint32_t size)
{
	return i == 16 ? (uint8_t)((size - 1) & 255) : i == 17 ? (uint8_t)((size - 1) >> 8) : eof_byte(i);
}

// ---- text, hash, matches ----
MCOM_DM_HD inline uint64_t load64(const uint64_t *w, uint32_t p)
{
	const uint32_t i = p >> 3, s = (p & 7) * 8;
	const uint64_t lo = w[i];
	return s ? (lo >> s) | (w[i + 1] << (64 - s)) : lo;
}
MCOM_DM_HD inline uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - HASH_BITS); }

// common prefix of the text at p and at q < p, at most maxlen <= n - p
MCOM_DM_HD inline uint32_t match_len(const uint64_t *w, uint32_t p, uint32_t q, uint32_t maxlen)
{
	uint32_t i = 0;
	while (i < maxlen) {
		const uint64_t x = load64(w, p + i) ^ load64(w, q + i);
		if (x) { i += (uint32_t)__builtin_ctzll(x) >> 3; break; }
		i += 8;
	}
	return i < maxlen ? i : maxlen;
}

struct Match { uint32_t len, dist; };                   // len 0: a literal
// entry: the table's word for hash4(p) as it stood before p's tile (position + 1, 0 = none); looked at only when p + 4 <= n
MCOM_DM_HD inline Match find_match(const uint64_t *w, uint32_t n, uint32_t p, uint32_t entry)
{
	Match m = {0, 0};
	const uint32_t maxlen = n - p < MAX_MATCH ? n - p : MAX_MATCH;
	if (maxlen < 3) return m;
	uint32_t la = 0, lb = 0, db = 0;
	if (p >= 1) la = match_len(w, p, p - 1, maxlen);
	if (p + 4 <= n && entry) {
		db = p - (entry - 1);
		if (db <= WINDOW) lb = match_len(w, p, entry - 1, maxlen);
	}
	uint32_t len = la, dist = 1;
	if (lb > la) { len = lb; dist = db; }
	if (len >= 4 || (len == 3 && dist == 1)) { m.len = len; m.dist = dist; }
	return m;
}

// tokens: a literal is its byte, the end of the block is EOB, a match is TOK_MATCH | (len - 3) << 16 | (dist - 1)
MCOM_DM_HD inline uint32_t match_token(Match m) { return (uint32_t)TOK_MATCH | ((m.len - 3) << 16) | (m.dist - 1); }

// ---- RFC 1951 symbols ----
MCOM_DM_HD inline void len_symbol(uint32_t len, uint32_t &sym, uint32_t &ebits, uint32_t &eval)
{
	const uint32_t l = len - 3;
	if (len == MAX_MATCH) { sym = 285; ebits = 0; eval = 0; return; }
	if (l < 8) { sym = 257 + l; ebits = 0; eval = 0; return; }
	ebits = 29 - (uint32_t)__builtin_clz(l);                      // floor(log2(l)) - 2
	sym = 261 + 4 * ebits + ((l - (4u << ebits)) >> ebits);
	eval = l & ((1u << ebits) - 1);
}
MCOM_DM_HD inline void dist_symbol(uint32_t dist, uint32_t &sym, uint32_t &ebits, uint32_t &eval)
{
	const uint32_t d = dist - 1;
	if (d < 4) { sym = d; ebits = 0; eval = 0; return; }
	const uint32_t k = 31 - (uint32_t)__builtin_clz(d);
	ebits = k - 1;
	sym = 2 * k + ((d >> (k - 1)) & 1);
	eval = d & ((1u << ebits) - 1);
}
MCOM_DM_HD inline uint32_t len_extra_bits(uint32_t sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }
MCOM_DM_HD inline uint32_t dist_extra_bits(uint32_t sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }

// ---- length-limited prefix codes ----
struct Work {                                           // scratch of make_lengths / plan_block (in LDS on the device)
	uint32_t f[288];
	uint32_t wt[576];
	uint16_t sym[288], par[576];
	uint8_t dep[576], cat[N_LL + N_D + 4];
	uint32_t num[48];
};

// Code lengths of at most maxbits for the symbols with freq > 0.  Fewer than two used symbols are padded to two as zlib does (the
// code is then complete and every inflater takes it).  Symbols are sorted by (frequency, symbol); the Huffman tree is built with two
// queues, a leaf before an internal node of the same weight; only the NUMBER of codes per length is kept, lengths above maxbits are
// folded down and the Kraft sum is repaired from the longest codes; the sorted symbols then take the lengths, rarest longest.
MCOM_DM_HD inline void make_lengths(const uint32_t *freq, uint32_t nsym, uint32_t maxbits, uint8_t *lens, Work *k)
{
	uint32_t m = 0;
	int maxcode = -1;
	for (uint32_t s = 0; s < nsym; ++s) { k->f[s] = freq[s]; lens[s] = 0; if (freq[s]) { ++m; maxcode = (int)s; } }
	while (m < 2) {
		const uint32_t node = maxcode < 2 ? (uint32_t)++maxcode : 0;
		k->f[node] = 1; ++m;
	}
	// insertion sort by (frequency, symbol): symbols come in ascending order, so equal frequencies keep it
	m = 0;
	for (uint32_t s = 0; s < nsym; ++s) {
		if (!k->f[s]) continue;
		uint32_t i = m++;
		while (i > 0 && k->f[k->sym[i - 1]] > k->f[s]) { k->sym[i] = k->sym[i - 1]; --i; }
		k->sym[i] = (uint16_t)s;
	}
	for (uint32_t i = 0; i < m; ++i) k->wt[i] = k->f[k->sym[i]];
	uint32_t a = 0, b = m;
	for (uint32_t t = m; t < 2 * m - 1; ++t) {
		uint32_t w = 0;
		for (int c = 0; c < 2; ++c) {
			uint32_t x;
			if (a < m && (b >= t || k->wt[a] <= k->wt[b])) x = a++; else x = b++;
			w += k->wt[x]; k->par[x] = (uint16_t)t;
		}
		k->wt[t] = w;
	}
	for (uint32_t i = 0; i < 48; ++i) k->num[i] = 0;
	k->dep[2 * m - 2] = 0;
	for (int x = (int)(2 * m - 3); x >= 0; --x) {
		const uint32_t d = k->dep[k->par[x]] + 1u;
		k->dep[x] = (uint8_t)(d < 47 ? d : 47);
		if ((uint32_t)x < m) ++k->num[k->dep[x]];
	}
	for (uint32_t i = maxbits + 1; i < 48; ++i) { k->num[maxbits] += k->num[i]; k->num[i] = 0; }
	uint32_t total = 0;
	for (uint32_t i = maxbits; i > 0; --i) total += k->num[i] << (maxbits - i);
	while (total > (1u << maxbits)) {
		--k->num[maxbits];
		for (uint32_t i = maxbits - 1; i > 0; --i) if (k->num[i]) { --k->num[i]; k->num[i + 1] += 2; break; }
		--total;
	}
	uint32_t at = 0;
	for (uint32_t l = maxbits; l > 0; --l) for (uint32_t c = 0; c < k->num[l]; ++c) lens[k->sym[at++]] = (uint8_t)l;
}

MCOM_DM_HD inline uint32_t bit_reverse(uint32_t v, uint32_t bits)
{
	uint32_t r = 0;
	for (uint32_t i = 0; i < bits; ++i) { r = (r << 1) | (v & 1); v >>= 1; }
	return r;
}
// canonical codes (RFC 1951 3.2.2), bit-reversed: ready to be written from bit 0
MCOM_DM_HD inline void make_codes(const uint8_t *lens, uint32_t nsym, uint32_t maxbits, uint16_t *codes)
{
	uint32_t count[16], next[16];
	for (uint32_t i = 0; i < 16; ++i) count[i] = 0;
	for (uint32_t s = 0; s < nsym; ++s) ++count[lens[s]];
	count[0] = 0;
	uint32_t code = 0;
	next[0] = 0;
	for (uint32_t b = 1; b <= maxbits; ++b) { code = (code + count[b - 1]) << 1; next[b] = code; }
	for (uint32_t s = 0; s < nsym; ++s) codes[s] = lens[s] ? (uint16_t)bit_reverse(next[lens[s]]++, lens[s]) : 0;
}

// ---- the block's plan: both codes, the coded code lengths, dynamic or stored ----
struct Plan {
	uint16_t ll_code[288], d_code[32], cl_code[N_CL];
	uint16_t rle[N_LL + N_D + 4];                       // symbol of the code-length code | extra value << 5
	uint8_t ll_len[288], d_len[32], cl_len[N_CL];
	uint32_t n_rle, hlit, hdist, hclen, stored;
	uint64_t dyn_bits;                                  // the whole dynamic block: its 3 header bits to the end-of-block code
};
MCOM_DM_HD inline uint32_t cl_order(uint32_t i)
{
	return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? (19 - i) >> 1 : (i + 12) >> 1;           // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
}

// ll_freq counts the end-of-block symbol once; n: the block's bytes
MCOM_DM_HD inline void plan_block(const uint32_t *ll_freq, const uint32_t *d_freq, uint32_t n, Plan *pl, Work *k)
{
	make_lengths(ll_freq, N_LL, LL_BITS, pl->ll_len, k);
	make_lengths(d_freq, N_D, LL_BITS, pl->d_len, k);
	make_codes(pl->ll_len, N_LL, LL_BITS, pl->ll_code);
	make_codes(pl->d_len, N_D, LL_BITS, pl->d_code);
	uint32_t hlit = N_LL, hdist = N_D;
	while (hlit > 257 && !pl->ll_len[hlit - 1]) --hlit;
	while (hdist > 1 && !pl->d_len[hdist - 1]) --hdist;
	pl->hlit = hlit; pl->hdist = hdist;
	const uint32_t nc = hlit + hdist;
	for (uint32_t i = 0; i < hlit; ++i) k->cat[i] = pl->ll_len[i];
	for (uint32_t i = 0; i < hdist; ++i) k->cat[hlit + i] = pl->d_len[i];
	// runs of equal lengths, across the border of the two alphabets: zeros as 18 (11 .. 138) while 11 are left, then 17 (3 .. 10); another
	// length once as itself, then 16 (3 .. 6) while 3 are left; what remains as itself
	uint32_t cl_freq[N_CL];
	for (uint32_t i = 0; i < N_CL; ++i) cl_freq[i] = 0;
	uint32_t nr = 0;
	for (uint32_t i = 0; i < nc; ) {
		const uint32_t v = k->cat[i];
		uint32_t run = 1;
		while (i + run < nc && k->cat[i + run] == v) ++run;
		i += run;
		if (v == 0) {
			while (run >= 11) { const uint32_t c = run < 138 ? run : 138; pl->rle[nr++] = (uint16_t)(18 | ((c - 11) << 5)); ++cl_freq[18]; run -= c; }
			if (run >= 3) { pl->rle[nr++] = (uint16_t)(17 | ((run - 3) << 5)); ++cl_freq[17]; run = 0; }
		} else {
			pl->rle[nr++] = (uint16_t)v; ++cl_freq[v]; --run;
			while (run >= 3) { const uint32_t c = run < 6 ? run : 6; pl->rle[nr++] = (uint16_t)(16 | ((c - 3) << 5)); ++cl_freq[16]; run -= c; }
		}
		for (; run; --run) { pl->rle[nr++] = (uint16_t)v; ++cl_freq[v]; }
	}
	pl->n_rle = nr;
	make_lengths(cl_freq, N_CL, CL_BITS, pl->cl_len, k);
	make_codes(pl->cl_len, N_CL, CL_BITS, pl->cl_code);
	uint32_t hclen = N_CL;
	while (hclen > 4 && !pl->cl_len[cl_order(hclen - 1)]) --hclen;
	pl->hclen = hclen;
	uint64_t bits = 3 + 5 + 5 + 4 + 3 * hclen;
	for (uint32_t i = 0; i < N_CL; ++i) bits += (uint64_t)cl_freq[i] * (pl->cl_len[i] + (i == 16 ? 2u : i == 17 ? 3u : i == 18 ? 7u : 0u));
	for (uint32_t s = 0; s < N_LL; ++s) bits += (uint64_t)ll_freq[s] * (pl->ll_len[s] + len_extra_bits(s));
	for (uint32_t s = 0; s < N_D; ++s) bits += (uint64_t)d_freq[s] * (pl->d_len[s] + dist_extra_bits(s));
	pl->dyn_bits = bits;
	pl->stored = (bits + 7) / 8 < (uint64_t)STORED_BYTES + n ? 0 : 1;             // dynamic only where it is strictly smaller
}

// the dynamic block's header through put(value, bits), least significant bit first
template <class Put> MCOM_DM_HD inline void write_header(const Plan *pl, Put &put)
{
	put(1u, 1u); put(2u, 2u);                                                      // BFINAL, BTYPE = dynamic
	put(pl->hlit - 257, 5u); put(pl->hdist - 1, 5u); put(pl->hclen - 4, 4u);
	for (uint32_t i = 0; i < pl->hclen; ++i) put((uint32_t)pl->cl_len[cl_order(i)], 3u);
	for (uint32_t i = 0; i < pl->n_rle; ++i) {
		const uint32_t s = pl->rle[i] & 31, e = pl->rle[i] >> 5;
		put((uint32_t)pl->cl_code[s], (uint32_t)pl->cl_len[s]);
		if (s >= 16) put(e, s == 16 ? 2u : s == 17 ? 3u : 7u);
	}
}

// a token's bits (at most 48) and their number
MCOM_DM_HD inline void encode_token(const Plan *pl, uint32_t tok, uint64_t &bits, uint32_t &nbits)
{
	if (!(tok & (uint32_t)TOK_MATCH)) { bits = pl->ll_code[tok]; nbits = pl->ll_len[tok]; return; }
	uint32_t s, eb, ev;
	len_symbol(((tok >> 16) & 255) + 3, s, eb, ev);
	bits = pl->ll_code[s]; nbits = pl->ll_len[s];
	bits |= (uint64_t)ev << nbits; nbits += eb;
	dist_symbol((tok & 0xFFFF) + 1, s, eb, ev);
	bits |= (uint64_t)pl->d_code[s] << nbits; nbits += pl->d_len[s];
	bits |= (uint64_t)ev << nbits; nbits += eb;
}

// ---- CRC-32 (reflected, 0xEDB88320) ----
MCOM_DM_HD inline uint32_t crc_table_entry(uint32_t i)
{
	uint32_t c = i;
	for (int b = 0; b < 8; ++b) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
	return c;
}
// CRC-32 of the text's bytes [begin, end)
MCOM_DM_HD inline uint32_t crc_chunk(const uint64_t *w, uint32_t begin, uint32_t end, const uint32_t *table)
{
	uint32_t c = 0xFFFFFFFFu;
	for (uint32_t p = begin; p < end; ++p) c = table[(c ^ (uint32_t)(w[p >> 3] >> ((p & 7) * 8))) & 255] ^ (c >> 8);
	return ~c;
}
// a(x) b(x) mod P(x), polynomials with the coefficient of x^0 in bit 31
MCOM_DM_HD inline uint32_t crc_mul(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (uint32_t m = 0x80000000u; m; m >>= 1) {
		if (a & m) p ^= b;
		b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
	}
	return p;
}
// CRC-32 of A B from crc(A), crc(B) and the length of B: crc(A) x^(8 len) + crc(B)
MCOM_DM_HD inline uint32_t crc_combine(uint32_t crc_a, uint32_t crc_b, uint32_t len_b)
{
	uint32_t r = 0x80000000u, sq = 0x00800000u;                                    // 1 and x^8
	for (uint32_t n = len_b; n; n >>= 1) {
		if (n & 1) r = crc_mul(sq, r);
		if (n > 1) sq = crc_mul(sq, sq);
	}
	return crc_mul(r, crc_a) ^ crc_b;
}

}  // namespace mcom_deflate
