// minicom_amd/csrc/inflate_model.hpp -- gzip members inflated on the GPU: the ONE statement of everything that
// decides whether a member is valid and what comes out of it.  csrc/inflate.hip (the kernel) and host/mcom_gzip_gpu.cpp (the host twin)
// both compile it: the bit reader over a bounded payload, the three block headers, the code-length code with its repeat codes, the
// table build, the decoding of one token and every bounds rule.
//
// Every loop here ends on any input: a step either takes at least one bit of the bounded payload, or raises a counter that is bounded
// by a constant, or stops.  No table index comes from the stream unmasked, no distance reaches in front of the member's own output and
// no store behind its slot.
//
// Tables (compact, so that many members are in flight per CU): a first level of 2^10 (literal/length) and 2^8 (distance) 16-bit
// entries `symbol << 4 | code length`, 0 where no code of at most that many bits ends; longer codes, and the unused patterns of an
// incomplete code, go through the canonical walk over the number of codes per length (at most 15 steps).
#pragma once
#include "deflate_model.hpp"

namespace mcom_inflate_model {

using mcom_deflate::bit_reverse;
using mcom_deflate::cl_order;
using mcom_deflate::len_extra_bits;
using mcom_deflate::dist_extra_bits;

enum { ST_OK = 0, ST_CORRUPT = 1, ST_TRUNCATED = 2, ST_ROOM = 3, ST_CHECK = 4,
       ST_EOB = 16 };                                   // decode_token only: the block's end code (never a member's status)
enum { LL_FAST = 10, D_FAST = 8, BATCH = 64, N_LL_MAX = 288, N_D_MAX = 32, N_CL = 19, MAX_BITS = 15,
       TOK_MATCH = (int)0x80000000 };

// ---- the bit reader: `bl` valid bits at the bottom of `bb`, nothing above them; p[at ..] not yet loaded ----
struct Bits { const uint8_t *p; uint64_t n, at, bb; uint32_t bl; };

MCOM_DM_HD inline void bits_begin(Bits &b, const uint8_t *p, uint64_t n) { b.p = p; b.n = n; b.at = 0; b.bb = 0; b.bl = 0; }
// afterwards bl >= 57, or every bit of the payload that is left is in bb (at most 8 steps)
MCOM_DM_HD inline void refill(Bits &b)
{
	while (b.bl <= 56 && b.at < b.n) { b.bb |= (uint64_t)b.p[b.at++] << b.bl; b.bl += 8; }
}
// k <= 16 bits, the caller has seen bl >= k
MCOM_DM_HD inline uint32_t take(Bits &b, uint32_t k)
{
	const uint32_t v = (uint32_t)b.bb & ((1u << k) - 1);
	b.bb >>= k; b.bl -= k;
	return v;
}

// ---- a canonical code: codes per length, and where each length begins among the codes and among the sorted symbols ----
struct Code { uint16_t cnt[16], first[16], off[16]; };

struct Tables {
	uint16_t ll_fast[1 << LL_FAST], d_fast[1 << D_FAST];
	uint16_t ll_sym[N_LL_MAX], d_sym[N_D_MAX], cl_sym[N_CL + 1];
	Code ll, d, cl;
	uint8_t lens[N_LL_MAX + N_D_MAX];                   // the block's code lengths: hlit of the literal/length code, then hdist
	uint8_t cl_len[N_CL + 1];
	uint32_t hlit, hdist;
};

// Code lengths -> cnt, first, off and the symbols sorted by (length, symbol).  false: over-subscribed.  An incomplete code is taken (a
// distance code of one length is legal and zlib writes it); its unused patterns are corrupt when the stream shows one.
MCOM_DM_HD inline bool count_code(const uint8_t *lens, uint32_t n, Code &c, uint16_t *sym)
{
	for (uint32_t l = 0; l < 16; ++l) c.cnt[l] = 0;
	for (uint32_t s = 0; s < n; ++s) ++c.cnt[lens[s] & 15];
	c.cnt[0] = 0;
	uint32_t left = 1;
	for (uint32_t l = 1; l <= MAX_BITS; ++l) { left <<= 1; if (c.cnt[l] > left) return false; left -= c.cnt[l]; }
	uint32_t code = 0, o = 0;
	c.first[0] = 0; c.off[0] = 0;
	for (uint32_t l = 1; l <= MAX_BITS; ++l) { code = (code + c.cnt[l - 1]) << 1; c.first[l] = (uint16_t)code; c.off[l] = (uint16_t)o; o += c.cnt[l]; }
	uint16_t nx[16];
	for (uint32_t l = 0; l < 16; ++l) nx[l] = c.off[l];
	for (uint32_t s = 0; s < n; ++s) { const uint32_t l = lens[s] & 15; if (l) sym[nx[l]++] = (uint16_t)s; }
	return true;
}
MCOM_DM_HD inline uint32_t code_symbols(const Code &c) { return (uint32_t)c.off[MAX_BITS] + c.cnt[MAX_BITS]; }

// The first level, in two steps that many lanes share (i0 = the lane, stride = their number) with a barrier between them.
MCOM_DM_HD inline void clear_fast(uint16_t *fast, uint32_t fast_bits, uint32_t i0, uint32_t stride)
{
	for (uint32_t i = i0; i < (1u << fast_bits); i += stride) fast[i] = 0;
}
MCOM_DM_HD inline void fill_fast(const uint8_t *lens, const Code &c, const uint16_t *sym, uint16_t *fast, uint32_t fast_bits, uint32_t i0, uint32_t stride)
{
	const uint32_t total = code_symbols(c);
	for (uint32_t i = i0; i < total; i += stride) {
		const uint32_t s = sym[i], l = lens[s] & 15;
		if (!l || l > fast_bits) continue;
		const uint32_t r = bit_reverse((uint32_t)c.first[l] + (i - c.off[l]), l);
		for (uint32_t j = r; j < (1u << fast_bits); j += 1u << l) fast[j] = (uint16_t)((s << 4) | l);
	}
}

// One symbol.  fast may be NULL (the code-length code).  ST_TRUNCATED: the code needs bits behind the payload's end.
MCOM_DM_HD inline int decode_sym(Bits &b, const Code &c, const uint16_t *sym, const uint16_t *fast, uint32_t fast_bits, uint32_t &out)
{
	if (fast) {
		const uint32_t e = fast[(uint32_t)b.bb & ((1u << fast_bits) - 1)];
		if (e) {
			const uint32_t l = e & 15;
			if (l > b.bl) return ST_TRUNCATED;
			(void)take(b, l);
			out = e >> 4;
			return ST_OK;
		}
	}
	uint32_t code = 0, first = 0, index = 0, v = (uint32_t)b.bb;
	for (uint32_t l = 1; l <= MAX_BITS; ++l) {
		code |= v & 1; v >>= 1;
		const uint32_t count = c.cnt[l];
		if (code < first + count) {                            // (code >= first always: the walk keeps it so)
			if (l > b.bl) return ST_TRUNCATED;
			(void)take(b, l);
			out = sym[index + (code - first)];
			return ST_OK;
		}
		index += count; first = (first + count) << 1; code <<= 1;
	}
	return b.bl < MAX_BITS ? ST_TRUNCATED : ST_CORRUPT;
}

// ---- block headers ----
// The three header bits.  type 0: stored_begin follows; 1 and 2: T.lens, T.hlit and T.hdist are set and block_codes follows.
MCOM_DM_HD inline int block_header(Bits &b, Tables &T, uint32_t &last, uint32_t &type)
{
	refill(b);
	if (b.bl < 3) return ST_TRUNCATED;
	last = take(b, 1); type = take(b, 2);
	if (type == 3) return ST_CORRUPT;
	if (type == 0) return ST_OK;
	if (type == 1) {
		for (uint32_t i = 0; i < 288; ++i) T.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
		for (uint32_t i = 0; i < 32; ++i) T.lens[288 + i] = 5;
		T.hlit = 288; T.hdist = 32;                            // (symbols 286, 287 and distances 30, 31 have codes; decode_token refuses them)
		return ST_OK;
	}
	refill(b);
	if (b.bl < 14) return ST_TRUNCATED;
	const uint32_t hlit = take(b, 5) + 257, hdist = take(b, 5) + 1, hclen = take(b, 4) + 4;
	if (hlit > 286 || hdist > 30) return ST_CORRUPT;
	for (uint32_t i = 0; i < N_CL; ++i) T.cl_len[i] = 0;
	for (uint32_t i = 0; i < hclen; ++i) {
		refill(b);
		if (b.bl < 3) return ST_TRUNCATED;
		T.cl_len[cl_order(i)] = (uint8_t)take(b, 3);
	}
	if (!count_code(T.cl_len, N_CL, T.cl, T.cl_sym)) return ST_CORRUPT;
	const uint32_t total = hlit + hdist;
	uint32_t at = 0;
	while (at < total) {                                       // every turn takes a bit and raises `at`, or returns
		refill(b);
		uint32_t s = 0;
		const int st = decode_sym(b, T.cl, T.cl_sym, nullptr, 0, s);
		if (st) return st;
		if (s < 16) { T.lens[at++] = (uint8_t)s; continue; }
		uint32_t rep, xb; uint8_t v = 0;
		if (s == 16) { if (!at) return ST_CORRUPT; v = T.lens[at - 1]; xb = 2; rep = 3; }
		else if (s == 17) { xb = 3; rep = 3; }
		else { xb = 7; rep = 11; }
		if (b.bl < xb) return ST_TRUNCATED;
		rep += take(b, xb);
		if (at + rep > total) return ST_CORRUPT;               // a repeat may cross from the literal lengths into the distance lengths, not past both
		for (uint32_t i = 0; i < rep; ++i) T.lens[at + i] = v;
		at += rep;
	}
	if (T.lens[256] == 0) return ST_CORRUPT;                   // no end-of-block code
	T.hlit = hlit; T.hdist = hdist;
	return ST_OK;
}
// both codes of a Huffman block from T.lens (one lane); the first levels follow through clear_fast / fill_fast (all lanes)
MCOM_DM_HD inline int block_codes(Tables &T)
{
	if (!count_code(T.lens, T.hlit, T.ll, T.ll_sym) || !count_code(T.lens + T.hlit, T.hdist, T.d, T.d_sym)) return ST_CORRUPT;
	return ST_OK;
}
MCOM_DM_HD inline void block_fast_clear(Tables &T, uint32_t i0, uint32_t stride)
{
	clear_fast(T.ll_fast, LL_FAST, i0, stride); clear_fast(T.d_fast, D_FAST, i0, stride);
}
MCOM_DM_HD inline void block_fast_fill(Tables &T, uint32_t i0, uint32_t stride)
{
	fill_fast(T.lens, T.ll, T.ll_sym, T.ll_fast, LL_FAST, i0, stride);
	fill_fast(T.lens + T.hlit, T.d, T.d_sym, T.d_fast, D_FAST, i0, stride);
}

// A stored block behind its three header bits: the rest of the byte is dropped, LEN and NLEN checked; its len bytes are p[at ..) and
// the caller copies them (ST_ROOM when they do not fit) and calls stored_end.
MCOM_DM_HD inline int stored_begin(Bits &b, uint32_t &len)
{
	b.at -= b.bl >> 3; b.bb = 0; b.bl = 0;                     // whole bytes in the buffer go back
	if (b.n - b.at < 4) return ST_TRUNCATED;
	const uint32_t l = (uint32_t)b.p[b.at] | ((uint32_t)b.p[b.at + 1] << 8), nl = (uint32_t)b.p[b.at + 2] | ((uint32_t)b.p[b.at + 3] << 8);
	if ((l ^ nl) != 0xFFFFu) return ST_CORRUPT;
	b.at += 4;
	if (b.n - b.at < l) return ST_TRUNCATED;
	len = l;
	return ST_OK;
}
MCOM_DM_HD inline void stored_end(Bits &b, uint32_t len) { b.at += len; }

// ---- one token of a Huffman block ----
// written: bytes of this member that tokens before this one produce; room: bytes left in its slot behind them.  ST_OK: tok is a
// literal (its byte) or TOK_MATCH | (length - 3) << 16 | (distance - 1), nbytes what it produces.  ST_EOB: the block's end code.
MCOM_DM_HD inline int decode_token(Bits &b, const Tables &T, uint64_t written, uint64_t room, uint32_t &tok, uint32_t &nbytes)
{
	refill(b);                                                 // 15 + 5 + 15 + 13 bits at most: one refill serves the token
	uint32_t s = 0;
	int st = decode_sym(b, T.ll, T.ll_sym, T.ll_fast, LL_FAST, s);
	if (st) return st;
	if (s < 256) {
		if (room < 1) return ST_ROOM;
		tok = s; nbytes = 1;
		return ST_OK;
	}
	if (s == 256) return ST_EOB;
	if (s > 285) return ST_CORRUPT;
	const uint32_t xb = len_extra_bits(s);
	const uint32_t lbase = s < 265 ? s - 254 : s == 285 ? 258 : 3 + ((4 + ((s - 261) & 3)) << xb);
	if (b.bl < xb) return ST_TRUNCATED;
	const uint32_t len = lbase + take(b, xb);
	uint32_t ds = 0;
	st = decode_sym(b, T.d, T.d_sym, T.d_fast, D_FAST, ds);
	if (st) return st;
	if (ds >= 30) return ST_CORRUPT;
	const uint32_t dxb = dist_extra_bits(ds);
	const uint32_t dbase = ds < 4 ? ds + 1 : 1 + ((2 + (ds & 1)) << dxb);
	if (b.bl < dxb) return ST_TRUNCATED;
	const uint32_t dist = dbase + take(b, dxb);
	if (dist > written) return ST_CORRUPT;                     // in front of the member's own output
	if (len > room) return ST_ROOM;
	tok = (uint32_t)TOK_MATCH | ((len - 3) << 16) | (dist - 1);
	nbytes = len;
	return ST_OK;
}
MCOM_DM_HD inline bool tok_is_match(uint32_t tok) { return (tok & (uint32_t)TOK_MATCH) != 0; }
MCOM_DM_HD inline uint32_t tok_len(uint32_t tok) { return ((tok >> 16) & 255) + 3; }
MCOM_DM_HD inline uint32_t tok_dist(uint32_t tok) { return (tok & 0xFFFF) + 1; }

// Behind the last block: the payload must end with the byte the block ends in.
MCOM_DM_HD inline int stream_end(const Bits &b) { return b.at - (b.bl >> 3) == b.n ? ST_OK : ST_CORRUPT; }

// ---- CRC-32 of bytes at any address ----
MCOM_DM_HD inline uint32_t crc_bytes(const uint8_t *p, uint64_t n, const uint32_t *table)
{
	uint32_t c = 0xFFFFFFFFu;
	for (uint64_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 255] ^ (c >> 8);
	return ~c;
}

// ---- the whole member, one thread: the host twin's loop (the kernel spreads the same calls over a wave) ----
// pay[0 .. n): the DEFLATE payload; out[0 .. slot): the member's slot.  The status before the CRC-32 / ISIZE check; *written = bytes
// produced (all of them inside the slot).
MCOM_DM_HD inline int inflate_payload(const uint8_t *pay, uint64_t n, uint8_t *out, uint64_t slot, Tables &T, uint64_t *written)
{
	Bits b;
	bits_begin(b, pay, n);
	uint64_t w = 0;
	*written = 0;
	for (;;) {                                                 // every block takes its three header bits
		uint32_t last = 0, type = 0;
		int st = block_header(b, T, last, type);
		if (st) { *written = w; return st; }
		if (type == 0) {
			uint32_t len = 0;
			st = stored_begin(b, len);
			if (!st && len > slot - w) st = ST_ROOM;
			if (st) { *written = w; return st; }
			for (uint32_t i = 0; i < len; ++i) out[w + i] = b.p[b.at + i];
			stored_end(b, len);
			w += len;
		} else {
			st = block_codes(T);
			if (st) { *written = w; return st; }
			block_fast_clear(T, 0, 1);
			block_fast_fill(T, 0, 1);
			for (;;) {                                         // every token takes a bit
				uint32_t tok = 0, nb = 0;
				st = decode_token(b, T, w, slot - w, tok, nb);
				if (st == ST_EOB) break;
				if (st) { *written = w; return st; }
				if (!tok_is_match(tok)) out[w] = (uint8_t)tok;
				else {
					const uint32_t d = tok_dist(tok);
					for (uint32_t j = 0; j < nb; ++j) out[w + j] = out[w + j - d];
				}
				w += nb;
			}
		}
		if (last) break;
	}
	*written = w;
	return stream_end(b);
}

// ---- the walk over the members of a BGZF buffer (host code; the layout of Member is mcom_gzip_member's) ----
struct Member { uint64_t in_off, in_bytes, out_off; uint32_t isize, crc; };
inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t le32(const uint8_t *p) { return le16(p) | (le16(p + 2) << 16); }
// gzip headers that carry the `BC` subfield, header by header; further FEXTRA subfields, FNAME, FCOMMENT and FHCRC are skipped as RFC
// 1952 lays them out.  false at the first member without `BC`, with reserved flag bits, or of a size that leaves the buffer or is
// below header plus trailer; the three counts then describe the whole members in front of it.  members NULL: counts only; otherwise the
// walk ends (true) when cap members are filled.
inline bool walk_members(const uint8_t *file, uint64_t bytes, Member *members, uint64_t cap, uint64_t *n_members, uint64_t *text_bytes, uint64_t *used)
{
	uint64_t off = 0, count = 0, text = 0;
	bool ok = true;
	while (off < bytes) {                                          // every turn moves off forward by a member of at least 26 bytes, or stops
		const uint64_t rem = bytes - off;
		const uint8_t *h = file + off;
		ok = false;
		if (rem < 18 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8) break;
		const uint32_t flg = h[3];
		if ((flg & 0xE0) || !(flg & 4)) break;                     // reserved bits; no FEXTRA, so no BC field
		const uint64_t xend = 12 + (uint64_t)le16(h + 10);
		if (xend > rem) break;
		uint64_t q = 12, bsize = 0;
		while (q + 4 <= xend) {                                    // the subfields: SI1 SI2 LEN data
			const uint64_t sl = le16(h + q + 2);
			if (q + 4 + sl > xend) break;
			if (h[q] == 'B' && h[q + 1] == 'C' && sl == 2) { bsize = (uint64_t)le16(h + q + 4) + 1; break; }
			q += 4 + sl;
		}
		if (!bsize || bsize > rem) break;
		uint64_t p = xend;
		if (flg & 8) { while (p < bsize && h[p]) ++p; ++p; }       // FNAME
		if (flg & 16) { while (p < bsize && h[p]) ++p; ++p; }      // FCOMMENT
		if (flg & 2) p += 2;                                       // FHCRC
		if (p + 8 > bsize) break;
		ok = true;
		if (members && count == cap) break;                        // the table is full: *used says where the next call begins
		if (members) {
			Member &M = members[count];
			M.in_off = off + p; M.in_bytes = bsize - 8 - p; M.out_off = text;
			M.crc = le32(h + bsize - 8); M.isize = le32(h + bsize - 4);
		}
		text += le32(h + bsize - 4);
		++count; off += bsize;
	}
	*n_members = count; *text_bytes = text; *used = off;
	return ok;
}

// One member of a table against its buffers, all of it: the status the device call stores for it.
inline int inflate_member(const uint8_t *in, const Member &M, uint8_t *out, Tables &T, const uint32_t *crc_table)
{
	uint64_t w = 0;
	int st = inflate_payload(in + M.in_off, M.in_bytes, out + M.out_off, M.isize, T, &w);
	if (!st && w != M.isize) st = ST_CHECK;
	if (!st && crc_bytes(out + M.out_off, w, crc_table) != M.crc) st = ST_CHECK;
	return st;
}
// The extents of a table: every payload inside [0, in_bytes), every slot inside [0, out_bytes), slots in order and apart.  -1 = fine,
// otherwise the first member that is not.
inline int64_t check_table(const Member *tab, uint64_t n, uint64_t in_bytes, uint64_t out_bytes, int *why)
{
	uint64_t end = 0;
	for (uint64_t m = 0; m < n; ++m) {
		const Member &M = tab[m];
		if (M.in_off > in_bytes || M.in_bytes > in_bytes - M.in_off) { *why = 0; return (int64_t)m; }
		if (M.out_off > out_bytes || M.isize > out_bytes - M.out_off) { *why = 1; return (int64_t)m; }
		if (M.out_off < end) { *why = 2; return (int64_t)m; }
		end = M.out_off + M.isize;
	}
	return -1;
}

}  // namespace mcom_inflate_model
