// minicom_amd/csrc/name_model.hpp -- the `.mcn` member format: read names and the text of the third FASTQ line.
// Header, token rule, op rule, the walk that rebuilds a record from the streams, and the checks that need no decoding.  Header only,
// no HIP call: the ONE copy that the host twin (host/mcom_names.cpp) and the device route (csrc/names.hip) share -- the token rule, the
// op rule and the record walk are the same functions on the host and inside the kernels (MCOM_NM_HD), so that both emit the same bytes
// and refuse the same members.
//
//   name text = for record 0, 1, ..: line 1 without its '@', '\n', line 3 without its '+', '\n'          (2 n lines, any byte but '\n')
//   member    = header (96 bytes) | ops | delta | num | tlen | text | plus | ptext      kind 0: each a `.bwt` member (section 3.8) of
//                                                                                       that stream, or nothing where the stream is empty
//             = header (96 bytes) | the `.rans` member (section 3.6, hint 0) of the name text             kind 1
//   header    = "MCNM" | version u8 = 1 | kind u8 | token cap u8 = 24 | 0 u8 | n_records u64 | text_len u64 | crc32 of the name text u32 |
//               recs_per_seg u16 | 0 u16 | the seven member lengths, u64 each (kind 1: all 0) | 0 u64
//   tokens    a name is cut into maximal runs of ASCII digits and maximal runs of other bytes; a digit run of at most 9 digits without a
//             leading '0' (the single digit "0" is one) is NUMERIC, every other run is TEXT; at most 24 tokens: tokens 0 .. 22 by that
//             rule, token 23 the whole rest as TEXT
//   ops       per record one byte per token, then END; token t against token t (as coded) of the record before, the first record of a
//             segment of recs_per_seg records against a record without tokens; the first that applies of
//               0 MATCH (same class, same bytes) | 1 INC (numeric, previous + 1) | 2 DELTA (numeric, previous + d, 2 <= d <= 255: d -> delta)
//               | 3 NUM (the value, u32 -> num) | 4 TEXT (length u8 -> tlen, bytes -> text) | 5 END
//   plus      per record: 0 the third line is a bare '+' | 1 its text equals the name | 2 a literal
//   ptext     the lengths (u8) of all literals, record after record, then their bytes, literal after literal
//   kind 2     the name text of the second file of a pair, coded against the first file's name text, its MATE:
//             the seven streams and the op bytes of kind 0, but token t of record r is coded against token t of the mate's line 2 r cut
//             by the token rule (never against the record before: recs_per_seg = 1), and a MATCH of a text token takes its bytes from
//             the mate text.  Offset 88 holds the crc32 of the mate text (u32), then 0 u32; n_records is the mate's.  Only a reader that
//             is handed the mate (read_nheader(.., true), walk_record_mate) takes kind 2; every other one refuses it as before.
// All integers little endian.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "rans_model.hpp"
#include "bwt_model.hpp"

#if defined(__HIP__)
#define MCOM_NM_HD __host__ __device__
#else
#define MCOM_NM_HD
#endif

namespace mcom_name {

using mcom_rans::put_u16; using mcom_rans::put_u32; using mcom_rans::put_u64; using mcom_rans::get_u16; using mcom_rans::get_u32; using mcom_rans::get_u64;

enum { KIND_STREAMS = 0, KIND_RANS = 1, KIND_MATE = 2 };
enum { S_OPS = 0, S_DELTA, S_NUM, S_TLEN, S_TEXT, S_PLUS, S_PTEXT, N_STREAMS };
enum { OP_MATCH = 0, OP_INC, OP_DELTA, OP_NUM, OP_TEXT, OP_END };
enum { PLUS_BARE = 0, PLUS_NAME = 1, PLUS_LITERAL = 2 };
// what a walk or a check raises (the device's flag word; the host twin refuses on any of them)
enum { NM_F_OP = 1,        // an op above 5, a plus byte above 2
       NM_F_PREV = 2,      // MATCH / INC / DELTA without a previous token t, or on the wrong class
       NM_F_VALUE = 4,     // a numeric value that reaches 10^9
       NM_F_TOKENS = 8,    // a 25th token
       NM_F_LONG = 16,     // a name or '+' text above 255 bytes
       NM_F_NL = 32,       // a '\n' inside a text token or a literal
       NM_F_RUN = 64,      // a stream read beyond its end (cannot be once the counts agree)
       NM_F_LINES = 128,   // encoder: the name text is not 2 n complete lines
       NM_F_MATE = 256 };  // kind 2: the mate text is not the 2 n lines (of at most 255 bytes) the member was coded against
constexpr size_t NHEADER_BYTES = 96;
constexpr uint32_t TOKEN_CAP = 24, NM_NAME_MAX = 255, RPS = 256, RPS_MAX = 4096, VALUE_END = 1000000000u, NUMERIC = 0xFFFFFFFFu;
constexpr uint64_t N_MAX = 0xFFFFFFFFull / (TOKEN_CAP + 1);        // the ops of n records stay below 4 GiB whatever the names: 171 798 691
constexpr uint64_t TEXT_MAX = mcom_bwt::RAW_MAX;                   // a stream is one `.bwt` member

struct NHeader {
	uint8_t kind = KIND_STREAMS;
	uint64_t n_records = 0, text_len = 0;
	uint32_t crc = 0, rps = RPS, mate_crc = 0;                  // mate_crc: kind 2 alone
	uint64_t len[N_STREAMS] = {0, 0, 0, 0, 0, 0, 0};
	uint64_t n_seg() const { return (n_records + rps - 1) / rps; }
	uint64_t streams_bytes() const { uint64_t s = 0; for (int k = 0; k < N_STREAMS; ++k) s += len[k]; return s; }
};
static inline void write_nheader(uint8_t *p, const NHeader &h)
{
	memcpy(p, "MCNM", 4); p[4] = 1; p[5] = h.kind; p[6] = (uint8_t)TOKEN_CAP; p[7] = 0;
	put_u64(p + 8, h.n_records); put_u64(p + 16, h.text_len); put_u32(p + 24, h.crc); put_u16(p + 28, h.rps); put_u16(p + 30, 0);
	for (int k = 0; k < N_STREAMS; ++k) put_u64(p + 32 + 8 * k, h.len[k]);
	put_u32(p + 88, h.kind == KIND_MATE ? h.mate_crc : 0); put_u32(p + 92, 0);
}
// the fields alone, from the first 96 bytes: magic, version and the ranges every member keeps.  mate: the reader holds a mate text, so
// kind 2 is taken as well (recs_per_seg 1, the mate's crc at offset 88)
static inline bool read_nfields(const uint8_t *p, uint64_t len, NHeader &h, bool mate = false)
{
	if (len < NHEADER_BYTES || memcmp(p, "MCNM", 4) || p[4] != 1) return false;
	h.kind = p[5];
	h.n_records = get_u64(p + 8); h.text_len = get_u64(p + 16); h.crc = get_u32(p + 24); h.rps = get_u16(p + 28);
	for (int k = 0; k < N_STREAMS; ++k) h.len[k] = get_u64(p + 32 + 8 * k);
	if (h.kind > (mate ? KIND_MATE : KIND_RANS) || p[6] != TOKEN_CAP || p[7] != 0 || get_u16(p + 30) != 0 || get_u32(p + 92) != 0) return false;
	h.mate_crc = get_u32(p + 88);
	if (h.kind == KIND_MATE ? h.rps != 1 : h.mate_crc != 0) return false;
	if (h.rps < 1 || h.rps > RPS_MAX || h.n_records > N_MAX || h.text_len > TEXT_MAX) return false;
	return h.text_len >= 2 * h.n_records && h.text_len <= 2 * (uint64_t)(NM_NAME_MAX + 1) * h.n_records;
}
// Everything the header says about sizes, against the member's length: true only when the member is exactly as long as it says.
static inline bool read_nheader(const uint8_t *p, uint64_t len, NHeader &h, bool mate = false)
{
	if (!read_nfields(p, len, h, mate)) return false;
	const uint64_t rest = len - NHEADER_BYTES;
	if (h.kind == KIND_RANS) {
		if (h.n_records == 0 || h.streams_bytes() != 0) return false;
		mcom_rans::Header rh;
		return mcom_rans::read_header(p + NHEADER_BYTES, rest, rh) && rh.raw_len == h.text_len && rh.crc == h.crc;
	}
	uint64_t sum = 0;
	for (int k = 0; k < N_STREAMS; ++k) {
		if (h.len[k] > rest - sum) return false;
		if (h.len[k] && h.len[k] < mcom_bwt::HEADER_BYTES + mcom_rans::HEADER_BYTES) return false;
		sum += h.len[k];
	}
	return sum == rest;
}
// The raw lengths the seven embedded members state (0: no member), against the header's counts: what can be told before a stream is decoded.
static inline bool check_raw_lens(const NHeader &h, const uint64_t raw[N_STREAMS])
{
	const uint64_t n = h.n_records;
	for (int k = 0; k < N_STREAMS; ++k) if ((raw[k] == 0) != (h.len[k] == 0)) return false;      // (an empty stream has no member, a member is not empty)
	if (raw[S_PLUS] != n || raw[S_OPS] < n || raw[S_OPS] > (TOKEN_CAP + 1) * n) return false;
	const uint64_t tokens = raw[S_OPS] - n;
	if (raw[S_NUM] & 3) return false;
	if (raw[S_DELTA] > tokens || raw[S_NUM] / 4 > tokens || raw[S_TLEN] > tokens || raw[S_DELTA] + raw[S_NUM] / 4 + raw[S_TLEN] > tokens) return false;
	return raw[S_TEXT] <= h.text_len - 2 * n && raw[S_PTEXT] <= h.text_len - n;
}
// one embedded `.bwt` member's header (its first 40 bytes) against the length the `.mcn` header gives it
static inline bool embedded_raw_len(const uint8_t *bwt_head, uint64_t member_len, uint64_t &raw)
{
	mcom_bwt::Header bh;
	if (!mcom_bwt::read_header(bwt_head, member_len, bh)) return false;
	raw = bh.raw_len;
	return true;
}
// room that is enough: the member is never larger than its header and the `.rans` member (hint 0: at most 32 + n) of the text
static inline uint64_t bound(uint64_t text_len) { return NHEADER_BYTES + mcom_rans::HEADER_BYTES + text_len + 64; }

// ---- the token rule ---------------------------------------------------------------------------------------------------------------------
struct Tok { uint32_t at, len, val; bool num; };
MCOM_NM_HD static inline bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
MCOM_NM_HD static inline uint32_t n_digits(uint32_t v)
{
	uint32_t d = 1;
	for (uint32_t p = 10; d < 10 && v >= p; p *= 10) ++d;         // (v < 10^9: at most 9)
	return d;
}
MCOM_NM_HD static inline void put_digits(uint8_t *o, uint32_t v, uint32_t nd) { for (uint32_t k = nd; k-- > 0; v /= 10) o[k] = (uint8_t)('0' + v % 10); }
// token t of the name s[0 .. len) that starts at `pos`; false at the end of the name
MCOM_NM_HD static inline bool next_token(const uint8_t *s, uint32_t len, uint32_t &pos, uint32_t t, Tok &k)
{
	if (pos >= len) return false;
	k.at = pos; k.val = 0; k.num = false;
	if (t + 1 >= TOKEN_CAP) { k.len = len - pos; pos = len; return true; }
	const bool d = is_digit(s[pos]);
	uint32_t e = pos + 1;
	while (e < len && is_digit(s[e]) == d) ++e;
	k.len = e - pos;
	if (d && k.len <= 9 && (s[pos] != '0' || k.len == 1)) {
		k.num = true;
		for (uint32_t j = pos; j < e; ++j) k.val = k.val * 10 + (uint32_t)(s[j] - '0');
	}
	pos = e;
	return true;
}
MCOM_NM_HD static inline bool same_bytes(const uint8_t *a, const uint8_t *b, uint32_t n) { for (uint32_t j = 0; j < n; ++j) if (a[j] != b[j]) return false; return true; }

// ---- the op rule: one record against the one before it (plen tokens of prv count only when !first) ---------------------------------------
// Sink: op(u8), delta(u8), num(u32), text(bytes, len) [the length goes to tlen, the bytes to text], plus(u8), literal(bytes, len).
// Returns the record's plus kind, so that a caller that only counts need not take the literal's length through its sink.
template <class Sink>
MCOM_NM_HD static inline uint32_t code_record(const uint8_t *cur, uint32_t clen, const uint8_t *prv, uint32_t plen, bool first,
                                          const uint8_t *pl, uint32_t pl_len, Sink &s)
{
	uint32_t cpos = 0, ppos = 0;
	Tok c, p;
	bool have_p = !first;
	for (uint32_t t = 0; next_token(cur, clen, cpos, t, c); ++t) {
		have_p = have_p && next_token(prv, plen, ppos, t, p);
		if (have_p && c.num == p.num && (c.num ? c.val == p.val : c.len == p.len && same_bytes(cur + c.at, prv + p.at, c.len))) s.op(OP_MATCH);
		else if (have_p && c.num && p.num && c.val == p.val + 1) s.op(OP_INC);
		else if (have_p && c.num && p.num && c.val > p.val && c.val - p.val <= 255) { s.op(OP_DELTA); s.delta((uint8_t)(c.val - p.val)); }
		else if (c.num) { s.op(OP_NUM); s.num(c.val); }
		else { s.op(OP_TEXT); s.text(cur + c.at, c.len); }
	}
	s.op(OP_END);
	const uint32_t kind = pl_len == 0 ? (uint32_t)PLUS_BARE : pl_len == clen && same_bytes(pl, cur, clen) ? (uint32_t)PLUS_NAME : (uint32_t)PLUS_LITERAL;
	s.plus(kind);
	if (kind == PLUS_LITERAL) s.literal(pl, pl_len);
	return kind;
}

// ---- the record walk: the decoder's one step ---------------------------------------------------------------------------------------------
struct View {                                                // the five streams a name is made of; n_num counts values, not bytes
	const uint8_t *ops, *delta, *num, *tlen, *text;
	uint64_t n_ops, n_delta, n_num, n_tlen, n_text;
};
struct Cursor { uint64_t op = 0, delta = 0, num = 0, tlen = 0, text = 0; };
// Tab: val(t), len(t) -> uint32_t&: the tokens of the record before as coded -- len = NUMERIC and val the value, or len the length of a
// text token and val its offset in `text`; n_prev of them stand.  out: the name's bytes (NULL: lengths only), room <= NM_NAME_MAX: the bytes a
// name may have here.  Returns 0 or NM_F_* bits; a refused record has read nothing outside the streams and written at most `room` bytes.  At most TOKEN_CAP + 1 steps.
template <class Tab>
MCOM_NM_HD static inline uint32_t walk_record(const View &v, Cursor &c, Tab &tab, uint32_t &n_prev, uint8_t *out, uint32_t room, uint32_t &name_len)
{
	uint32_t nl = 0, t = 0;
	for (uint32_t step = 0; step <= TOKEN_CAP; ++step) {
		if (c.op >= v.n_ops) return NM_F_RUN;
		const uint32_t op = v.ops[c.op++];
		if (op == OP_END) { n_prev = t; name_len = nl; return 0; }
		if (op > OP_END) return NM_F_OP;
		if (step == TOKEN_CAP) return NM_F_TOKENS;
		uint32_t val = 0, len = NUMERIC;
		if (op <= OP_DELTA) {
			if (t >= n_prev) return NM_F_PREV;
			val = tab.val(t); len = tab.len(t);
			if (op != OP_MATCH) {
				if (len != NUMERIC) return NM_F_PREV;
				uint32_t d = 1;
				if (op == OP_DELTA) { if (c.delta >= v.n_delta) return NM_F_RUN; d = v.delta[c.delta++]; }
				val += d;                                              // (val < 10^9, d <= 255)
			}
		} else if (op == OP_NUM) {
			if (c.num >= v.n_num) return NM_F_RUN;
			{ const uint8_t *q = v.num + 4 * c.num++; val = q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24; }
		} else {
			if (c.tlen >= v.n_tlen) return NM_F_RUN;
			len = v.tlen[c.tlen++];
			if (len > v.n_text - c.text) return NM_F_RUN;
			val = (uint32_t)c.text; c.text += len;
		}
		if (len == NUMERIC && val >= VALUE_END) return NM_F_VALUE;
		const uint32_t bytes = len == NUMERIC ? n_digits(val) : len;
		if (nl + bytes > room) return NM_F_LONG;
		if (out) {
			if (len == NUMERIC) put_digits(out + nl, val, bytes);
			else for (uint32_t j = 0; j < bytes; ++j) out[nl + j] = v.text[(uint64_t)val + j];
		}
		tab.val(t) = val; tab.len(t) = len;
		nl += bytes; ++t;
	}
	return NM_F_TOKENS;                                          // (not reached: step TOKEN_CAP returns)
}

// The same step for kind 2: the tokens of the mate's name m[0 .. mlen) stand where the record before stood.  They are cut by the token
// rule as the walk goes (token t only ever looks at mate token t), so nothing is kept between records and a lane can take any record.
// A MATCH of a text token copies the mate's bytes.  Reads nothing outside the streams and m[0 .. mlen); writes at most `room` bytes.
MCOM_NM_HD static inline uint32_t walk_record_mate(const View &v, Cursor &c, const uint8_t *m, uint32_t mlen, uint8_t *out, uint32_t room, uint32_t &name_len)
{
	uint32_t nl = 0, mpos = 0;
	bool have_m = true;
	Tok k;
	for (uint32_t step = 0; step <= TOKEN_CAP; ++step) {
		if (c.op >= v.n_ops) return NM_F_RUN;
		const uint32_t op = v.ops[c.op++];
		if (op == OP_END) { name_len = nl; return 0; }
		if (op > OP_END) return NM_F_OP;
		if (step == TOKEN_CAP) return NM_F_TOKENS;
		have_m = have_m && next_token(m, mlen, mpos, step, k);
		uint32_t val = 0, len = NUMERIC;
		const uint8_t *src = v.text;
		if (op <= OP_DELTA) {
			if (!have_m) return NM_F_PREV;
			if (op == OP_MATCH) { if (k.num) val = k.val; else { len = k.len; val = k.at; src = m; } }
			else {
				if (!k.num) return NM_F_PREV;
				uint32_t d = 1;
				if (op == OP_DELTA) { if (c.delta >= v.n_delta) return NM_F_RUN; d = v.delta[c.delta++]; }
				val = k.val + d;                                       // (k.val < 10^9, d <= 255)
			}
		} else if (op == OP_NUM) {
			if (c.num >= v.n_num) return NM_F_RUN;
			{ const uint8_t *q = v.num + 4 * c.num++; val = q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24; }
		} else {
			if (c.tlen >= v.n_tlen) return NM_F_RUN;
			len = v.tlen[c.tlen++];
			if (len > v.n_text - c.text) return NM_F_RUN;
			val = (uint32_t)c.text; c.text += len;
		}
		if (len == NUMERIC && val >= VALUE_END) return NM_F_VALUE;
		const uint32_t bytes = len == NUMERIC ? n_digits(val) : len;
		if (nl + bytes > room) return NM_F_LONG;
		if (out) {
			if (len == NUMERIC) put_digits(out + nl, val, bytes);
			else for (uint32_t j = 0; j < bytes; ++j) out[nl + j] = src[(uint64_t)val + j];
		}
		nl += bytes;
	}
	return NM_F_TOKENS;                                          // (not reached: step TOKEN_CAP returns)
}

}  // namespace mcom_name
