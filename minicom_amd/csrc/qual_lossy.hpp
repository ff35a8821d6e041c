// minicom_amd/csrc/qual_lossy.hpp -- lossy quality values (`minicom -b SPEC`): the ONE statement of the spec
// text, the two named byte maps, the idempotence rule and the P-block walk.  csrc/qual_lossy.hip (the kernels) and
// host/mcom_qual_lossy.cpp (the host twin) both compile it, so the two cannot drift apart; tests/qual_lossy_reference.py states the
// same transform a second time, from the text of section 3.13, and shares nothing with this file.
//
//   ill8         Phred 2..9 -> 6, 10..19 -> 15, 20..24 -> 22, 25..29 -> 27, 30..34 -> 33, 35..39 -> 37, 40..93 -> 40 (Phred = byte - 33);
//                Phred 0 and 1 and every byte outside 33 .. 126 stay
//   thr:T:LO:HI  Phred < T -> LO, otherwise HI (0 <= T, LO, HI <= 93); other bytes stay.  Idempotent only with LO < T <= HI
//   pblock:P     1 <= P <= 47: greedy blocks of range <= 2 P along a row, every byte of a block becomes lo + floor((hi - lo) / 2)
// A byte map is accepted only when lut[lut[v]] == lut[v] for every v.  pblock is NOT idempotent (a second pass can join blocks).
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define MCOM_QL_HD __host__ __device__
#else
#define MCOM_QL_HD
#endif

namespace mcom_qlossy {

enum { K_ILL8 = 1, K_THR = 2, K_PBLOCK = 3, K_LUT = 4 };     // = MCOM_QUAL_LOSSY_* (include/mcom.h), MCOMH_QUAL_LOSSY_* (include/mcom_host.h)
enum { PHRED_MAX = 93, P_MAX = 47, SPEC_TEXT_MAX = 32 };

// layout of mcom_qual_lossy_spec / mcomh_qual_lossy_spec
struct Spec {
	uint32_t kind;
	uint32_t p[3];                                          // thr: T, LO, HI; pblock: P
	uint8_t lut[256];                                       // K_LUT: the map (the named maps are built from p)
};
// layout of mcom_qual_lossy_report / mcomh_qual_lossy_report
struct Report { uint64_t changed, sum_abs, sum_sq, max_abs; };

inline void build_ill8(uint8_t lut[256])
{
	for (int v = 0; v < 256; ++v) {
		int o = v;
		if (v >= 33 && v <= 126) {
			const int q = v - 33;
			const int b = q < 2 ? q : q < 10 ? 6 : q < 20 ? 15 : q < 25 ? 22 : q < 30 ? 27 : q < 35 ? 33 : q < 40 ? 37 : 40;
			o = b + 33;
		}
		lut[v] = (uint8_t)o;
	}
}
inline void build_thr(uint8_t lut[256], uint32_t T, uint32_t LO, uint32_t HI)
{
	for (int v = 0; v < 256; ++v) lut[v] = (uint8_t)(v >= 33 && v <= 126 ? ((uint32_t)(v - 33) < T ? LO : HI) + 33 : (uint32_t)v);
}
inline bool idempotent(const uint8_t lut[256])
{
	for (int v = 0; v < 256; ++v) if (lut[lut[v]] != lut[v]) return false;
	return true;
}

// Is the spec one the transform takes?  For a byte map `lut` gets the map to apply.
inline bool resolve(const Spec &s, uint8_t lut[256])
{
	if (s.kind == K_PBLOCK) return s.p[0] >= 1 && s.p[0] <= P_MAX;
	if (s.kind == K_ILL8) build_ill8(lut);
	else if (s.kind == K_THR) {
		if (s.p[0] > PHRED_MAX || s.p[1] > PHRED_MAX || s.p[2] > PHRED_MAX) return false;
		if (s.p[1] >= s.p[0] || s.p[2] < s.p[0]) return false;              // LO >= T or HI < T: not idempotent (T = 0, where LO is unused, falls under the rule as written)
		build_thr(lut, s.p[0], s.p[1], s.p[2]);
	}
	else if (s.kind == K_LUT) { for (int v = 0; v < 256; ++v) lut[v] = s.lut[v]; }
	else return false;
	return idempotent(lut);
}

// a decimal number without a sign or leading zeros, at most 3 digits; *at moves behind it
inline bool parse_number(const char *t, size_t &at, uint32_t &out)
{
	if (t[at] < '0' || t[at] > '9') return false;
	if (t[at] == '0' && t[at + 1] >= '0' && t[at + 1] <= '9') return false;
	uint32_t v = 0; int digits = 0;
	while (t[at] >= '0' && t[at] <= '9') { if (++digits > 3) return false; v = v * 10 + (uint32_t)(t[at] - '0'); ++at; }
	out = v;
	return true;
}
inline bool starts(const char *t, const char *w, size_t &at)
{
	size_t i = 0;
	for (; w[i]; ++i) if (t[i] != w[i]) return false;
	at = i;
	return true;
}
// The text of a spec (NUL-terminated, the canonical form only) -> Spec.  false: refused, *s untouched.
inline bool parse(const char *text, Spec &s)
{
	if (!text) return false;
	Spec n; n.kind = 0; n.p[0] = n.p[1] = n.p[2] = 0;
	for (int v = 0; v < 256; ++v) n.lut[v] = (uint8_t)v;
	size_t at = 0;
	if (starts(text, "ill8", at)) { if (text[at]) return false; n.kind = K_ILL8; }
	else if (starts(text, "thr:", at)) {
		if (!parse_number(text, at, n.p[0]) || text[at++] != ':' || !parse_number(text, at, n.p[1]) || text[at++] != ':' || !parse_number(text, at, n.p[2]) || text[at]) return false;
		n.kind = K_THR;
	} else if (starts(text, "pblock:", at)) {
		if (!parse_number(text, at, n.p[0]) || text[at]) return false;
		n.kind = K_PBLOCK;
	} else return false;
	uint8_t lut[256];
	if (!resolve(n, lut)) return false;
	if (n.kind != K_PBLOCK) for (int v = 0; v < 256; ++v) n.lut[v] = lut[v];
	s = n;
	return true;
}
inline size_t put_number(char *out, uint32_t v)
{
	char d[10]; size_t n = 0;
	do { d[n++] = (char)('0' + v % 10); v /= 10; } while (v);
	for (size_t i = 0; i < n; ++i) out[i] = d[n - 1 - i];
	return n;
}
// Spec -> its canonical text (NUL-terminated, at most SPEC_TEXT_MAX bytes with the NUL).  false: not a spec that has a text (a general
// map, a refused spec) or cap too small.
inline bool print(const Spec &s, char *out, size_t cap)
{
	uint8_t lut[256];
	if (!out || s.kind == K_LUT || !resolve(s, lut)) return false;
	char b[SPEC_TEXT_MAX]; size_t n = 0;
	const char *w = s.kind == K_ILL8 ? "ill8" : s.kind == K_THR ? "thr:" : "pblock:";
	for (; *w; ++w) b[n++] = *w;
	if (s.kind == K_THR) { n += put_number(b + n, s.p[0]); b[n++] = ':'; n += put_number(b + n, s.p[1]); b[n++] = ':'; n += put_number(b + n, s.p[2]); }
	if (s.kind == K_PBLOCK) n += put_number(b + n, s.p[0]);
	b[n++] = 0;
	if (n > cap) return false;
	for (size_t i = 0; i < n; ++i) out[i] = b[i];
	return true;
}

// what one row (or one thread's bytes) adds to the report: 32 bits are enough for 65536 bytes of a byte map, far more for a P-block row
struct RowStat {
	uint32_t changed = 0, sum_abs = 0, sum_sq = 0, max_abs = 0;
	MCOM_QL_HD inline void add(uint32_t from, uint32_t to)
	{
		const uint32_t d = from > to ? from - to : to - from;
		changed += d != 0; sum_abs += d; sum_sq += d * d; max_abs = d > max_abs ? d : max_abs;
	}
};

// The P-block walk over one row of L >= 1 bytes, in place.  A block starts at column s with lo = hi = q[s]; column j joins while
// max - min over [s, j] stays <= 2 P; otherwise [s, j) is closed -- every byte becomes lo + floor((hi - lo) / 2) -- and j starts the next
// block; the last block closes at L.  Written as ONE loop of exactly 2 L steps, each of which either looks at the next column or rewrites
// one byte of the block just closed: the lanes of a wave, one row each, then stay in step whatever their rows hold (a nested fill loop
// would make every lane wait for every other lane's blocks).  The walk never looks at a byte it has rewritten: it pauses while a block
// is filled, and the fill ends in front of the column the walk has reached.
MCOM_QL_HD inline void pblock_row(uint8_t *q, uint32_t L, uint32_t P, RowStat &st)
{
	uint32_t lo = q[0], hi = lo;
	uint32_t j = 1, s = 0, f = 0, end = 0, m = 0;
	bool fill = false;
	for (uint32_t it = 0; it < 2 * L; ++it) {
		if (fill) {
			st.add(q[f], m);
			q[f] = (uint8_t)m;
			if (++f == end) fill = false;
		} else if (j < L) {
			const uint32_t v = q[j], nlo = v < lo ? v : lo, nhi = v > hi ? v : hi;
			if (nhi - nlo <= 2 * P) { lo = nlo; hi = nhi; }
			else { m = lo + ((hi - lo) >> 1); f = s; end = j; fill = true; s = j; lo = hi = v; }
			++j;
		} else if (s < L) { m = lo + ((hi - lo) >> 1); f = s; end = L; fill = true; s = L; }
	}
}

}  // namespace mcom_qlossy
