// minicom_amd/csrc/rans_model.hpp -- the `.rans` member format: header, histograms -> normalised tables, their
// serialisation, the cost estimate and the model choice.  Plain host C++, header only, no HIP: the ONE copy that both routes use -- the
// host twin (host/mcom_entropy.cpp) and the host half of the device route (csrc/entropy.hip: histograms come down, tables go up) -- so
// that the two emit the same bytes and refuse the same members.
//
//   member  = header (32 bytes) | tables (table_bytes) | run lengths (n_seg x u16) | runs, back to back        (order-0, order-1)
//           = header (32 bytes) | raw bytes                                                                      (stored)
//   header  = "MCRS" | version u8 = 1 | model u8 | stride u8 | seg_log2 u8 | raw_len u64 | crc32 u32 | table_bytes u32 | payload_bytes u64
//   tables  = for plane 0 .. stride-1, for context 0 .. (order-1 ? 255 : 0):  n u16, then n x { symbol u8, freq u16 }, symbols ascending,
//             freq >= 1, sum = 4096; n = 0: the context does not occur
//   run     = the rANS state after the segment's FIRST symbol was coded last (u32, little endian), then the renormalisation bytes in the
//             order the decoder takes them
// All integers little endian.  Byte i of a segment belongs to plane i mod stride (segments are multiples of 4 bytes, so this is also
// its plane in the member); the order-1 context is byte i - stride of the same segment, 0 for the first `stride` bytes of a segment.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <math.h>
#include <vector>

namespace mcom_rans {

enum { STORED = 0, ORDER0 = 1, ORDER1 = 2 };
constexpr uint32_t PROB_BITS = 12, PROB_M = 1u << PROB_BITS;
constexpr uint32_t STATE_L = 1u << 23;                       // the state lives in [2^23, 2^31): byte-wise renormalisation
constexpr uint32_t SEG_LOG2 = 11, SEG = 1u << SEG_LOG2;      // what the encoders write; the decoders take 8 .. 15
constexpr uint32_t SEG_LOG2_MIN = 8, SEG_LOG2_MAX = 15;
constexpr size_t HEADER_BYTES = 32;
constexpr uint32_t ROW = 257;                                // a cumulative row: cum[0] = 0 .. cum[256] = 4096 (0: the context does not occur)
constexpr uint32_t N_PLANES_ALL = 7;                         // the planes of stride 1, 2, 4 side by side: 0 | 1 2 | 3 4 5 6
constexpr uint64_t RUN_OVERHEAD = 8;                         // bytes a run may take beyond its share of the model's bits, its u16 length included
// (derivation, DESIGN 3.6: a coding step grows the state by at most the factor M/f * (1 + 2^-11), 0.0007 bit per symbol and < 6 bits over a
// segment of 2^15 / < 1.5 bits over 2^11; renormalisation bytes <= (bits + 1.5) / 8 rounded up, + 4 bytes of state, + 2 of length < 8.)
static inline uint32_t plane_base(int stride) { return stride == 1 ? 0u : stride == 2 ? 1u : 3u; }
constexpr size_t run_cap(uint32_t seg) { return (size_t)seg * 3 / 2 + 8; }      // 12 bits per symbol at most, + state, + slack: < 2^16 for seg <= 2^15

// candidates in the order "simpler first" (ties of the estimate go to the earlier one)
struct Candidate { int model, stride; };
static const Candidate CANDIDATES[7] = {{STORED, 1}, {ORDER0, 1}, {ORDER0, 2}, {ORDER0, 4}, {ORDER1, 1}, {ORDER1, 2}, {ORDER1, 4}};
#define MCOM_RANS_HINT_OF(model, stride) (0x100 | ((model) << 4) | (stride))

struct Header {
	uint8_t model = 0, stride = 1, seg_log2 = SEG_LOG2;
	uint64_t raw_len = 0, payload_bytes = 0;
	uint32_t crc = 0, table_bytes = 0;
	uint64_t n_seg() const { return (raw_len + ((uint64_t)1 << seg_log2) - 1) >> seg_log2; }
};
static inline void put_u16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
static inline void put_u32(uint8_t *p, uint32_t v) { put_u16(p, v & 0xFFFF); put_u16(p + 2, v >> 16); }
static inline void put_u64(uint8_t *p, uint64_t v) { put_u32(p, (uint32_t)v); put_u32(p + 4, (uint32_t)(v >> 32)); }
static inline uint32_t get_u16(const uint8_t *p) { return p[0] | (uint32_t)p[1] << 8; }
static inline uint32_t get_u32(const uint8_t *p) { return get_u16(p) | get_u16(p + 2) << 16; }
static inline uint64_t get_u64(const uint8_t *p) { return get_u32(p) | (uint64_t)get_u32(p + 4) << 32; }

static inline void write_header(uint8_t *p, const Header &h)
{
	memcpy(p, "MCRS", 4); p[4] = 1; p[5] = h.model; p[6] = h.stride; p[7] = h.seg_log2;
	put_u64(p + 8, h.raw_len); put_u32(p + 16, h.crc); put_u32(p + 20, h.table_bytes); put_u64(p + 24, h.payload_bytes);
}
// Everything the header says about sizes, against the member's length: true only when the member is exactly as long as it says.
static inline bool read_header(const uint8_t *p, uint64_t len, Header &h)
{
	if (len < HEADER_BYTES || memcmp(p, "MCRS", 4) || p[4] != 1) return false;
	h.model = p[5]; h.stride = p[6]; h.seg_log2 = p[7];
	h.raw_len = get_u64(p + 8); h.crc = get_u32(p + 16); h.table_bytes = get_u32(p + 20); h.payload_bytes = get_u64(p + 24);
	if (h.model > ORDER1 || (h.stride != 1 && h.stride != 2 && h.stride != 4)) return false;
	if (h.seg_log2 < SEG_LOG2_MIN || h.seg_log2 > SEG_LOG2_MAX) return false;
	const uint64_t rest = len - HEADER_BYTES;
	if (h.model == STORED) return h.stride == 1 && h.table_bytes == 0 && h.payload_bytes == h.raw_len && rest == h.raw_len;
	if (h.raw_len > ((uint64_t)1 << 56)) return false;
	const uint64_t ns = h.n_seg();
	if (h.table_bytes > rest || 2 * ns > rest - h.table_bytes) return false;
	if (rest - h.table_bytes - 2 * ns < 4 * ns) return false;                      // (every run holds its state)
	return rest - h.table_bytes - 2 * ns == h.payload_bytes;
}

// ---- histograms: o1[plane of N_PLANES_ALL][context][symbol]; o0[i mod 4][symbol] -----------------------------------------------------
struct Hist {
	std::vector<uint64_t> o0, o1;
	Hist() : o0(4 * 256, 0), o1((size_t)N_PLANES_ALL * 65536, 0) {}
};
static inline void hist_host(const uint8_t *in, uint64_t n, Hist &h)
{
	for (uint64_t i = 0; i < n; ++i) {
		const uint32_t b = in[i], at = (uint32_t)(i & (SEG - 1));
		++h.o0[(i & 3) * 256 + b];
		const uint32_t c1 = at >= 1 ? in[i - 1] : 0, c2 = at >= 2 ? in[i - 2] : 0, c4 = at >= 4 ? in[i - 4] : 0;
		++h.o1[(size_t)0 * 65536 + c1 * 256 + b];
		++h.o1[(size_t)(1 + (i & 1)) * 65536 + c2 * 256 + b];
		++h.o1[(size_t)(3 + (i & 3)) * 65536 + c4 * 256 + b];
	}
}
// the counts of one (model, stride, plane, context) row
static inline void row_counts(const Hist &h, int model, int stride, int plane, int ctx, uint64_t cnt[256])
{
	if (model == ORDER1) { memcpy(cnt, &h.o1[((size_t)(plane_base(stride) + plane) * 256 + ctx) * 256], 256 * 8); return; }
	for (int s = 0; s < 256; ++s) { cnt[s] = 0; for (int q = plane; q < 4; q += stride) cnt[s] += h.o0[q * 256 + s]; }
}

// counts -> frequencies that add up to 4096, >= 1 for every symbol that occurs.  Deterministic: floor of the share, at least 1; what is
// missing goes to the most frequent symbol (lowest value on a tie); what is too much is taken, one at a time, from the symbol with the
// largest frequency (lowest value on a tie).
static inline bool normalise(const uint64_t cnt[256], uint16_t freq[256])
{
	uint64_t tot = 0;
	for (int s = 0; s < 256; ++s) tot += cnt[s];
	if (!tot) { memset(freq, 0, 512); return false; }
	uint32_t f[256], sum = 0; int best = 0;
	for (int s = 0; s < 256; ++s) {
		f[s] = 0;
		if (cnt[s]) { const unsigned __int128 q = ((unsigned __int128)cnt[s] << PROB_BITS) / tot; f[s] = q ? (uint32_t)q : 1u; }
		sum += f[s];
		if (cnt[s] > cnt[best]) best = s;
	}
	if (sum < PROB_M) f[best] += PROB_M - sum;
	while (sum > PROB_M) { int big = 0; for (int s = 1; s < 256; ++s) if (f[s] > f[big]) big = s; --f[big]; --sum; }
	for (int s = 0; s < 256; ++s) freq[s] = (uint16_t)f[s];
	return true;
}

// A model ready for coding: cum[(plane * n_ctx + ctx) * ROW + s], and its serialised form.
struct Model {
	int model = STORED, stride = 1;
	std::vector<uint16_t> cum;
	std::vector<uint8_t> ser;
	double bits = 0;                                         // sum over the member of -log2(f / 4096)
	int n_ctx() const { return model == ORDER1 ? 256 : 1; }
};
static inline void build_model(const Hist &h, int model, int stride, Model &m)
{
	m.model = model; m.stride = stride; m.bits = 0; m.ser.clear();
	m.cum.assign((size_t)stride * m.n_ctx() * ROW, 0);
	for (int pl = 0; pl < stride; ++pl)
		for (int c = 0; c < m.n_ctx(); ++c) {
			uint64_t cnt[256]; uint16_t f[256];
			row_counts(h, model, stride, pl, c, cnt);
			uint16_t *row = &m.cum[((size_t)pl * m.n_ctx() + c) * ROW];
			const size_t at = m.ser.size();
			m.ser.resize(at + 2);
			if (!normalise(cnt, f)) { put_u16(&m.ser[at], 0); continue; }
			uint32_t nsym = 0, run = 0;
			for (int s = 0; s < 256; ++s) {
				row[s] = (uint16_t)run; run += f[s];
				if (!f[s]) continue;
				++nsym;
				m.ser.push_back((uint8_t)s); m.ser.push_back((uint8_t)f[s]); m.ser.push_back((uint8_t)(f[s] >> 8));
				m.bits += (double)cnt[s] * log2((double)PROB_M / (double)f[s]);
			}
			row[256] = (uint16_t)run;
			put_u16(&m.ser[at], nsym);
		}
}
// the estimated size of the coded member: what the choice compares and what the coder stays under (RUN_OVERHEAD)
static inline uint64_t estimate(const Model &m, uint64_t n)
{
	const uint64_t n_seg = (n + SEG - 1) >> SEG_LOG2;
	return HEADER_BYTES + m.ser.size() + (uint64_t)ceil(m.bits / 8.0) + RUN_OVERHEAD * n_seg;
}
// hint 0: the candidate with the smallest estimate (est[7] filled when not null), otherwise the hinted one; false: no such hint
static inline bool choose(const Hist &h, uint64_t n, int hint, Model &out, uint64_t *est7)
{
	if (hint && !est7) {
		const int model = (hint >> 4) & 15, stride = hint & 15;
		if ((hint & ~0xFF) != 0x100 || model > ORDER1 || (stride != 1 && stride != 2 && stride != 4) || (model == STORED && stride != 1)) return false;
		out = Model(); out.model = model; out.stride = stride;
		if (model != STORED) build_model(h, model, stride, out);
		return true;
	}
	uint64_t best = HEADER_BYTES + n;
	out = Model();
	if (est7) est7[0] = best;
	for (int c = 1; c < 7; ++c) {
		Model m;
		build_model(h, CANDIDATES[c].model, CANDIDATES[c].stride, m);
		const uint64_t e = estimate(m, n);
		if (est7) est7[c] = e;
		if (e < best) { best = e; out.model = m.model; out.stride = m.stride; out.bits = m.bits; out.cum.swap(m.cum); out.ser.swap(m.ser); }
	}
	return true;
}

// serialised tables -> cumulative rows; false when they are not exactly `len` bytes of well-formed rows
static inline bool parse_tables(const uint8_t *p, size_t len, int model, int stride, std::vector<uint16_t> &cum)
{
	const int n_ctx = model == ORDER1 ? 256 : 1;
	cum.assign((size_t)stride * n_ctx * ROW, 0);
	size_t at = 0;
	for (int r = 0; r < stride * n_ctx; ++r) {
		if (len - at < 2) return false;
		const uint32_t nsym = get_u16(p + at); at += 2;
		if (nsym > 256 || (len - at) / 3 < nsym) return false;
		if (!nsym) continue;
		uint16_t f[256] = {0};
		int last = -1; uint32_t sum = 0;
		for (uint32_t q = 0; q < nsym; ++q, at += 3) {
			const int s = p[at]; const uint32_t fr = get_u16(p + at + 1);
			if (s <= last || fr < 1 || fr > PROB_M) return false;
			f[s] = (uint16_t)fr; sum += fr; last = s;
		}
		if (sum != PROB_M) return false;
		uint16_t *row = &cum[(size_t)r * ROW];
		uint32_t run = 0;
		for (int s = 0; s < 256; ++s) { row[s] = (uint16_t)run; run += f[s]; }
		row[256] = (uint16_t)run;
	}
	return at == len;
}

// ---- CRC-32 of a concatenation from the CRCs of its parts (the device makes one per segment) ----------------------------------------
static inline uint32_t gf2_times(const uint32_t *mat, uint32_t vec) { uint32_t s = 0; for (; vec; vec >>= 1, ++mat) if (vec & 1) s ^= *mat; return s; }
static inline void gf2_square(uint32_t *sq, const uint32_t *mat) { for (int n = 0; n < 32; ++n) sq[n] = gf2_times(mat, mat[n]); }
struct CrcShift {                                            // the operator "append `len` zero bytes" on a CRC register
	uint32_t op[32];
	explicit CrcShift(uint64_t len)
	{
		uint32_t sq[32], cur[32];
		for (int n = 0; n < 32; ++n) op[n] = 1u << n;                                   // identity
		cur[0] = 0xEDB88320u; for (int n = 1; n < 32; ++n) cur[n] = 1u << (n - 1);       // one zero BIT
		for (uint64_t bits = len * 8; bits; bits >>= 1) {
			if (bits & 1) { uint32_t t[32]; for (int n = 0; n < 32; ++n) t[n] = gf2_times(cur, op[n]); memcpy(op, t, sizeof t); }
			gf2_square(sq, cur); memcpy(cur, sq, sizeof sq);
		}
	}
	uint32_t join(uint32_t crc_a, uint32_t crc_b) const { return gf2_times(op, crc_a) ^ crc_b; }     // crc(A || B), |B| = len
};

}  // namespace mcom_rans
