// minicom_amd/csrc/qual_model.hpp -- the `.mcq` member format: quality values as a matrix of n_rows x L bytes
// under a static context model.  Header, alphabet, context rule, histograms -> tables (normalised by rans_model.hpp's rule), their
// serialisation, the estimate and the model choice.  Plain host C++, header only, no HIP: the ONE copy that the host twin
// (host/mcom_qual.cpp) and the host half of the device route (csrc/qual.hip) share, so that both emit the same bytes and refuse the
// same members.
//
//   member  = header (64 bytes) | tables (table_bytes) | run lengths (n_seg x u16) | runs, back to back       kind 0, model 1 .. 4
//           = header (64 bytes) | the n_rows * L raw bytes, row after row                                       kind 0, model 0 (stored)
//           = header (64 bytes) | a `.rans` member (section 3.6) of the n_rows * L raw bytes                    kind 1
//   header  = "MCQV" | version u8 = 1 | kind u8 | model u8 | payload_bytes u40 | crc32 of the raw bytes u32 | n_rows u64 | L u16 |
//             rows_per_seg u16 | table_bytes u32 | alphabet map, 32 bytes: bit (v & 7) of byte (v >> 3) is set when byte value v occurs
//   tables  = for context 0 .. n_ctx - 1:  n u16, then n x { symbol u8 (dense rank), freq u16 }, symbols ascending, freq >= 1,
//             sum = 4096; n = 0: the context does not occur
//   run     = as in section 3.6: the final state u32, then the renormalisation bytes in the order the decoder takes them
// All integers little endian.  A = the number of bits set in the map; the symbol of a byte is its rank among the values that occur.
// A segment is rows_per_seg consecutive rows (the last one what is left), its symbols row after row, coded last symbol first.
#pragma once
#include "rans_model.hpp"

namespace mcom_qual {

using mcom_rans::PROB_BITS; using mcom_rans::PROB_M; using mcom_rans::STATE_L; using mcom_rans::RUN_OVERHEAD;
using mcom_rans::put_u16; using mcom_rans::put_u32; using mcom_rans::put_u64; using mcom_rans::get_u16; using mcom_rans::get_u32; using mcom_rans::get_u64;

enum { KIND_MODEL = 0, KIND_RANS = 1 };
enum { Q_STORED = 0, Q_ORDER0 = 1, Q_P = 2, Q_PP = 3, Q_PMP = 4, Q_MODELS = 5 };
constexpr size_t QHEADER_BYTES = 64;
constexpr uint32_t L_MAX = 256, RPS_MAX = 4096, SEG_SYMBOLS_MAX = 32768;      // a run stays below 2^16 bytes: 1.5 x 32768 + 8
constexpr uint64_t RAW_MAX = (uint64_t)1 << 34;                               // n_rows * L, as the `.rans` coder's limit
constexpr int HINT_RANS = 0x180;                                              // hints: 0 = choose, 0x100 | id = that model, 0x180 = kind 1
#define MCOM_QUAL_HINT_OF(id) (0x100 | (id))

static inline uint32_t default_rps(uint32_t L) { return 2048 / L ? 2048 / L : 1; }
constexpr size_t qrun_cap(uint32_t seg_symbols) { return (((size_t)seg_symbols * 3 / 2 + 8) + 3) & ~(size_t)3; }

struct QHeader {
	uint8_t kind = KIND_MODEL, model = Q_STORED;
	uint64_t n_rows = 0, payload_bytes = 0;
	uint32_t L = 1, rps = 1, crc = 0, table_bytes = 0;
	uint8_t map[32] = {0};
	uint64_t raw_len() const { return n_rows * L; }
	uint64_t n_seg() const { return (n_rows + rps - 1) / rps; }
	uint32_t A() const { uint32_t a = 0; for (int v = 0; v < 256; ++v) a += (map[v >> 3] >> (v & 7)) & 1u; return a; }
};
static inline void write_qheader(uint8_t *p, const QHeader &h)
{
	memcpy(p, "MCQV", 4); p[4] = 1; p[5] = h.kind; p[6] = h.model;
	for (int k = 0; k < 5; ++k) p[7 + k] = (uint8_t)(h.payload_bytes >> (8 * k));
	put_u32(p + 12, h.crc); put_u64(p + 16, h.n_rows); put_u16(p + 24, h.L); put_u16(p + 26, h.rps); put_u32(p + 28, h.table_bytes);
	memcpy(p + 32, h.map, 32);
}
// the fields alone, from the first 64 bytes: magic, version and the ranges every member keeps
static inline bool read_qfields(const uint8_t *p, uint64_t len, QHeader &h)
{
	if (len < QHEADER_BYTES || memcmp(p, "MCQV", 4) || p[4] != 1) return false;
	h.kind = p[5]; h.model = p[6];
	h.payload_bytes = 0;
	for (int k = 0; k < 5; ++k) h.payload_bytes |= (uint64_t)p[7 + k] << (8 * k);
	h.crc = get_u32(p + 12); h.n_rows = get_u64(p + 16); h.L = get_u16(p + 24); h.rps = get_u16(p + 26); h.table_bytes = get_u32(p + 28);
	memcpy(h.map, p + 32, 32);
	if (h.kind > KIND_RANS || h.model >= Q_MODELS) return false;
	if (h.L < 1 || h.L > L_MAX || h.rps < 1 || h.rps > RPS_MAX || h.rps * h.L > SEG_SYMBOLS_MAX) return false;
	return h.n_rows < ((uint64_t)1 << 32) && h.n_rows * h.L <= RAW_MAX;
}
// Everything the header says about sizes, against the member's length: true only when the member is exactly as long as it says.
static inline bool read_qheader(const uint8_t *p, uint64_t len, QHeader &h)
{
	if (!read_qfields(p, len, h)) return false;
	const uint64_t rest = len - QHEADER_BYTES, raw = h.raw_len();
	if (h.kind == KIND_RANS) {
		if (h.model != Q_STORED || h.table_bytes != 0 || h.payload_bytes != rest) return false;
		for (int k = 0; k < 32; ++k) if (h.map[k]) return false;
		mcom_rans::Header rh;
		return mcom_rans::read_header(p + QHEADER_BYTES, rest, rh) && rh.raw_len == raw && rh.crc == h.crc;
	}
	if (h.model == Q_STORED) return h.table_bytes == 0 && h.payload_bytes == raw && rest == raw;
	if (h.n_rows == 0 || h.A() == 0) return false;
	const uint64_t ns = h.n_seg();
	if (h.table_bytes > rest || 2 * ns > rest - h.table_bytes) return false;
	if (rest - h.table_bytes - 2 * ns < 4 * ns) return false;                          // (every run holds its state)
	return rest - h.table_bytes - 2 * ns == h.payload_bytes;
}

// ---- the context rule ---------------------------------------------------------------------------------------------------------------
struct Geometry {
	uint32_t A = 0, Q = 0, L = 1;
	uint8_t rank[256], value[256], mbin[256];                // byte -> dense symbol | dense symbol -> byte | floor(Q * v / A)
	void set(const uint8_t map[32], uint32_t L_)
	{
		A = 0; L = L_;
		memset(rank, 0, 256); memset(value, 0, 256); memset(mbin, 0, 256);
		for (int v = 0; v < 256; ++v) if ((map[v >> 3] >> (v & 7)) & 1u) { rank[v] = (uint8_t)A; value[A] = (uint8_t)v; ++A; }
		Q = A < 8 ? A : 8;
		for (uint32_t v = 0; v < A; ++v) mbin[v] = (uint8_t)(Q * v / A);
	}
	uint32_t n_ctx(int id) const { return id == Q_ORDER0 ? 1u : id == Q_P ? A : id == Q_PP ? A * 8 : id == Q_PMP ? A * Q * 8 : 0u; }
	size_t hist_words() const { return (size_t)A * Q * 8 * A; }
	// the context of column j whose three predecessors in the row are p1 (j - 1), p2, p3 (dense; 0 in front of the row)
	uint32_t ctx(int id, uint32_t p1, uint32_t p2, uint32_t p3, uint32_t j) const
	{
		const uint32_t pos = 8 * j / L;
		switch (id) {
		case Q_P: return p1;
		case Q_PP: return p1 * 8 + pos;
		case Q_PMP: return (p1 * Q + mbin[p2 > p3 ? p2 : p3]) * 8 + pos;
		default: return 0;
		}
	}
};
static inline void map_host(const uint8_t *rows, uint64_t n_rows, uint32_t L, uint64_t pitch, uint8_t map[32])
{
	memset(map, 0, 32);
	for (uint64_t r = 0; r < n_rows; ++r) { const uint8_t *s = rows + r * pitch; for (uint32_t j = 0; j < L; ++j) map[s[j] >> 3] |= (uint8_t)(1u << (s[j] & 7)); }
}
// the counts of model 4, [context of model 4][symbol]: the other models' are sums of them
static inline void hist_host(const uint8_t *rows, uint64_t n_rows, uint64_t pitch, const Geometry &g, std::vector<uint64_t> &h4)
{
	h4.assign(g.hist_words(), 0);
	for (uint64_t r = 0; r < n_rows; ++r) {
		const uint8_t *s = rows + r * pitch;
		uint32_t p1 = 0, p2 = 0, p3 = 0;
		for (uint32_t j = 0; j < g.L; ++j) {
			const uint32_t sym = g.rank[s[j]];
			++h4[(size_t)g.ctx(Q_PMP, p1, p2, p3, j) * g.A + sym];
			p3 = p2; p2 = p1; p1 = sym;
		}
	}
}
// model 4's context c4 = (p1 * Q + m) * 8 + pos  ->  the context of model `id` it belongs to
static inline uint32_t fold_ctx(const Geometry &g, int id, uint32_t c4)
{
	const uint32_t pos = c4 & 7, p1 = (c4 >> 3) / g.Q;
	return id == Q_PMP ? c4 : id == Q_PP ? p1 * 8 + pos : id == Q_P ? p1 : 0u;
}

// A model ready for coding: cum[ctx * (A + 1) + s], and its serialised form.
struct QModel {
	int id = Q_STORED;
	std::vector<uint16_t> cum;
	std::vector<uint8_t> ser;
	double bits = 0;
};
static inline void build_model(const Geometry &g, const std::vector<uint64_t> &h4, int id, QModel &m)
{
	const uint32_t A = g.A, nc = g.n_ctx(id), nc4 = g.n_ctx(Q_PMP);
	std::vector<uint64_t> cnt((size_t)nc * A, 0);
	for (uint32_t c4 = 0; c4 < nc4; ++c4) { const size_t to = (size_t)fold_ctx(g, id, c4) * A, from = (size_t)c4 * A; for (uint32_t s = 0; s < A; ++s) cnt[to + s] += h4[from + s]; }
	m.id = id; m.bits = 0; m.ser.clear();
	m.cum.assign((size_t)nc * (A + 1), 0);
	for (uint32_t c = 0; c < nc; ++c) {
		uint64_t row_cnt[256] = {0}; uint16_t f[256];
		memcpy(row_cnt, &cnt[(size_t)c * A], (size_t)A * 8);
		uint16_t *row = &m.cum[(size_t)c * (A + 1)];
		const size_t at = m.ser.size();
		m.ser.resize(at + 2);
		if (!mcom_rans::normalise(row_cnt, f)) { put_u16(&m.ser[at], 0); continue; }
		uint32_t nsym = 0, run = 0;
		for (uint32_t s = 0; s < A; ++s) {
			row[s] = (uint16_t)run; run += f[s];
			if (!f[s]) continue;
			++nsym;
			m.ser.push_back((uint8_t)s); m.ser.push_back((uint8_t)f[s]); m.ser.push_back((uint8_t)(f[s] >> 8));
			m.bits += (double)row_cnt[s] * log2((double)PROB_M / (double)f[s]);
		}
		row[A] = (uint16_t)run;
		put_u16(&m.ser[at], nsym);
	}
}
static inline uint64_t estimate(const QModel &m, uint64_t n_seg) { return QHEADER_BYTES + m.ser.size() + (uint64_t)ceil(m.bits / 8.0) + RUN_OVERHEAD * n_seg; }
// hint 0: the model with the smallest estimate (est[5] filled when not null; ties go to the earlier id); 0x100 | id: that one.
// An empty matrix is always stored.  false: no such hint (HINT_RANS is the caller's business).
static inline bool choose(const Geometry &g, const std::vector<uint64_t> &h4, uint64_t n_rows, uint64_t n_seg, int hint, QModel &out, uint64_t *est5)
{
	out = QModel();
	if (hint && ((hint & ~0xFF) != 0x100 || (hint & 0xFF) >= Q_MODELS)) return false;
	uint64_t best = QHEADER_BYTES + n_rows * g.L;
	if (est5) { for (int k = 0; k < Q_MODELS; ++k) est5[k] = 0; est5[0] = best; }
	if (!n_rows) return true;
	if (hint) { if ((hint & 0xFF) != Q_STORED) build_model(g, h4, hint & 0xFF, out); return true; }
	for (int id = Q_ORDER0; id < Q_MODELS; ++id) {
		QModel m;
		build_model(g, h4, id, m);
		const uint64_t e = estimate(m, n_seg);
		if (est5) est5[id] = e;
		if (e < best) { best = e; out.id = id; out.bits = m.bits; out.cum.swap(m.cum); out.ser.swap(m.ser); }
	}
	return true;
}

// serialised tables -> cumulative rows of A + 1 entries; false when they are not exactly `len` bytes of well-formed rows
static inline bool parse_tables(const uint8_t *p, size_t len, const Geometry &g, int id, std::vector<uint16_t> &cum)
{
	const uint32_t A = g.A, nc = g.n_ctx(id);
	cum.assign((size_t)nc * (A + 1), 0);
	size_t at = 0;
	for (uint32_t r = 0; r < nc; ++r) {
		if (len - at < 2) return false;
		const uint32_t nsym = get_u16(p + at); at += 2;
		if (nsym > A || (len - at) / 3 < nsym) return false;
		if (!nsym) continue;
		uint16_t f[256] = {0};
		int last = -1; uint32_t sum = 0;
		for (uint32_t q = 0; q < nsym; ++q, at += 3) {
			const int s = p[at]; const uint32_t fr = get_u16(p + at + 1);
			if (s <= last || (uint32_t)s >= A || fr < 1 || fr > PROB_M) return false;
			f[s] = (uint16_t)fr; sum += fr; last = s;
		}
		if (sum != PROB_M) return false;
		uint16_t *row = &cum[(size_t)r * (A + 1)];
		uint32_t run = 0;
		for (uint32_t s = 0; s < A; ++s) { row[s] = (uint16_t)run; run += f[s]; }
		row[A] = (uint16_t)run;
	}
	return at == len;
}

// room that is enough for any hint: a table row exists per context (2 bytes) and an entry per (context, symbol) pair that occurs
static inline uint64_t bound(uint64_t n_rows, uint32_t L)
{
	if (L < 1 || L > L_MAX) return 0;
	const uint64_t raw = n_rows * L, rps = default_rps(L), n_seg = (n_rows + rps - 1) / rps;
	const uint64_t model = 2 * (uint64_t)256 * 8 * 8 + 3 * raw + n_seg * (2 + qrun_cap((uint32_t)(rps * L)));
	const uint64_t rans = mcom_rans::HEADER_BYTES + (uint64_t)4 * 256 * (2 + 3 * 256) + ((raw + mcom_rans::SEG - 1) >> mcom_rans::SEG_LOG2) * (2 + mcom_rans::run_cap(mcom_rans::SEG)) + 64;
	return QHEADER_BYTES + (model > rans ? model : rans) + 64;
}

}  // namespace mcom_qual
