// minicom_amd/host/mcom_qual.cpp -- the quality-value coder on the host: the twin of csrc/qual.hip and its specification
// (DESIGN.md section 3.9).  Plain C++ on host buffers -- no GPU, no HIP call: the same alphabet, counts, normalisation, choice and
// serialisation (csrc/qual_model.hpp), the same coder step as the `.rans` coder, so the bytes equal the device's and the same
// members are refused.  Builds alone beside mcom_entropy.cpp (tests/fuzz_qual.cpp runs it under the sanitizers).
#include "../../include/mcom_host.h"
#include "../csrc/qual_model.hpp"
#include "mcom_inflate.hpp"
#include <cstring>
#include <new>
#include <vector>

using namespace mcom_qual;

namespace {

inline void code_symbol(uint32_t &x, uint8_t *&wp, const uint16_t *row, uint32_t sym)
{
	const uint32_t c = row[sym], f = row[sym + 1] - c;
	const uint32_t x_max = f << 19;
	while (x >= x_max) { *--wp = (uint8_t)x; x >>= 8; }
	x = ((x / f) << PROB_BITS) + (x % f) + c;
}

uint32_t crc_rows(const uint8_t *rows, uint64_t n_rows, uint32_t L, uint64_t pitch)
{
	uint32_t crc = 0;
	if (pitch == L) return n_rows ? mcom_crc32(0, rows, n_rows * L) : 0;
	for (uint64_t r = 0; r < n_rows; ++r) crc = mcom_crc32(crc, rows + r * pitch, L);
	return crc;
}

int encode(const uint8_t *rows, uint64_t n_rows, uint32_t L, uint64_t pitch, uint8_t *out, uint64_t cap, uint64_t *out_len, int hint)
{
	if (!out_len || !out || (n_rows && !rows)) return -1;
	*out_len = 0;
	if (L < 1 || L > L_MAX || pitch < L || n_rows >= ((uint64_t)1 << 32) || n_rows * L > RAW_MAX) return -1;
	if (cap < QHEADER_BYTES) return -4;
	const uint64_t raw = n_rows * L;
	QHeader hd; hd.n_rows = n_rows; hd.L = L; hd.rps = default_rps(L); hd.crc = crc_rows(rows, n_rows, L, pitch);
	const uint64_t n_seg = hd.n_seg();
	// kind 1: the `.rans` member of the flat bytes
	std::vector<uint8_t> rans;
	if (hint == 0 || hint == HINT_RANS) {
		std::vector<uint8_t> flat;
		const uint8_t *src = rows;
		if (pitch != L) { flat.resize(raw); for (uint64_t r = 0; r < n_rows; ++r) memcpy(&flat[r * L], rows + r * pitch, L); src = flat.data(); }
		rans.resize(mcom_rans::HEADER_BYTES + raw);
		uint64_t got = 0;
		if (mcomh_rans_encode(src, raw, rans.data(), rans.size(), &got, 0)) return -1;
		rans.resize(got);
	}
	QModel m;
	uint64_t total = 0;
	std::vector<uint8_t> body;                                  // tables | run lengths | runs
	Geometry g;
	if (hint != HINT_RANS) {
		map_host(rows, n_rows, L, pitch, hd.map);
		g.set(hd.map, L);
		std::vector<uint64_t> h4;
		hist_host(rows, n_rows, pitch, g, h4);
		if (!choose(g, h4, n_rows, n_seg, hint, m, nullptr)) return -1;
		hd.model = (uint8_t)m.id;
		if (m.id == Q_STORED) total = QHEADER_BYTES + raw;
		else {
			body.assign(m.ser.begin(), m.ser.end());
			body.resize(m.ser.size() + 2 * n_seg);
			std::vector<uint8_t> scratch(qrun_cap(hd.rps * L));
			const uint32_t A = g.A;
			for (uint64_t seg = 0; seg < n_seg; ++seg) {
				const uint64_t r0 = seg * hd.rps, r1 = r0 + hd.rps < n_rows ? r0 + hd.rps : n_rows;
				uint8_t *const top = scratch.data() + scratch.size(), *wp = top;
				uint32_t x = STATE_L;
				for (uint64_t r = r1; r-- > r0; ) {
					const uint8_t *s = rows + r * pitch;
					for (uint32_t j = L; j-- > 0; ) {
						const uint32_t p1 = j >= 1 ? g.rank[s[j - 1]] : 0u, p2 = j >= 2 ? g.rank[s[j - 2]] : 0u, p3 = j >= 3 ? g.rank[s[j - 3]] : 0u;
						code_symbol(x, wp, &m.cum[(size_t)g.ctx(m.id, p1, p2, p3, j) * (A + 1)], g.rank[s[j]]);
					}
				}
				*--wp = (uint8_t)(x >> 24); *--wp = (uint8_t)(x >> 16); *--wp = (uint8_t)(x >> 8); *--wp = (uint8_t)x;
				const size_t rl = (size_t)(top - wp);
				put_u16(&body[m.ser.size() + 2 * seg], (uint32_t)rl);
				body.insert(body.end(), wp, top);
			}
			hd.table_bytes = (uint32_t)m.ser.size();
			hd.payload_bytes = body.size() - m.ser.size() - 2 * n_seg;
			total = QHEADER_BYTES + body.size();
		}
	}
	if (hint == HINT_RANS || (hint == 0 && QHEADER_BYTES + rans.size() < total)) {
		QHeader rh; rh.kind = KIND_RANS; rh.n_rows = n_rows; rh.L = L; rh.rps = hd.rps; rh.crc = hd.crc; rh.payload_bytes = rans.size();
		if (cap < QHEADER_BYTES + rans.size()) return -4;
		write_qheader(out, rh);
		memcpy(out + QHEADER_BYTES, rans.data(), rans.size());
		*out_len = QHEADER_BYTES + rans.size();
		return 0;
	}
	if (cap < total) return -4;
	if (m.id == Q_STORED) {
		hd.payload_bytes = raw;
		write_qheader(out, hd);
		for (uint64_t r = 0; r < n_rows; ++r) memcpy(out + QHEADER_BYTES + r * L, rows + r * pitch, L);
	} else {
		write_qheader(out, hd);
		memcpy(out + QHEADER_BYTES, body.data(), body.size());
	}
	*out_len = total;
	return 0;
}

// One segment of the coded form: its run of rl bytes at p, n rows to dst, `pitch` apart.  false: the run is shorter than a state, the
// state leaves [2^23, 2^31), a slot no symbol owns, a symbol >= A, the run read beyond its end or not used up exactly.
bool decode_segment(const QHeader &hd, const Geometry &g, const std::vector<uint16_t> &cum, const uint8_t *p, uint32_t rl, uint64_t n, uint8_t *dst, uint64_t pitch)
{
	const uint32_t A = g.A, L = hd.L;
	const uint8_t *const end = p + rl;
	if (rl < 4) return false;
	uint32_t x = get_u32(p); p += 4;
	if (x < STATE_L || x >= (1u << 31)) return false;
	for (uint64_t r = 0; r < n; ++r) {
		uint8_t *d = dst + r * pitch;
		uint32_t p1 = 0, p2 = 0, p3 = 0;
		for (uint32_t j = 0; j < L; ++j) {
			const uint16_t *row = &cum[(size_t)g.ctx(hd.model, p1, p2, p3, j) * (A + 1)];
			const uint32_t slot = x & (PROB_M - 1);
			uint32_t sym = 0, st = 128;
			for (; st; st >>= 1) if (sym + st < A && row[sym + st] <= slot) sym += st;
			const uint32_t c = row[sym], f = row[sym + 1] - c;
			if (sym >= A || slot - c >= f) return false;
			x = f * (x >> PROB_BITS) + slot - c;
			while (x < STATE_L) { if (p >= end) return false; x = (x << 8) | *p++; }
			d[j] = g.value[sym];
			p3 = p2; p2 = p1; p1 = sym;
		}
	}
	return p == end && x == STATE_L;
}

// Accepts exactly what mcom_qual_decode accepts (section 3.9, "Untrusted input").
int decode(const uint8_t *in, uint64_t in_len, uint8_t *rows, uint64_t pitch, uint64_t cap_rows, uint64_t *n_rows, uint32_t *L_out)
{
	if (!n_rows || !L_out || (in_len && !in)) return -1;
	*n_rows = 0; *L_out = 0;
	QHeader hd;
	if (!in || !read_qheader(in, in_len, hd)) return -1;
	*n_rows = hd.n_rows; *L_out = hd.L;
	if (hd.n_rows > cap_rows) return -4;
	if (pitch < hd.L || (hd.n_rows && !rows)) { *n_rows = 0; *L_out = 0; return -1; }
	const uint32_t L = hd.L;
	const uint64_t raw = hd.raw_len();
	auto refuse = [&]() { *n_rows = 0; *L_out = 0; return -1; };
	if (hd.kind == KIND_RANS) {
		std::vector<uint8_t> flat(raw ? raw : 1);
		uint64_t got = 0;
		if (mcomh_rans_decode(in + QHEADER_BYTES, in_len - QHEADER_BYTES, flat.data(), raw, &got) || got != raw) return refuse();
		for (uint64_t r = 0; r < hd.n_rows; ++r) memcpy(rows + r * pitch, &flat[r * L], L);
		return 0;                                                  // (the embedded member's CRC is the header's: read_qheader)
	}
	if (hd.model == Q_STORED) {
		if ((raw ? mcom_crc32(0, in + QHEADER_BYTES, raw) : 0u) != hd.crc) return refuse();
		for (uint64_t r = 0; r < hd.n_rows; ++r) memcpy(rows + r * pitch, in + QHEADER_BYTES + r * L, L);
		return 0;
	}
	Geometry g; g.set(hd.map, L);
	std::vector<uint16_t> cum;
	if (!parse_tables(in + QHEADER_BYTES, hd.table_bytes, g, hd.model, cum)) return refuse();
	const uint64_t n_seg = hd.n_seg();
	const uint8_t *lens = in + QHEADER_BYTES + hd.table_bytes, *runs = lens + 2 * n_seg;
	uint64_t sum = 0;
	for (uint64_t s = 0; s < n_seg; ++s) sum += get_u16(lens + 2 * s);
	if (sum != hd.payload_bytes) return refuse();
	uint64_t at_run = 0;
	uint32_t crc = 0;
	for (uint64_t seg = 0; seg < n_seg; ++seg) {
		const uint32_t rl = get_u16(lens + 2 * seg);
		const uint64_t r0 = seg * hd.rps, r1 = r0 + hd.rps < hd.n_rows ? r0 + hd.rps : hd.n_rows;
		if (!decode_segment(hd, g, cum, runs + at_run, rl, r1 - r0, rows + r0 * pitch, pitch)) return refuse();
		at_run += rl;
		for (uint64_t r = r0; r < r1; ++r) crc = mcom_crc32(crc, rows + r * pitch, L);
	}
	if (crc != hd.crc) return refuse();
	return 0;
}

// Rows first_row .. first_row + count - 1 alone: accepts exactly what mcom_qual_decode_rows accepts.  The CRC-32
// covers all rows and is not checked for a part; a range that is the whole member is decode(), CRC included.
int decode_rows(const uint8_t *in, uint64_t in_len, uint64_t first_row, uint64_t count, uint8_t *rows, uint64_t pitch, uint64_t *n_rows, uint32_t *L_out)
{
	if (!n_rows || !L_out || (in_len && !in)) return -1;
	*n_rows = 0; *L_out = 0;
	QHeader hd;
	if (!in || !read_qheader(in, in_len, hd)) return -1;
	if (first_row > hd.n_rows) return -1;
	if (count > hd.n_rows - first_row) count = hd.n_rows - first_row;
	if (first_row == 0 && count == hd.n_rows) return decode(in, in_len, rows, pitch, hd.n_rows, n_rows, L_out);
	if (pitch < hd.L || (count && !rows)) return -1;
	const uint32_t L = hd.L;
	const uint64_t raw = hd.raw_len();
	if (hd.kind == KIND_RANS) {                                          // no segments of rows: the whole matrix, then the slice
		std::vector<uint8_t> flat(raw ? raw : 1);
		uint64_t got = 0;
		if (mcomh_rans_decode(in + QHEADER_BYTES, in_len - QHEADER_BYTES, flat.data(), raw, &got) || got != raw) return -1;
		for (uint64_t r = 0; r < count; ++r) memcpy(rows + r * pitch, &flat[(first_row + r) * L], L);
	} else if (hd.model == Q_STORED) {
		for (uint64_t r = 0; r < count; ++r) memcpy(rows + r * pitch, in + QHEADER_BYTES + (first_row + r) * L, L);
	} else {
		Geometry g; g.set(hd.map, L);
		std::vector<uint16_t> cum;
		if (!parse_tables(in + QHEADER_BYTES, hd.table_bytes, g, hd.model, cum)) return -1;
		const uint64_t n_seg = hd.n_seg();
		const uint8_t *lens = in + QHEADER_BYTES + hd.table_bytes, *runs = lens + 2 * n_seg;
		uint64_t sum = 0;
		for (uint64_t s = 0; s < n_seg; ++s) sum += get_u16(lens + 2 * s);
		if (sum != hd.payload_bytes) return -1;
		const uint64_t seg0 = count ? first_row / hd.rps : 0, seg1 = count ? (first_row + count - 1) / hd.rps + 1 : 0;
		uint64_t at_run = 0;
		for (uint64_t s = 0; s < seg0; ++s) at_run += get_u16(lens + 2 * s);
		std::vector<uint8_t> img((size_t)hd.rps * L);
		for (uint64_t seg = seg0; seg < seg1; ++seg) {
			const uint32_t rl = get_u16(lens + 2 * seg);
			const uint64_t r0 = seg * hd.rps, r1 = r0 + hd.rps < hd.n_rows ? r0 + hd.rps : hd.n_rows;
			if (!decode_segment(hd, g, cum, runs + at_run, rl, r1 - r0, img.data(), L)) return -1;
			at_run += rl;
			for (uint64_t r = r0 > first_row ? r0 : first_row; r < r1 && r < first_row + count; ++r) memcpy(rows + (r - first_row) * pitch, &img[(r - r0) * L], L);
		}
	}
	*n_rows = hd.n_rows; *L_out = hd.L;
	return 0;
}

}  // namespace

extern "C" uint64_t mcomh_qual_bound(uint64_t n_rows, uint32_t L) { return bound(n_rows, L); }

extern "C" int mcomh_qual_info(const uint8_t *prefix, uint64_t len, uint64_t *n_rows, uint32_t *L)
{
	QHeader hd;
	if (!prefix || !n_rows || !L || !read_qfields(prefix, len, hd)) return -1;
	*n_rows = hd.n_rows; *L = hd.L;
	return 0;
}

extern "C" int mcomh_qual_encode(const uint8_t *rows, uint64_t n_rows, uint32_t L, uint64_t pitch, uint8_t *out, uint64_t cap, uint64_t *out_len, int model_hint)
{
	try { return encode(rows, n_rows, L, pitch, out, cap, out_len, model_hint); } catch (const std::bad_alloc &) { if (out_len) *out_len = 0; return -1; }
}

extern "C" int mcomh_qual_decode(const uint8_t *in, uint64_t in_len, uint8_t *rows, uint64_t pitch, uint64_t cap_rows, uint64_t *n_rows, uint32_t *L)
{
	try { return decode(in, in_len, rows, pitch, cap_rows, n_rows, L); } catch (const std::bad_alloc &) { if (n_rows) *n_rows = 0; if (L) *L = 0; return -1; }
}

extern "C" int mcomh_qual_decode_rows(const uint8_t *in, uint64_t in_len, uint64_t first_row, uint64_t count, uint8_t *rows, uint64_t pitch, uint64_t *n_rows, uint32_t *L)
{
	try { return decode_rows(in, in_len, first_row, count, rows, pitch, n_rows, L); } catch (const std::bad_alloc &) { if (n_rows) *n_rows = 0; if (L) *L = 0; return -1; }
}

extern "C" int mcomh_qual_estimate(const uint8_t *rows, uint64_t n_rows, uint32_t L, uint64_t pitch, uint64_t est5[5])
{
	if ((n_rows && !rows) || !est5 || L < 1 || L > L_MAX || pitch < L || n_rows >= ((uint64_t)1 << 32)) return -1;
	uint8_t map[32]; Geometry g; std::vector<uint64_t> h4; QModel m;
	map_host(rows, n_rows, L, pitch, map); g.set(map, L);
	hist_host(rows, n_rows, pitch, g, h4);
	const uint64_t rps = default_rps(L);
	choose(g, h4, n_rows, (n_rows + rps - 1) / rps, 0, m, est5);
	return 0;
}

// rows through an order: the host twin of mcom_qual_gather_rows -- the same inputs refused, the same two flags
// raised, an index outside the table not followed, a row named twice copied both times
extern "C" int mcomh_qual_gather_rows(const uint8_t *rows, uint64_t n_src, uint32_t L, uint64_t pitch_in, const uint32_t *order, uint64_t n_rows, uint8_t *out, uint64_t pitch_out,
                                      uint32_t *flag)
{
	if (!flag || (n_rows && (!order || !out)) || (n_src && !rows)) return -1;
	if (L < 1 || L > L_MAX || pitch_in < L || pitch_out < L || n_src >= ((uint64_t)1 << 32) || n_rows >= ((uint64_t)1 << 32)) return -1;
	try {
		std::vector<bool> seen((size_t)n_src, false);
		for (uint64_t j = 0; j < n_rows; ++j) {
			const uint64_t s = order[j];
			if (s >= n_src) { *flag |= MCOMH_GATHER_F_BOUNDS; continue; }
			if (seen[(size_t)s]) *flag |= MCOMH_GATHER_F_DUP;
			seen[(size_t)s] = true;
			memcpy(out + j * pitch_out, rows + s * pitch_in, L);
		}
	} catch (const std::bad_alloc &) { return -1; }
	return 0;
}
