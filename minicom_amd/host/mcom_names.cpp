// minicom_amd/host/mcom_names.cpp -- the read-name coder on the host: the twin of csrc/names.hip and its specification (DESIGN.md
// sections 3.10 and 3.12).  Plain C++ on host buffers -- no GPU, no HIP call: the token rule, the op rule and the record walk are the functions
// of csrc/name_model.hpp that the kernels run, the streams go through the host twins of the `.bwt` and `.rans` coders, so the bytes
// equal the device's and the same members are refused.  Builds alone beside mcom_entropy.cpp and mcom_bwt.cpp (tests/fuzz_names.cpp
// runs it under the sanitizers).
#include "../../include/mcom_host.h"
#include "../csrc/name_model.hpp"
#include "mcom_inflate.hpp"
#include <cstring>
#include <new>
#include <vector>

using namespace mcom_name;

namespace {

struct VecSink {
	std::vector<uint8_t> s[N_STREAMS], lit_bytes;
	void op(uint32_t b) { s[S_OPS].push_back((uint8_t)b); }
	void delta(uint8_t b) { s[S_DELTA].push_back(b); }
	void num(uint32_t v) { const size_t at = s[S_NUM].size(); s[S_NUM].resize(at + 4); put_u32(&s[S_NUM][at], v); }
	void text(const uint8_t *p, uint32_t n) { s[S_TLEN].push_back((uint8_t)n); s[S_TEXT].insert(s[S_TEXT].end(), p, p + n); }
	void plus(uint32_t b) { s[S_PLUS].push_back((uint8_t)b); }
	void literal(const uint8_t *p, uint32_t n) { s[S_PTEXT].push_back((uint8_t)n); lit_bytes.insert(lit_bytes.end(), p, p + n); }
};
struct HostTab {
	uint32_t v[TOKEN_CAP], l[TOKEN_CAP];
	uint32_t &val(uint32_t t) { return v[t]; }
	uint32_t &len(uint32_t t) { return l[t]; }
};

// the 2 n lines of a name text: false when they are not 2 n complete lines; a line above 255 bytes names its record
bool lines_of(const uint8_t *text, uint64_t text_len, uint64_t n, std::vector<uint64_t> &start, uint64_t *bad_record)
{
	if (text_len < 2 * n) return false;
	start.assign(2 * n + 1, 0);
	uint64_t m = 0;
	for (uint64_t i = 0; i < text_len; ++i) if (text[i] == '\n') { if (m == 2 * n) return false; start[++m] = i + 1; }
	if (m != 2 * n || start[2 * n] != text_len) return false;
	for (uint64_t l = 0; l < 2 * n; ++l) if (start[l + 1] - 1 - start[l] > NM_NAME_MAX) { if (bad_record) *bad_record = l / 2; return false; }
	return true;
}

// the seven streams of the text as `.bwt` members behind one another, their lengths into hd.len.  mate NULL: every record against the
// one before it (kinds 0); otherwise against the mate's name of the same record (kind 2)
bool code_streams(const uint8_t *text, const std::vector<uint64_t> &start, uint64_t n, const uint8_t *mate, const std::vector<uint64_t> *mstart, NHeader &hd, std::vector<uint8_t> &body)
{
	VecSink sk;
	for (uint64_t r = 0; r < n; ++r) {
		const bool first = !mate && r % hd.rps == 0;
		const uint8_t *cur = text + start[2 * r], *pl = text + start[2 * r + 1];
		const uint8_t *prv = mate ? mate + (*mstart)[2 * r] : first ? cur : text + start[2 * r - 2];
		const uint32_t clen = (uint32_t)(start[2 * r + 1] - 1 - start[2 * r]), pl_len = (uint32_t)(start[2 * r + 2] - 1 - start[2 * r + 1]);
		const uint32_t plen = mate ? (uint32_t)((*mstart)[2 * r + 1] - 1 - (*mstart)[2 * r]) : first ? 0u : (uint32_t)(start[2 * r - 1] - 1 - start[2 * r - 2]);
		code_record(cur, clen, prv, plen, first, pl, pl_len, sk);
	}
	sk.s[S_PTEXT].insert(sk.s[S_PTEXT].end(), sk.lit_bytes.begin(), sk.lit_bytes.end());
	body.clear();
	for (int k = 0; k < N_STREAMS; ++k) {
		const std::vector<uint8_t> &s = sk.s[k];
		hd.len[k] = 0;
		if (s.empty()) continue;
		if (s.size() > mcom_bwt::RAW_MAX) return false;
		const size_t at = body.size();
		const uint64_t room = mcomh_bwt_bound(s.size());
		body.resize(at + room);
		uint64_t got = 0;
		if (mcomh_bwt_encode(s.data(), s.size(), &body[at], room, &got)) return false;
		body.resize(at + got);
		hd.len[k] = got;
	}
	return true;
}

int encode(const uint8_t *text, uint64_t text_len, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *bad_record)
{
	if (bad_record) *bad_record = ~(uint64_t)0;
	if (!out_len || !out || (text_len && !text)) return -1;
	*out_len = 0;
	if (n > N_MAX || text_len > TEXT_MAX || text_len < 2 * n || (n == 0 && text_len)) return -1;
	if (cap < NHEADER_BYTES) return -4;
	std::vector<uint64_t> start;
	if (!lines_of(text, text_len, n, start, bad_record)) return -1;
	NHeader hd; hd.n_records = n; hd.text_len = text_len; hd.crc = text_len ? mcom_crc32(0, text, text_len) : 0;
	std::vector<uint8_t> body;
	if (!code_streams(text, start, n, nullptr, nullptr, hd, body)) return -1;
	uint64_t total = NHEADER_BYTES + body.size();
	if (n) {
		// kind 1, made last: the `.rans` member of the name text
		std::vector<uint8_t> rans(mcom_rans::HEADER_BYTES + text_len);
		uint64_t got = 0;
		if (mcomh_rans_encode(text, text_len, rans.data(), rans.size(), &got, 0)) return -1;
		if (NHEADER_BYTES + got < total) {
			NHeader rh; rh.kind = KIND_RANS; rh.n_records = n; rh.text_len = text_len; rh.crc = hd.crc;
			total = NHEADER_BYTES + got;
			if (cap < total) return -4;
			write_nheader(out, rh);
			memcpy(out + NHEADER_BYTES, rans.data(), got);
			*out_len = total;
			return 0;
		}
	}
	if (cap < total) return -4;
	write_nheader(out, hd);
	if (!body.empty()) memcpy(out + NHEADER_BYTES, body.data(), body.size());
	*out_len = total;
	return 0;
}

// Kind 2 (section 3.12): the member encode() makes, unless the streams coded against the mate are strictly smaller.
int encode_mate(const uint8_t *text, uint64_t text_len, uint64_t n, const uint8_t *mate, uint64_t mate_len, uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *bad_record)
{
	const int rc = encode(text, text_len, n, out, cap, out_len, bad_record);
	if (rc) return rc;
	auto refuse = [&]() { *out_len = 0; return -1; };
	if (mate_len && !mate) return refuse();
	std::vector<uint64_t> start, mstart;
	if (mate_len > TEXT_MAX || !lines_of(mate, mate_len, n, mstart, nullptr)) return refuse();          // a mate of another n, or no name text at all
	if (n == 0) return 0;
	if (!lines_of(text, text_len, n, start, nullptr)) return refuse();
	NHeader hd; hd.kind = KIND_MATE; hd.rps = 1; hd.n_records = n; hd.text_len = text_len;
	hd.crc = mcom_crc32(0, text, text_len); hd.mate_crc = mcom_crc32(0, mate, mate_len);
	std::vector<uint8_t> body;
	if (!code_streams(text, start, n, mate, &mstart, hd, body)) return refuse();
	if (NHEADER_BYTES + body.size() >= *out_len) return 0;
	write_nheader(out, hd);
	memcpy(out + NHEADER_BYTES, body.data(), body.size());
	*out_len = NHEADER_BYTES + body.size();
	return 0;
}

// Accepts exactly what mcom_name_decode accepts (section 3.10, "Untrusted input").
// with_mate: the caller holds a mate text (mcomh_name_decode_mate): kind 2 is taken and decoded against it; kinds 0 and 1 do not look at it.
int decode(const uint8_t *in, uint64_t in_len, uint8_t *text, uint64_t cap, uint64_t *text_len, uint64_t *n_records, bool with_mate = false, const uint8_t *mate = nullptr, uint64_t mate_len = 0)
{
	if (!text_len || !n_records || (in_len && !in) || (with_mate && mate_len && !mate)) return -1;
	*text_len = 0; *n_records = 0;
	NHeader hd;
	if (!in || !read_nheader(in, in_len, hd, with_mate)) return -1;
	*text_len = hd.text_len; *n_records = hd.n_records;
	if (hd.text_len > cap) return -4;
	auto refuse = [&]() { *text_len = 0; *n_records = 0; return -1; };
	if (hd.text_len && !text) return refuse();
	const uint64_t n = hd.n_records;
	std::vector<uint64_t> mstart;
	if (hd.kind == KIND_MATE) {                                            // the mate: the 2 n lines the member was coded against
		if (mate_len > TEXT_MAX || !lines_of(mate, mate_len, n, mstart, nullptr)) return refuse();
		if ((mate_len ? mcom_crc32(0, mate, mate_len) : 0u) != hd.mate_crc) return refuse();
	}
	if (hd.kind == KIND_RANS) {
		uint64_t got = 0;
		if (mcomh_rans_decode(in + NHEADER_BYTES, in_len - NHEADER_BYTES, text, hd.text_len, &got) || got != hd.text_len) return refuse();
		// (the embedded member's CRC is the header's: read_nheader.)  The text must still be 2 n lines of at most 255 bytes.
		uint64_t lines = 0, at = 0;
		for (uint64_t i = 0; i < got; ++i) if (text[i] == '\n') { if (i - at > NM_NAME_MAX) return refuse(); at = i + 1; ++lines; }
		if (lines != 2 * n || at != got) return refuse();
		return 0;
	}
	// the seven streams
	std::vector<uint8_t> s[N_STREAMS];
	uint64_t raw[N_STREAMS] = {0};
	const uint8_t *m[N_STREAMS];
	{
		const uint8_t *p = in + NHEADER_BYTES;
		for (int k = 0; k < N_STREAMS; ++k) { m[k] = p; p += hd.len[k]; if (hd.len[k] && !embedded_raw_len(m[k], hd.len[k], raw[k])) return refuse(); }
	}
	if (!check_raw_lens(hd, raw)) return refuse();
	for (int k = 0; k < N_STREAMS; ++k) {
		if (!hd.len[k]) continue;
		s[k].resize(raw[k]);
		uint64_t got = 0;
		if (mcomh_bwt_decode(m[k], hd.len[k], s[k].data(), raw[k], &got) || got != raw[k]) return refuse();
	}
	// the counts
	uint64_t cnt[OP_END + 1] = {0};
	for (uint8_t b : s[S_OPS]) { if (b > OP_END) return refuse(); ++cnt[b]; }
	if (cnt[OP_END] != n || (n && s[S_OPS].back() != OP_END)) return refuse();
	if (cnt[OP_DELTA] != raw[S_DELTA] || 4 * cnt[OP_NUM] != raw[S_NUM] || cnt[OP_TEXT] != raw[S_TLEN]) return refuse();
	uint64_t sum = 0;
	for (uint8_t b : s[S_TLEN]) sum += b;
	if (sum != raw[S_TEXT]) return refuse();
	uint64_t K = 0;
	for (uint8_t b : s[S_PLUS]) { if (b > PLUS_LITERAL) return refuse(); K += b == PLUS_LITERAL; }
	if (K > raw[S_PTEXT]) return refuse();
	sum = K;
	for (uint64_t k = 0; k < K; ++k) sum += s[S_PTEXT][k];
	if (sum != raw[S_PTEXT]) return refuse();
	for (uint8_t b : s[S_TEXT]) if (b == '\n') return refuse();
	for (uint64_t k = K; k < raw[S_PTEXT]; ++k) if (s[S_PTEXT][k] == '\n') return refuse();
	// the walk, twice as on the device: lengths, then bytes
	View v = { s[S_OPS].data(), s[S_DELTA].data(), s[S_NUM].data(), s[S_TLEN].data(), s[S_TEXT].data(), raw[S_OPS], raw[S_DELTA], raw[S_NUM] / 4, raw[S_TLEN], raw[S_TEXT] };
	for (int pass = 0; pass < 2; ++pass) {
		Cursor c; HostTab tab; uint32_t n_prev = 0;
		uint64_t at = 0, lit = 0, lit_at = K;
		uint8_t name[NM_NAME_MAX + 1];
		for (uint64_t r = 0; r < n; ++r) {
			if (r % hd.rps == 0) n_prev = 0;
			uint32_t nl = 0;
			if (hd.kind == KIND_MATE) {
				if (walk_record_mate(v, c, mate + mstart[2 * r], (uint32_t)(mstart[2 * r + 1] - 1 - mstart[2 * r]), pass ? name : nullptr, NM_NAME_MAX, nl)) return refuse();
			} else if (walk_record(v, c, tab, n_prev, pass ? name : nullptr, NM_NAME_MAX, nl)) return refuse();
			const uint32_t kind = s[S_PLUS][r];
			const uint32_t pl = kind == PLUS_BARE ? 0u : kind == PLUS_NAME ? nl : (uint32_t)s[S_PTEXT][lit];
			if (pass) {
				memcpy(text + at, name, nl); text[at + nl] = '\n';
				if (kind == PLUS_NAME) memcpy(text + at + nl + 1, name, nl);
				else if (kind == PLUS_LITERAL) memcpy(text + at + nl + 1, &s[S_PTEXT][lit_at], pl);
				text[at + nl + 1 + pl] = '\n';
			}
			if (kind == PLUS_LITERAL) { ++lit; lit_at += pl; }
			at += (uint64_t)nl + pl + 2;
			if (at > hd.text_len) return refuse();
		}
		if (at != hd.text_len) return refuse();
	}
	if ((hd.text_len ? mcom_crc32(0, text, hd.text_len) : 0u) != hd.crc) return refuse();
	return 0;
}

}  // namespace

extern "C" uint64_t mcomh_name_bound(uint64_t text_len) { return bound(text_len); }

extern "C" int mcomh_name_info(const uint8_t *prefix, uint64_t len, uint64_t *n_records, uint64_t *text_len)
{
	NHeader hd;
	if (!prefix || !n_records || !text_len || !read_nfields(prefix, len, hd)) return -1;
	*n_records = hd.n_records; *text_len = hd.text_len;
	return 0;
}

extern "C" int mcomh_name_info_mate(const uint8_t *prefix, uint64_t len, uint64_t *n_records, uint64_t *text_len)
{
	NHeader hd;
	if (!prefix || !n_records || !text_len || !read_nfields(prefix, len, hd, true)) return -1;
	*n_records = hd.n_records; *text_len = hd.text_len;
	return 0;
}

extern "C" int mcomh_name_encode(const uint8_t *text, uint64_t text_len, uint64_t n_records, uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *bad_record)
{
	try { return encode(text, text_len, n_records, out, cap, out_len, bad_record); } catch (const std::bad_alloc &) { if (out_len) *out_len = 0; return -1; }
}

extern "C" int mcomh_name_decode(const uint8_t *in, uint64_t in_len, uint8_t *text, uint64_t cap, uint64_t *text_len, uint64_t *n_records)
{
	try { return decode(in, in_len, text, cap, text_len, n_records); } catch (const std::bad_alloc &) { if (text_len) *text_len = 0; if (n_records) *n_records = 0; return -1; }
}

extern "C" int mcomh_name_encode_mate(const uint8_t *text, uint64_t text_len, uint64_t n_records, const uint8_t *mate, uint64_t mate_len, uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *bad_record)
{
	try { return encode_mate(text, text_len, n_records, mate, mate_len, out, cap, out_len, bad_record); } catch (const std::bad_alloc &) { if (out_len) *out_len = 0; return -1; }
}

extern "C" int mcomh_name_decode_mate(const uint8_t *in, uint64_t in_len, const uint8_t *mate, uint64_t mate_len, uint8_t *text, uint64_t cap, uint64_t *text_len, uint64_t *n_records)
{
	try { return decode(in, in_len, text, cap, text_len, n_records, true, mate, mate_len); } catch (const std::bad_alloc &) { if (text_len) *text_len = 0; if (n_records) *n_records = 0; return -1; }
}
