// minicom_amd/host/mcom_bwt.cpp -- the block-sorting coder on the host: the twin of csrc/bwt.hip and its specification (DESIGN.md
// section 3.8; format and checks: csrc/bwt_model.hpp).
//
// mcomh_bwt_encode / mcomh_bwt_decode are plain C++ on host buffers -- no GPU, no HIP call.  Per block: the suffixes sorted by prefix
// doubling (groups of equal rank are sorted by the rank h positions on, settled groups are skipped), the transformed bytes, the primary
// index and the anchors; sequential move-to-front; the ranks of all blocks through mcomh_rans_encode.  The plain `.rans` coding of the
// raw bytes is made as well and the smaller of the two is written (a tie goes to plain).  The bytes equal the device's and the same
// members are refused.  Builds alone beside mcom_entropy.cpp with -DMCOM_ENTROPY_HOST_ONLY (tests/fuzz_bwt.cpp runs it under the
// sanitizers).
#include "../../include/mcom_host.h"
#include "../csrc/bwt_model.hpp"
#include "mcom_inflate.hpp"
#include <algorithm>
#include <new>
#include <numeric>
#include <vector>

using namespace mcom_bwt;

namespace {

// sa[0 .. len): the start positions of the suffixes of t[0 .. len) in ascending order, the end of the block below every byte
void suffix_sort(const uint8_t *t, uint32_t len, std::vector<uint32_t> &sa, std::vector<uint32_t> &rank, std::vector<uint32_t> &tmp)
{
	sa.resize(len); rank.assign((size_t)len + 1, 0); tmp.resize(len);
	uint32_t cnt[257] = {0};
	for (uint32_t i = 0; i < len; ++i) ++cnt[t[i] + 1];
	for (int c = 0; c < 256; ++c) cnt[c + 1] += cnt[c];
	for (uint32_t i = 0; i < len; ++i) sa[cnt[t[i]]++] = i;
	// rank = 1 + the index of the first suffix of the group in sa; rank[len] = 0 is the empty suffix
	for (uint32_t j = 0; j < len; ++j) rank[sa[j]] = j && t[sa[j]] == t[sa[j - 1]] ? rank[sa[j - 1]] : j + 1;
	for (uint64_t h = 1; ; h *= 2) {
		bool all_single = true;
		auto key = [&](uint32_t p) { return (uint64_t)p + h <= len ? rank[p + h] : 0u; };
		for (uint32_t a = 0; a < len; ) {
			uint32_t b = a + 1;
			while (b < len && rank[sa[b]] == rank[sa[a]]) ++b;
			tmp[a] = a + 1;
			if (b - a > 1) {
				all_single = false;
				std::sort(sa.begin() + a, sa.begin() + b, [&](uint32_t p, uint32_t q) { return key(p) < key(q); });
				for (uint32_t j = a + 1; j < b; ++j) tmp[j] = key(sa[j]) == key(sa[j - 1]) ? tmp[j - 1] : j + 1;
			}
			a = b;
		}
		if (all_single) return;
		for (uint32_t j = 0; j < len; ++j) rank[sa[j]] = tmp[j];              // (only now: the keys above are the old ranks)
	}
}

void mtf_encode(const uint8_t *in, uint64_t n, uint8_t *out)
{
	uint8_t list[256];
	std::iota(list, list + 256, 0);
	for (uint64_t i = 0; i < n; ++i) {
		const uint8_t c = in[i];
		uint32_t k = 0;
		while (list[k] != c) ++k;
		memmove(list + 1, list, k);
		list[0] = c; out[i] = (uint8_t)k;
	}
}
void mtf_decode(const uint8_t *in, uint64_t n, uint8_t *out)
{
	uint8_t list[256];
	std::iota(list, list + 256, 0);
	for (uint64_t i = 0; i < n; ++i) {
		const uint32_t k = in[i];
		const uint8_t c = list[k];
		memmove(list + 1, list, k);
		list[0] = c; out[i] = c;
	}
}

}  // namespace

extern "C" uint64_t mcomh_bwt_bound(uint64_t n) { return HEADER_BYTES + mcom_rans::HEADER_BYTES + n + 4 * ((n >> ANC_LOG2) + (n >> BLK_LOG2) + 2); }

// stage results for tests and tools: the transformed bytes (n), the index (4 bytes per anchor, as in the member) and the ranks (n)
static int bwt_stages_impl(const uint8_t *in, uint64_t n, uint8_t *bwt, uint8_t *index, uint8_t *ranks)
{
	if ((n && !in) || n > RAW_MAX) return -1;
	Header hd; hd.raw_len = n;
	std::vector<uint32_t> sa, rank, tmp;
	const uint64_t af = hd.anchors_full();
	for (uint64_t b = 0; b < hd.n_blocks(); ++b) {
		const uint8_t *t = in + (b << hd.blk_log2);
		const uint32_t len = (uint32_t)hd.block_len(b);
		suffix_sort(t, len, sa, rank, tmp);
		uint8_t *o = bwt ? bwt + (b << hd.blk_log2) : nullptr;
		uint32_t at = 0;
		if (o) o[at] = t[len - 1];
		++at;
		for (uint32_t j = 0; j < len; ++j) {                                // row j + 1
			const uint32_t p = sa[j];
			if (index && (p & ((1u << hd.anc_log2) - 1)) == 0) put_u32(index + 4 * (b * af + (p >> hd.anc_log2)), j + 1);
			if (p) { if (o) o[at] = t[p - 1]; ++at; }
		}
		if (ranks && o) mtf_encode(o, len, ranks + (b << hd.blk_log2));
	}
	return 0;
}
// (an allocation that fails is an error return, never an exception through the C boundary)
extern "C" int mcomh_bwt_stages(const uint8_t *in, uint64_t n, uint8_t *bwt, uint8_t *index, uint8_t *ranks)
{
	try { return bwt_stages_impl(in, n, bwt, index, ranks); } catch (const std::bad_alloc &) { return -3; }
}

static int bwt_encode_impl(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len)
{
	if (!out_len || !out || (n && !in)) return -1;
	*out_len = 0;
	if (n > RAW_MAX) return -1;
	Header hd; hd.raw_len = n; hd.crc = n ? mcom_crc32(0, in, n) : 0;
	std::vector<uint8_t> plain(mcom_rans::HEADER_BYTES + n);
	uint64_t plain_len = 0, coded_len = 0;
	if (mcomh_rans_encode(in, n, plain.data(), plain.size(), &plain_len, 0)) return -1;
	const uint64_t index_bytes = 4 * hd.n_anchors();
	std::vector<uint8_t> coded;
	if (n) {
		std::vector<uint8_t> bwt(n), ranks(n), index(index_bytes);
		if (mcomh_bwt_stages(in, n, bwt.data(), index.data(), ranks.data())) return -1;
		coded.resize(index_bytes + mcom_rans::HEADER_BYTES + n);
		memcpy(coded.data(), index.data(), index_bytes);
		if (mcomh_rans_encode(ranks.data(), n, coded.data() + index_bytes, coded.size() - index_bytes, &coded_len, 0)) return -1;
	}
	const bool use_bwt = n && index_bytes + coded_len < plain_len;
	hd.kind = use_bwt ? KIND_BWT : KIND_PLAIN;
	hd.index_bytes = use_bwt ? index_bytes : 0;
	hd.member_bytes = use_bwt ? coded_len : plain_len;
	const uint64_t total = HEADER_BYTES + hd.index_bytes + hd.member_bytes;
	if (total > cap) return -4;
	write_header(out, hd);
	memcpy(out + HEADER_BYTES, use_bwt ? coded.data() : plain.data(), total - HEADER_BYTES);
	*out_len = total;
	return 0;
}
// (an allocation that fails is an error return, never an exception through the C boundary)
extern "C" int mcomh_bwt_encode(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len)
{
	try { return bwt_encode_impl(in, n, out, cap, out_len); } catch (const std::bad_alloc &) { if (out_len) *out_len = 0; return -3; }
}

// Accepts exactly what mcom_bwt_decode accepts (the refusal rules of DESIGN 3.8).
static int bwt_decode_impl(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t cap, uint64_t *out_len)
{
	if (!out_len || (in_len && !in)) return -1;
	*out_len = 0;
	Header hd;
	if (!read_header(in, in_len, hd)) return -1;
	const uint8_t *index = in + HEADER_BYTES, *member = index + hd.index_bytes;
	if (!check_embedded(member, hd)) return -1;
	if (hd.kind == KIND_BWT && !check_index(index, hd)) return -1;
	*out_len = hd.raw_len;
	if (hd.raw_len > cap) return -4;
	if (hd.raw_len && !out) return -1;
	uint64_t got = 0;
	if (hd.kind == KIND_PLAIN) {
		if (mcomh_rans_decode(member, hd.member_bytes, out, cap, &got) || got != hd.raw_len) { *out_len = 0; return -1; }
		return 0;                                                           // (its CRC is the header's: check_embedded)
	}
	const uint64_t n = hd.raw_len, af = hd.anchors_full(), A = (uint64_t)1 << hd.anc_log2;
	std::vector<uint8_t> ranks(n), bwt(n);
	if (mcomh_rans_decode(member, hd.member_bytes, ranks.data(), n, &got) || got != n) { *out_len = 0; return -1; }
	std::vector<uint32_t> lf;
	bool bad = false;
	for (uint64_t b = 0; b < hd.n_blocks() && !bad; ++b) {
		const uint64_t at = b << hd.blk_log2;
		const uint32_t len = (uint32_t)hd.block_len(b), na = (uint32_t)hd.anchors_of(len);
		uint8_t *o = bwt.data() + at, *t = out + at;
		mtf_decode(ranks.data() + at, len, o);
		// the row that follows transformed byte j: 1 + the bytes below it + the equal bytes in front of it
		uint32_t cnt[257] = {0};
		for (uint32_t j = 0; j < len; ++j) ++cnt[o[j] + 1];
		for (int c = 0; c < 256; ++c) cnt[c + 1] += cnt[c];
		lf.resize(len);
		for (uint32_t j = 0; j < len; ++j) lf[j] = 1 + cnt[o[j]]++;
		const uint8_t *ix = index + 4 * b * af;
		const uint32_t r0 = get_u32(ix);
		for (uint32_t k = 0; k < na && !bad; ++k) {
			const uint64_t lo = k * A, hi = lo + A < len ? lo + A : len;
			uint32_t r = hi == len ? 0u : get_u32(ix + 4 * (k + 1));
			for (uint64_t p = hi; p > lo; ) {
				if (r == r0 || r > len) { bad = true; break; }                  // the row without a byte, or no row of this block
				const uint32_t j = r < r0 ? r : r - 1;
				t[--p] = o[j]; r = lf[j];
			}
			if (!bad && r != get_u32(ix + 4 * k)) bad = true;                  // the stretch ends where the index says it begins
		}
	}
	if (bad || mcom_crc32(0, out, n) != hd.crc) { *out_len = 0; return -1; }
	return 0;
}
// (an allocation that fails is an error return, never an exception through the C boundary)
extern "C" int mcomh_bwt_decode(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t cap, uint64_t *out_len)
{
	try { return bwt_decode_impl(in, in_len, out, cap, out_len); } catch (const std::bad_alloc &) { if (out_len) *out_len = 0; return -3; }
}

// what a member says its raw length is (file routes and bindings size their buffers from it); -1: not a `.bwt` header for in_len bytes
extern "C" int mcomh_bwt_raw_len(const uint8_t *in, uint64_t in_len, uint64_t *raw_len)
{
	Header hd;
	if (!in || !raw_len || in_len < HEADER_BYTES) return -1;
	uint8_t hb[HEADER_BYTES]; memcpy(hb, in, HEADER_BYTES);
	if (!read_header(hb, in_len, hd)) return -1;
	*raw_len = hd.raw_len;
	return 0;
}
