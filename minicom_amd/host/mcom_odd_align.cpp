// minicom_amd/host/mcom_odd_align.cpp -- the odd reads of a -V archive coded against the contigs (`minicom -p -V -A`).
//
// The rule and the member are stated in csrc/odd_align_model.hpp.  Here:
//   mcomh_odd_text_append    `bases` bases of a ref.bin image behind base `at` of the packed text T
//   mcomh_odd_index_build    the seed grid of T as sorted (key, position) pairs          (the twin of mcom_odd_index_build)
//   mcomh_odd_align          one hit word per odd record                                 (... of mcom_odd_align)
//   mcomh_odd_align_encode   hit words + odd text -> the member odd.aln and the residual (... of mcom_odd_align_encode)
//   mcomh_odd_align_decode   member + T + residual -> the full odd text                  (... of mcom_odd_align_decode)
//   mcomh_odd_align_folder   the ungrouped stream files of a folder: odd.aln written, odd.seq rewritten; on GPU `device` by the device calls,
//                            device -1 by the twins: the same bytes
//   mcom_odd_align_rebuild   what the decoders run when a folder holds odd.aln: the full odd text in place of the residual
#include "../../include/mcom_host.h"
#include "mcom_ragged.hpp"
#include "mcom_streams.hpp"
#include "../csrc/odd_align_model.hpp"
#include <zlib.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#ifndef MCOM_ENTROPY_HOST_ONLY
#include "../../include/mcom.h"
#include <hip/hip_runtime.h>
#endif

struct mcomh_odd_index { std::vector<std::pair<uint64_t, uint64_t>> grid; };   // (key, position), sorted

namespace {
int fail(char *err, size_t cap, const char *msg) { if (err && cap) snprintf(err, cap, "%s", msg); return -1; }

bool write_file(const std::string &path, const uint8_t *p, size_t n)
{
	FILE *f = fopen(path.c_str(), "wb");
	if (!f) return false;
	const bool ok = !n || fwrite(p, 1, n, f) == n;
	if (fclose(f) || !ok) { remove(path.c_str()); return false; }
	return true;
}

// the bases the contigs of one stream set hold (what mcom_decode_member_table reports in *h_ref_bases): per contig its last begin position + L
bool set_ref_bases(const std::vector<uint8_t> &pos, int L, uint64_t &bases)
{
	size_t pp = 0;
	bases = 0;
	while (pp + 4 <= pos.size()) {
		uint32_t num; memcpy(&num, pos.data() + pp, 4); pp += 4;
		if (2 * (uint64_t)num > pos.size() - pp) return false;
		uint64_t p = 0;
		for (uint32_t q = 0; q < num; ++q) { uint16_t d; memcpy(&d, pos.data() + pp, 2); pp += 2; p += d; }
		if (p + (uint64_t)L > 0x7FFFFFFFull) return false;
		if (num) bases += p + (uint64_t)L;
	}
	return true;
}

// T of a folder of ungrouped stream files
// refs / nb: the ref.bin image of every set and the bases taken from it; t: T packed on the host (pack = true: the twins and the host decoder;
// the GPU route appends the images on the card instead)
struct FolderText { std::vector<uint64_t> t; uint64_t bases = 0; int L = 0; std::vector<std::vector<uint8_t>> refs; std::vector<uint64_t> nb; };
bool folder_text(const std::string &dir, FolderText &F, std::string &why, bool pack = true)
{
	using namespace mcom_streams;
	StreamInfo I;
	if (!read_info(ORDER, dir, I)) { why = "no info.txt of a -p archive"; return false; }
	F.L = I.L;
	std::vector<std::vector<uint8_t>> &refs = F.refs;
	std::vector<uint64_t> &nb = F.nb;
	refs.assign((size_t)I.nth, std::vector<uint8_t>()); nb.assign((size_t)I.nth, 0);
	uint64_t total = 0;
	for (int th = 0; th < I.nth; ++th) {
		std::vector<uint8_t> pos;
		const std::string sfx = "." + std::to_string(th);
		if (!slurp(dir + "/ref.bin" + sfx, refs[th]) || !slurp(dir + "/beg_pos.bin" + sfx, pos)) { why = "cannot read ref.bin / beg_pos.bin of a stream set"; return false; }
		if (!set_ref_bases(pos, I.L, nb[th]) || nb[th] > 4 * (uint64_t)refs[th].size()) { why = "ref.bin is shorter than its contigs"; return false; }
		total += nb[th];
		if (total >= OA_MAX_T) { why = "the contigs hold 2^40 bases or more"; return false; }
	}
	if (!pack) { F.bases = total; return true; }
	F.t.assign((size_t)oa_words(total), 0);
	for (int th = 0; th < I.nth; ++th) { mcomh_odd_text_append(F.t.data(), F.bases, refs[th].data(), refs[th].size(), nb[th]); F.bases += nb[th]; }
	return true;
}

// the odd records of len.bin: off[j] = where odd record j begins in the full odd text, off[n_odd] = its size
void odd_offsets(const std::vector<uint8_t> &len, int L, std::vector<uint64_t> &off)
{
	off.clear(); off.push_back(0);
	for (uint8_t b : len) if ((int)b + 1 != L) off.push_back(off.back() + (uint64_t)b + 1);
}
}  // namespace

extern "C" const char *mcomh_odd_align_refusal(uint32_t flags) { return oa_refusal(flags); }

extern "C" void mcomh_odd_text_append(uint64_t *t, uint64_t at, const uint8_t *ref, uint64_t ref_bytes, uint64_t bases)
{
	if (bases > 4 * ref_bytes) bases = 4 * ref_bytes;
	for (uint64_t i = 0; i < bases; ++i) {
		const uint64_t c = (ref[i >> 2] >> (2 * (i & 3))) & 3u, b = at + i;
		t[b >> 5] |= c << (2 * (b & 31));
	}
}

extern "C" int mcomh_odd_index_build(const uint64_t *t, uint64_t t_bases, mcomh_odd_index **idx)
{
	if (!idx || (t_bases && !t) || t_bases >= OA_MAX_T) return -1;
	try {
		mcomh_odd_index *X = new mcomh_odd_index;
		const uint64_t n = oa_grid_size(t_bases);
		X->grid.reserve((size_t)n);
		for (uint64_t g = 0; g < n; ++g) X->grid.emplace_back(oa_key(t, g * OA_G), g * OA_G);
		std::sort(X->grid.begin(), X->grid.end());
		*idx = X;
		return 0;
	} catch (...) { return -1; }
}
extern "C" void mcomh_odd_index_free(mcomh_odd_index *idx) { delete idx; }
extern "C" uint64_t mcomh_odd_index_size(const mcomh_odd_index *idx) { return idx ? idx->grid.size() : 0; }

extern "C" int mcomh_odd_align(const mcomh_odd_index *idx, const uint64_t *t, uint64_t t_bases, const uint8_t *odd, const uint64_t *off, uint64_t n_odd, uint64_t *hits)
{
	if (!idx || !off || (n_odd && !hits) || (t_bases && !t) || t_bases >= OA_MAX_T) return -1;
	const auto &grid = idx->grid;
	for (uint64_t r = 0; r < n_odd; ++r) {
		hits[r] = OA_NONE;
		if (off[r + 1] < off[r] || off[r + 1] - off[r] > OA_MAX_LEN) return -1;
		const uint32_t l = (uint32_t)(off[r + 1] - off[r]);
		if (l < OA_MIN_LEN || l > t_bases) continue;
		const uint8_t *read = odd + off[r];
		const uint32_t E = oa_budget(l);
		uint32_t code[OA_MAX_LEN];
		for (uint32_t s = 0; s < 2; ++s) {
			for (uint32_t j = 0; j < l; ++j) code[j] = s ? oa_comp(oa_code(read[l - 1 - j])) : oa_code(read[j]);   // the read as it is laid on T
			for (uint32_t o = 0; o + OA_K <= l; ++o) {
				uint64_t key = 0; bool clean = true;
				for (uint32_t j = 0; j < OA_K; ++j) { if (code[o + j] > 3) { clean = false; break; } key |= (uint64_t)code[o + j] << (2 * j); }
				if (!clean) continue;
				auto lo = std::lower_bound(grid.begin(), grid.end(), std::make_pair(key, (uint64_t)0));
				auto hi = lo;
				while (hi != grid.end() && hi->first == key) ++hi;
				if (hi - lo > OA_M) continue;
				for (auto it = lo; it != hi; ++it) {
					if (it->second < o) continue;
					const uint64_t p = it->second - o;
					if (p + l > t_bases) continue;
					uint32_t d = 0;
					for (uint32_t j = 0; j < l && d <= E; ++j) d += code[j] != oa_base(t, p + j);
					if (d > E) continue;
					const uint64_t h = oa_hit(d, s, p);
					if (h < hits[r]) hits[r] = h;
				}
			}
		}
	}
	return 0;
}

extern "C" int mcomh_odd_align_encode(const uint64_t *hits, const uint8_t *odd, const uint64_t *off, uint64_t n_odd, const uint64_t *t, uint64_t t_bases, uint8_t *member,
                                      uint64_t member_cap, uint64_t *member_len, uint8_t *residual, uint64_t res_cap, uint64_t *res_len)
{
	if (!off || !member_len || !res_len || (n_odd && !hits) || t_bases >= OA_MAX_T) return -1;
	*member_len = *res_len = 0;
	// the sizes and every check of the hit words first
	uint64_t n_aligned = 0, n_mm = 0, res = 0;
	for (uint64_t r = 0; r < n_odd; ++r) {
		if (off[r + 1] < off[r] || off[r + 1] - off[r] > OA_MAX_LEN) return -1;
		const uint32_t l = (uint32_t)(off[r + 1] - off[r]);
		for (uint32_t j = 0; j < l; ++j) if (oa_code(odd[off[r] + j]) > 4) return -1;
		if (hits[r] == OA_NONE) { res += l; continue; }
		const uint64_t p = oa_hit_p(hits[r]);
		const uint32_t d = oa_hit_d(hits[r]), s = oa_hit_s(hits[r]);
		if (hits[r] != oa_hit(d, s, p) || l < OA_MIN_LEN || p > t_bases || l > t_bases - p || d > oa_budget(l) || oa_encode_read(t, odd + off[r], l, s, p, nullptr, nullptr) != d) return -1;
		++n_aligned; n_mm += d;
	}
	const uint64_t odd_bytes = off[n_odd];
	if (!n_aligned) {                                                           // no member: the residual is the text
		*res_len = odd_bytes;
		if (!residual) return 0;
		if (odd_bytes > res_cap) return -2;
		if (odd_bytes) memcpy(residual, odd, (size_t)odd_bytes);
		return 0;
	}
	const OaLayout Y = oa_layout(n_odd, n_aligned, n_mm);
	*member_len = Y.total; *res_len = res;
	if (!member) return 0;
	if (Y.total > member_cap || res > res_cap || (res && !residual)) return -2;
	memset(member, 0, (size_t)Y.total);
	OaHeader H;
	H.K = OA_K; H.G = OA_G; H.M = OA_M;
	{ uLong c = crc32(0, nullptr, 0); for (uint64_t a = 0; a < odd_bytes; a += 1u << 30) c = crc32(c, odd + a, (uInt)std::min<uint64_t>(odd_bytes - a, 1u << 30)); H.crc = (uint32_t)c; }
	H.n_odd = n_odd; H.n_aligned = n_aligned; H.t_bases = t_bases; H.n_mm = n_mm; H.residual = res;
	oa_header_put(member, H);
	uint64_t a = 0, m = 0, ro = 0;
	for (uint64_t r = 0; r < n_odd; ++r) {
		const uint32_t l = (uint32_t)(off[r + 1] - off[r]);
		if (hits[r] == OA_NONE) { memcpy(residual + ro, odd + off[r], l); ro += l; continue; }
		const uint64_t p = oa_hit_p(hits[r]);
		const uint32_t d = oa_hit_d(hits[r]), s = oa_hit_s(hits[r]);
		member[Y.aligned + (r >> 3)] |= (uint8_t)(1u << (r & 7));
		if (s) member[Y.strand + (a >> 3)] |= (uint8_t)(1u << (a & 7));
		for (int b = 0; b < 5; ++b) member[Y.p + (uint64_t)b * n_aligned + a] = (uint8_t)(p >> (8 * b));
		member[Y.d + a] = (uint8_t)d;
		oa_encode_read(t, odd + off[r], l, s, p, member + Y.mm_off + m, member + Y.mm_base + m);
		++a; m += d;
	}
	return 0;
}

extern "C" int mcomh_odd_align_decode(const uint8_t *member, uint64_t member_len, const uint64_t *t, uint64_t t_bases, const uint8_t *residual, uint64_t res_len, const uint64_t *off,
                                      uint64_t n_odd, uint8_t *out, uint32_t *flags)
{
	if (!member || !off || !flags || (t_bases && !t) || (res_len && !residual)) return -1;
	const uint64_t odd_bytes = off[n_odd];
	if (odd_bytes && !out) return -1;
	OaHeader H;
	if ((*flags = oa_header_check(member, member_len, n_odd, odd_bytes, t_bases, res_len, H))) return -1;
	const OaLayout Y = oa_layout(H.n_odd, H.n_aligned, H.n_mm);
	const uint8_t *ab = member + Y.aligned, *sb = member + Y.strand, *dd = member + Y.d;
	// the counts: the bits, the sum of d, the lengths of the unaligned records
	uint64_t na = 0, nm = 0, res = 0;
	for (uint64_t r = 0; r < n_odd; ++r) {
		if (off[r + 1] < off[r] || off[r + 1] - off[r] > OA_MAX_LEN) return -1;
		if ((ab[r >> 3] >> (r & 7)) & 1u) ++na; else res += off[r + 1] - off[r];
	}
	if (n_odd & 7 && ab[n_odd >> 3] >> (n_odd & 7)) *flags |= OA_F_COUNT;
	if (H.n_aligned & 7 && sb[H.n_aligned >> 3] >> (H.n_aligned & 7)) *flags |= OA_F_COUNT;
	for (uint64_t a = 0; a < H.n_aligned; ++a) nm += dd[a];
	if (na != H.n_aligned || nm != H.n_mm || res != H.residual) *flags |= OA_F_COUNT;
	if (*flags) return -1;
	uint64_t a = 0, m = 0, ro = 0;
	for (uint64_t r = 0; r < n_odd; ++r) {
		const uint32_t l = (uint32_t)(off[r + 1] - off[r]);
		if (!((ab[r >> 3] >> (r & 7)) & 1u)) { memcpy(out + off[r], residual + ro, l); ro += l; continue; }
		uint64_t p = 0;
		for (int b = 0; b < 5; ++b) p |= (uint64_t)member[Y.p + (uint64_t)b * H.n_aligned + a] << (8 * b);
		*flags |= oa_decode_read(t, t_bases, l, (sb[a >> 3] >> (a & 7)) & 1u, p, dd[a], member + Y.mm_off + m, member + Y.mm_base + m, out + off[r]);
		m += dd[a]; ++a;
	}
	if (*flags) return -1;
	uLong c = crc32(0, nullptr, 0);
	for (uint64_t at = 0; at < odd_bytes; at += 1u << 30) c = crc32(c, out + at, (uInt)std::min<uint64_t>(odd_bytes - at, 1u << 30));
	if ((uint32_t)c != H.crc) { *flags = OA_F_CRC; return -1; }
	return 0;
}

// ---- the folder ---------------------------------------------------------------------------------------------------------------------------
#ifndef MCOM_ENTROPY_HOST_ONLY
namespace {
struct Dev {
	mcom_ctx *ctx = nullptr; mcom_odd_index *idx = nullptr; std::vector<void*> v;
	~Dev() { if (ctx) (void)mcom_sync(ctx); if (idx) mcom_odd_index_free(ctx, idx); for (void *p : v) (void)hipFree(p); if (ctx) mcom_destroy(ctx); }
	template <class T> T *alloc(size_t n) { void *p = nullptr; if (hipMalloc(&p, (n ? n : 1) * sizeof(T) + 16) != hipSuccess) return nullptr; v.push_back(p); return (T*)p; }
	template <class T> T *upload(const T *h, size_t n) { T *d = alloc<T>(n); if (d && n && hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr; return d; }
};
// index, hits, member and residual on GPU `device`
int device_encode(int device, const FolderText &F, const std::vector<uint8_t> &odd, const std::vector<uint64_t> &off, std::vector<uint8_t> &member, std::vector<uint8_t> &residual,
                  char *err, size_t err_cap)
{
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev || hipSetDevice(device) != hipSuccess) return fail(err, err_cap, "no such GPU");
	Dev D;
	if (mcom_create(&D.ctx, device, nullptr) != MCOM_OK) { D.ctx = nullptr; return fail(err, err_cap, "cannot create a context on the GPU"); }
	const uint64_t n_odd = off.size() - 1;
	// T on the card: the ref.bin images go up as they are and are appended there, set after set
	const uint64_t t_words = oa_words(F.bases);
	uint64_t *d_t = D.alloc<uint64_t>((size_t)t_words);
	if (!d_t || hipMemset(d_t, 0, (size_t)t_words * 8) != hipSuccess) return fail(err, err_cap, "no room on the card");
	uint64_t at = 0;
	for (size_t th = 0; th < F.refs.size(); ++th) {
		const uint8_t *d_ref = D.upload(F.refs[th].data(), F.refs[th].size());
		if (!d_ref) return fail(err, err_cap, "no room on the card");
		if (mcom_odd_text_append(D.ctx, d_t, t_words, at, d_ref, F.refs[th].size(), F.nb[th])) return fail(err, err_cap, mcom_last_error(D.ctx));
		at += F.nb[th];
	}
	const uint8_t *d_odd = D.upload(odd.data(), odd.size());
	const uint64_t *d_off = D.upload(off.data(), off.size());
	uint64_t *d_hits = D.alloc<uint64_t>(n_odd);
	if (!d_odd || !d_off || !d_hits) return fail(err, err_cap, "no room on the card");
	uint64_t ml = 0, rl = 0;
	if (mcom_odd_index_build(D.ctx, d_t, F.bases, &D.idx) || mcom_odd_align(D.ctx, D.idx, d_t, F.bases, d_odd, d_off, n_odd, d_hits) ||
	    mcom_odd_align_encode(D.ctx, d_hits, d_odd, d_off, n_odd, d_t, F.bases, nullptr, 0, &ml, nullptr, 0, &rl)) return fail(err, err_cap, mcom_last_error(D.ctx));
	uint8_t *d_member = D.alloc<uint8_t>(ml), *d_res = D.alloc<uint8_t>(rl);
	if (!d_member || !d_res) return fail(err, err_cap, "no room on the card");
	if (mcom_odd_align_encode(D.ctx, d_hits, d_odd, d_off, n_odd, d_t, F.bases, d_member, ml, &ml, d_res, rl, &rl)) return fail(err, err_cap, mcom_last_error(D.ctx));
	member.resize(ml); residual.resize(rl);
	if ((ml && hipMemcpy(member.data(), d_member, ml, hipMemcpyDeviceToHost) != hipSuccess) || (rl && hipMemcpy(residual.data(), d_res, rl, hipMemcpyDeviceToHost) != hipSuccess))
		return fail(err, err_cap, "download failed");
	return 0;
}
}  // namespace
#endif

extern "C" int mcomh_odd_align_folder(const char *folder, int device, uint64_t *n_odd_out, uint64_t *n_aligned_out, uint64_t *residual_out, char *err, size_t err_cap)
{
	if (!folder) return fail(err, err_cap, "null pointer");
	try {
		const std::string dir(folder);
		std::string why;
		FolderText F;
		std::vector<uint8_t> len, odd, member, residual;
		std::vector<uint64_t> off;
		if (mcom_streams::exists(dir + "/odd.aln")) return fail(err, err_cap, "the folder holds odd.aln already");
		if (!mcom_streams::slurp(dir + "/len.bin", len) || !mcom_streams::slurp(dir + "/odd.seq", odd)) return fail(err, err_cap, "no len.bin and odd.seq: not the stream files of an archive made with -V");
		if (!folder_text(dir, F, why, device < 0)) return fail(err, err_cap, why.c_str());
		odd_offsets(len, F.L, off);
		const uint64_t n_odd = off.size() - 1;
		if (off.back() != odd.size()) return fail(err, err_cap, "the lengths of len.bin do not add up to the size of odd.seq");
		for (uint8_t c : odd) if (oa_code(c) > 4) return fail(err, err_cap, "odd.seq holds a byte outside ACGTN");
		if (device < 0) {
			mcomh_odd_index *idx = nullptr;
			std::vector<uint64_t> hits((size_t)n_odd);
			if (mcomh_odd_index_build(F.t.data(), F.bases, &idx)) return fail(err, err_cap, "cannot build the seed index");
			const int rc = mcomh_odd_align(idx, F.t.data(), F.bases, odd.data(), off.data(), n_odd, hits.data());
			mcomh_odd_index_free(idx);
			uint64_t ml = 0, rl = 0;
			if (rc || mcomh_odd_align_encode(hits.data(), odd.data(), off.data(), n_odd, F.t.data(), F.bases, nullptr, 0, &ml, nullptr, 0, &rl)) return fail(err, err_cap, "the aligner failed");
			member.resize((size_t)ml); residual.resize((size_t)rl);
			if (mcomh_odd_align_encode(hits.data(), odd.data(), off.data(), n_odd, F.t.data(), F.bases, member.data(), ml, &ml, residual.data(), rl, &rl)) return fail(err, err_cap, "the aligner failed");
		} else {
#ifndef MCOM_ENTROPY_HOST_ONLY
			if (device_encode(device, F, odd, off, member, residual, err, err_cap)) return -1;
#else
			return fail(err, err_cap, "built without the device route");
#endif
		}
		uint64_t n_aligned = 0;
		if (!member.empty()) {
			n_aligned = oa_get(member.data() + 32, 8);
			if (!write_file(dir + "/odd.aln", member.data(), member.size())) return fail(err, err_cap, "cannot write odd.aln");
			if (!write_file(dir + "/odd.seq", residual.data(), residual.size())) { remove((dir + "/odd.aln").c_str()); return fail(err, err_cap, "cannot rewrite odd.seq"); }
		}
		if (n_odd_out) *n_odd_out = n_odd;
		if (n_aligned_out) *n_aligned_out = n_aligned;
		if (residual_out) *residual_out = residual.size();
		return 0;
	} catch (...) { return fail(err, err_cap, "out of memory"); }
}

// ---- the decoders: a folder that holds odd.aln (the residual may have been removed as an empty file).  P.len is loaded; P.odd_seq becomes the full text.
bool mcom_odd_align_present(const char *folder) { return mcom_streams::exists(std::string(folder) + "/odd.aln"); }

bool mcom_odd_align_rebuild(const char *folder, int L, McomRaggedParts &P, std::string &why)
{
	try {
	const std::string dir(folder);
	std::vector<uint8_t> member, residual;
	if (!mcom_streams::slurp(dir + "/odd.aln", member)) { why = "cannot read odd.aln"; return false; }
	(void)mcom_streams::slurp(dir + "/odd.seq", residual);                     // (missing: empty)
	FolderText F;
	if (!folder_text(dir, F, why)) return false;
	if (F.L != L) { why = "info.txt states another read length"; return false; }
	std::vector<uint64_t> off;
	odd_offsets(P.len, L, off);
	uint32_t flags = 0;
	P.odd_seq.assign((size_t)off.back(), 0);
	if (mcomh_odd_align_decode(member.data(), member.size(), F.t.data(), F.bases, residual.data(), residual.size(), off.data(), off.size() - 1, P.odd_seq.data(), &flags)) {
		why = flags ? oa_refusal(flags) : "odd.aln: refused";
		return false;
	}
	return true;
	} catch (...) { why = "odd.aln: no memory for the contigs' bases and the odd text the side members state"; return false; }
}
