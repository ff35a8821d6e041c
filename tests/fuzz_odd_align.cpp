// tests/fuzz_odd_align.cpp -- the host side of `minicom -p -V -A` as a stand-alone program, built with
// AddressSanitizer and UBSan by `make -C minicom_amd/host fuzz_odd_align` (CPU only; tests/test_odd_align.py builds and runs it).
// fuzz_odd_align DIR, where DIR/arch is a folder of stream files with len.bin, odd.aln and the residual odd.seq (the test makes it):
//   1. texts made here: index, hits, member and residual by the twins in buffers of exactly the room needed, decoded again to the text;
//   2. mcomh_odd_align_decode over the folder's member with seeded byte changes, cut short and grown, over a changed residual and over
//      changed record lengths, every buffer of exact size: refused with a reason or decoded to a text of the stated CRC, never outside;
//   3. mcom_ragged_load over the folder with the same damage done to odd.aln, odd.seq and len.bin: refused with words, or loaded.
#include "../include/mcom_host.h"
#include "../minicom_amd/host/mcom_ragged.hpp"
#include <sys/stat.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static uint64_t g_x = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return g_x; }
typedef std::vector<uint8_t> Bytes;

static bool slurp(const std::string &p, Bytes &out)
{
	FILE *f = fopen(p.c_str(), "rb");
	if (!f) return false;
	out.clear();
	uint8_t buf[65536]; size_t got;
	while ((got = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + got);
	fclose(f);
	return true;
}
static bool spill(const std::string &p, const Bytes &b)
{
	FILE *f = fopen(p.c_str(), "wb");
	if (!f) return false;
	const bool ok = b.empty() || fwrite(b.data(), 1, b.size(), f) == b.size();
	return fclose(f) == 0 && ok;
}
// a heap block of exactly n bytes (never a vector's spare capacity): what the sanitizer watches the ends of
struct Exact {
	uint8_t *p; size_t n;
	explicit Exact(const Bytes &b) : p((uint8_t*)malloc(b.size() ? b.size() : 1)), n(b.size()) { if (n) memcpy(p, b.data(), n); }
	explicit Exact(size_t bytes) : p((uint8_t*)malloc(bytes ? bytes : 1)), n(bytes) {}
	~Exact() { free(p); }
	Exact(const Exact&) = delete;
};
struct Text { uint64_t *t; uint64_t bases; Text() : t(nullptr), bases(0) {} ~Text() { free(t); } };
static void make_text(Text &T, const uint8_t *ref, uint64_t ref_bytes, uint64_t bases)
{
	const size_t words = (size_t)((bases + 31) / 32 + 1);
	T.t = (uint64_t*)calloc(words, 8); T.bases = bases;
	mcomh_odd_text_append(T.t, 0, ref, ref_bytes, bases);
}

static void mutate(Bytes &b, int kind)
{
	if (kind == 0 && !b.empty()) for (int k = 1 + (int)(rnd() % 3); k > 0; --k) b[rnd() % b.size()] = (uint8_t)rnd();
	if (kind == 1 && !b.empty()) b[rnd() % b.size()] ^= (uint8_t)(1u << (rnd() % 8));
	if (kind == 2 && !b.empty()) b.resize(rnd() % b.size());
	if (kind == 3) for (int k = 1 + (int)(rnd() % 70); k > 0; --k) b.push_back((uint8_t)rnd());
	if (kind == 4 && b.size() >= 64) b[24 + rnd() % 40] = (uint8_t)rnd();          // the counts of the header
}

// ---- 1. round trips of texts made here ------------------------------------------------------------------------------------------------------
static int self_made(size_t &n_members)
{
	for (int round = 0; round < 60; ++round) {
		const uint64_t bases = round % 7 == 0 ? rnd() % 40 : 200 + rnd() % 3000;
		Bytes ref((size_t)(bases + 3) / 4);
		for (uint8_t &v : ref) v = (uint8_t)rnd();
		Text T;
		make_text(T, ref.data(), ref.size(), bases);
		Bytes odd; std::vector<uint64_t> off(1, 0);
		const uint64_t n_odd = rnd() % 40;
		for (uint64_t r = 0; r < n_odd; ++r) {
			const uint32_t l = 1 + (uint32_t)(rnd() % 256);
			if (rnd() % 3 && l <= bases) {                                     // a piece of T, either strand, a few changes
				const uint64_t p = rnd() % (bases - l + 1);
				const bool rev = rnd() & 1;
				for (uint32_t j = 0; j < l; ++j) { const uint64_t b = p + (rev ? l - 1 - j : j); uint32_t c = (uint32_t)(T.t[b >> 5] >> (2 * (b & 31))) & 3u; odd.push_back("ACGT"[rev ? 3 - c : c]); }
				for (int k = (int)(rnd() % 4); k > 0; --k) odd[odd.size() - 1 - rnd() % l] = "ACGTN"[rnd() % 5];
			} else for (uint32_t j = 0; j < l; ++j) odd.push_back("ACGTN"[rnd() % 5]);
			off.push_back(odd.size());
		}
		mcomh_odd_index *idx = nullptr;
		if (mcomh_odd_index_build(T.t, T.bases, &idx)) { fprintf(stderr, "round %d: no index\n", round); return 1; }
		Exact text(odd), hits((size_t)n_odd * 8);
		const int rc = mcomh_odd_align(idx, T.t, T.bases, text.p, off.data(), n_odd, (uint64_t*)hits.p);
		mcomh_odd_index_free(idx);
		uint64_t ml = 0, rl = 0;
		if (rc || mcomh_odd_align_encode((const uint64_t*)hits.p, text.p, off.data(), n_odd, T.t, T.bases, nullptr, 0, &ml, nullptr, 0, &rl)) { fprintf(stderr, "round %d: the twins refuse their own text\n", round); return 1; }
		Exact member((size_t)ml), res((size_t)rl);
		if (mcomh_odd_align_encode((const uint64_t*)hits.p, text.p, off.data(), n_odd, T.t, T.bases, member.p, ml, &ml, res.p, rl, &rl)) { fprintf(stderr, "round %d: encode failed\n", round); return 1; }
		if (!ml) { if (rl != odd.size() || (rl && memcmp(res.p, text.p, rl))) { fprintf(stderr, "round %d: no member, and the residual is not the text\n", round); return 1; } continue; }
		++n_members;
		Exact out(odd.size());
		uint32_t flags = 0;
		if (mcomh_odd_align_decode(member.p, ml, T.t, T.bases, res.p, rl, off.data(), n_odd, out.p, &flags) || (odd.size() && memcmp(out.p, text.p, odd.size()))) {
			fprintf(stderr, "round %d: the member does not decode to its text (%s)\n", round, mcomh_odd_align_refusal(flags));
			return 1;
		}
	}
	return 0;
}

// the bases the contigs of a beg_pos.bin image hold: per contig its last begin position + L
static uint64_t contig_bases(const Bytes &pos, int L)
{
	size_t pp = 0; uint64_t bases = 0;
	while (pp + 4 <= pos.size()) {
		uint32_t num; memcpy(&num, pos.data() + pp, 4); pp += 4;
		uint64_t p = 0;
		for (uint32_t q = 0; q < num && pp + 2 <= pos.size(); ++q) { uint16_t d; memcpy(&d, pos.data() + pp, 2); pp += 2; p += d; }
		if (num) bases += p + (uint64_t)L;
	}
	return bases;
}

int main(int argc, char **argv)
{
	size_t n_members = 0;
	if (self_made(n_members)) return 1;
	if (argc < 2) { printf("fuzz_odd_align ok: %zu members made here (no folder given)\n", n_members); return 0; }
	const std::string dir = std::string(argv[1]) + "/arch", mut = std::string(argv[1]) + "/mut";
	Bytes member, residual, len, ref, pos, info;
	if (!slurp(dir + "/odd.aln", member) || !slurp(dir + "/odd.seq", residual) || !slurp(dir + "/len.bin", len) || !slurp(dir + "/ref.bin.0", ref) || !slurp(dir + "/beg_pos.bin.0", pos) ||
	    !slurp(dir + "/info.txt", info)) { fprintf(stderr, "no folder of stream files with odd.aln in %s\n", dir.c_str()); return 1; }
	info.push_back(0);
	const int L = atoi((const char*)info.data());
	Text T;
	make_text(T, ref.data(), ref.size(), contig_bases(pos, L));
	auto offsets = [&](const Bytes &lens, std::vector<uint64_t> &off, uint64_t &n_even) {
		off.assign(1, 0); n_even = 0;
		for (uint8_t b : lens) { if ((int)b + 1 == L) ++n_even; else off.push_back(off.back() + (uint64_t)b + 1); }
	};
	std::vector<uint64_t> off; uint64_t n_even = 0;
	offsets(len, off, n_even);
	// ---- 2. the decode twin
	size_t n_ok = 0, n_refused = 0;
	for (int round = 0; round < 3000; ++round) {
		Bytes m = member, r = residual, l = len;
		const int target = round % 8;
		if (round) { if (target < 5) mutate(m, round % 5); else if (target == 5) mutate(r, (int)(rnd() % 4)); else if (target == 6) mutate(l, 1); else { mutate(m, 1); mutate(l, 1); } }
		std::vector<uint64_t> o; uint64_t ne = 0;
		offsets(l, o, ne);
		Exact em(m), er(r), out((size_t)o.back());
		uint32_t flags = 0;
		const int rc = mcomh_odd_align_decode(em.p, em.n, T.t, T.bases, er.p, er.n, o.data(), o.size() - 1, out.p, &flags);
		if (!rc && flags) { fprintf(stderr, "round %d: decoded with flags %u\n", round, flags); return 1; }
		if (rc && !flags) { fprintf(stderr, "round %d: refused without a reason\n", round); return 1; }
		if (!round && rc) { fprintf(stderr, "the folder's own member is refused: %s\n", mcomh_odd_align_refusal(flags)); return 1; }
		if (rc) ++n_refused; else ++n_ok;
	}
	// ---- 3. the loader of the decoders
	mkdir(mut.c_str(), 0700);
	if (!spill(mut + "/info.txt", Bytes(info.begin(), info.end() - 1)) || !spill(mut + "/ref.bin.0", ref) || !spill(mut + "/beg_pos.bin.0", pos)) return 1;
	size_t l_ok = 0, l_refused = 0;
	for (int round = 0; round < 300; ++round) {
		Bytes m = member, r = residual, l = len, rf = ref, ps = pos;
		const int target = round % 6;
		if (round) { if (target < 3) mutate(m, round % 5); else if (target == 3) mutate(r, (int)(rnd() % 4)); else if (target == 4) mutate(l, 1); else { mutate(ps, (int)(rnd() % 3)); mutate(rf, 2); } }
		if (!spill(mut + "/odd.aln", m) || !spill(mut + "/odd.seq", r) || !spill(mut + "/len.bin", l) || !spill(mut + "/ref.bin.0", rf) || !spill(mut + "/beg_pos.bin.0", ps)) return 1;
		std::vector<uint64_t> o; uint64_t ne = 0;
		offsets(l, o, ne);
		McomRaggedParts P;
		std::string why;
		const bool ok = mcom_ragged_load(mut.c_str(), L, ne, false, P, why);
		if (!ok && why.empty()) { fprintf(stderr, "round %d: refused without words\n", round); return 1; }
		if (ok && P.odd_seq.size() != o.back()) { fprintf(stderr, "round %d: loaded a text of another size\n", round); return 1; }
		if (!round && !ok) { fprintf(stderr, "the folder itself is refused: %s\n", why.c_str()); return 1; }
		if (ok) ++l_ok; else ++l_refused;
	}
	for (const char *f : {"/odd.aln", "/odd.seq", "/len.bin", "/info.txt", "/ref.bin.0", "/beg_pos.bin.0"}) remove((mut + f).c_str());
	remove(mut.c_str());
	printf("fuzz_odd_align ok: %zu members made here; decode twin %zu decoded, %zu refused; loader %zu loaded, %zu refused\n", n_members, n_ok, n_refused, l_ok, l_refused);
	return 0;
}
