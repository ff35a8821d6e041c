// tests/fuzz_mate_names.cpp -- the host twin of `.mcn` kind 2 (host/mcom_names.cpp: mcomh_name_encode_mate / mcomh_name_decode_mate, DESIGN.md
// section 3.12) under AddressSanitizer and UBSan: `make -C minicom_amd/host fuzz_mate_names && minicom_amd/lib/fuzz_mate_names`.  A stand-alone
// CPU program, run by hand; never on a GPU machine and never loaded into Python.
//   1. round trips of generated pairs of name texts (the three pair styles, names that differ at random, degenerate ones, every kind of
//      third line); the member is never larger than mcomh_name_encode's, and a kind-2 member is refused without its mate
//   2. hostile members under the true mate: every truncation of a kind-2 member, seeded bit flips
//   3. hostile mates under an intact member: bit flips, truncations and random texts -- as they are (refused by the mate's crc), and with
//      the member's mate crc set to theirs, so that the walk itself meets a mate it was not made for
// Each hostile call must refuse or decode, never crash; what decodes under the true crc must be the text.  Prints the counts; exit status 1 when a
// round trip fails.
#include "../include/mcom_host.h"
#include "mcom_inflate.hpp"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

// name i of file `file` (1 or 2)
static std::string make_name(int style, uint64_t i, int file, uint32_t a, uint32_t b)
{
	char s[320];
	switch (style) {
	case 0: snprintf(s, sizeof s, "A00123:45:HXXXXDSXX:%u:%u:%u:%u %d:N:0:ACGTACGT+TTGCAAGC", 1 + (unsigned)(i / 900), 1101 + (unsigned)(i / 300 % 20), a, b, file); return s;
	case 1: snprintf(s, sizeof s, "HWUSI-EAS100R:6:73:%u:%u#0/%d", a, b, file); return s;
	case 2: snprintf(s, sizeof s, "SRR001666.%llu 071112_SLXA-EAS1_s_7:5:%u:%u length=36", (unsigned long long)i + 1, a % 1000, b % 1000); return s;
	case 3: { std::string r; const uint32_t runs = a % 40; uint64_t st = (uint64_t)b * 2654435761u + (uint64_t)file * (a % 3 == 0);
	          for (uint32_t j = 0; j < runs && r.size() < 240; ++j) { st = st * 6364136223846793005ull + 1442695040888963407ull; snprintf(s, sizeof s, "%u%c", (unsigned)(st >> 40) % (j % 4 ? 1000u : 4000000000u), "._:/ "[(st >> 33) % 5]); r += s; }
	          return r; }
	default: { static const char *edge[] = {"", "0", "007", "999999999", "1000000000", "a999999998", "a999999999", "a", "00", "4294967295", "a1b2", "a1b2c3d4"}; return edge[(a + (uint32_t)file * (b % 5)) % 12]; }
	}
}

static void make_pair(int style, uint64_t n, std::vector<uint8_t> &text, std::vector<uint8_t> &mate)
{
	text.clear(); mate.clear();
	for (uint64_t i = 0; i < n; ++i) {
		const uint32_t a = rnd(), b = rnd();
		const int st = style == 5 ? (int)(rnd() % 5) : style;
		for (int file = 1; file <= 2; ++file) {
			std::vector<uint8_t> &t = file == 1 ? mate : text;
			const std::string nm = make_name(st, i, file, a % 30000, b % 200000);
			t.insert(t.end(), nm.begin(), nm.end()); t.push_back('\n');
			const uint32_t k = rnd() % 4;
			if (k == 1) t.insert(t.end(), nm.begin(), nm.end());
			else if (k == 2) { const std::string p = make_name(4, i, file, rnd(), rnd()); t.insert(t.end(), p.begin(), p.end()); }
			t.push_back('\n');
		}
	}
}

static bool round_trip(const std::vector<uint8_t> &text, const std::vector<uint8_t> &mate, uint64_t n, std::vector<uint8_t> &member, uint64_t &kind2)
{
	member.resize(mcomh_name_bound(text.size()));
	std::vector<uint8_t> alone(member.size());
	uint64_t len = 0, alone_len = 0, bad = 0;
	if (mcomh_name_encode_mate(text.data(), text.size(), n, mate.data(), mate.size(), member.data(), member.size(), &len, &bad)) return false;
	if (mcomh_name_encode(text.data(), text.size(), n, alone.data(), alone.size(), &alone_len, &bad) || len > alone_len) return false;
	member.resize(len);
	uint64_t gn = 0, gt = 0;
	if (mcomh_name_info_mate(member.data(), member.size(), &gn, &gt) || gn != n || gt != text.size()) return false;
	std::vector<uint8_t> back(gt + 1);
	if (mcomh_name_decode_mate(member.data(), member.size(), mate.data(), mate.size(), back.data(), gt, &gt, &gn)) return false;
	if (gt != text.size() || (gt && memcmp(back.data(), text.data(), gt))) return false;
	if (member[5] == 2) {
		++kind2;
		if (len >= alone_len) return false;
		if (!mcomh_name_info(member.data(), member.size(), &gn, &gt)) return false;                                    // no mate: refused
		if (!mcomh_name_decode(member.data(), member.size(), back.data(), text.size(), &gt, &gn)) return false;
	} else if (len != alone_len || memcmp(member.data(), alone.data(), len)) return false;
	return true;
}

// must_be: when the call decodes, the text it has to give (NULL: anything)
static bool hostile(const std::vector<uint8_t> &m, const std::vector<uint8_t> &mate, const std::vector<uint8_t> *must_be, uint64_t &refused, uint64_t &decoded)
{
	uint64_t n = 0, t = 0;
	if (mcomh_name_info_mate(m.data(), m.size(), &n, &t) || t > ((uint64_t)1 << 26)) { ++refused; return true; }
	std::vector<uint8_t> out(t + 1);
	if (mcomh_name_decode_mate(m.data(), m.size(), mate.data(), mate.size(), out.data(), t, &t, &n)) { ++refused; return true; }
	++decoded;
	return !must_be || (t == must_be->size() && !memcmp(out.data(), must_be->data(), t));
}

int main()
{
	uint64_t trips = 0, failed = 0, kind2 = 0, refused = 0, decoded = 0, wrong = 0;
	for (int round = 0; round < 420; ++round) {
		const int style = round % 6;
		const uint64_t n = round < 12 ? (uint64_t)round / 2 : rnd() % (round % 60 == 0 ? 3000 : 600);
		std::vector<uint8_t> text, mate, member;
		make_pair(style, n, text, mate);
		++trips;
		if (!round_trip(text, mate, n, member, kind2)) { ++failed; fprintf(stderr, "round %d (style %d, %llu records) failed\n", round, style, (unsigned long long)n); continue; }
		if ((round == 60 || round == 61 || round == 62 || round == 65) && member[5] == 2) {
			// hostile members under the true mate
			for (size_t cut = 0; cut < member.size(); cut += member.size() > 4000 ? 37 : 1) { std::vector<uint8_t> m(member.begin(), member.begin() + cut); if (!hostile(m, mate, &text, refused, decoded)) ++wrong; }
			for (int f = 0; f < 2000; ++f) {
				std::vector<uint8_t> m = member; const size_t at = rnd() % m.size(); m[at] ^= (uint8_t)(1u << (rnd() % 8));
				if (!hostile(m, mate, at >= 24 && at < 28 ? nullptr : &text, refused, decoded)) ++wrong;       // (a flip in the text's own crc may meet a flip-free decode: not here, but the claim is not made)
			}
			// hostile mates under the intact member
			for (int f = 0; f < 1500; ++f) {
				std::vector<uint8_t> hm = mate;
				const int how = f % 5;
				if (how == 0) hm[rnd() % hm.size()] ^= (uint8_t)(1u << (rnd() % 8));
				else if (how == 1) hm.resize(rnd() % hm.size());
				else if (how == 2) for (int k = 0; k < 20; ++k) hm[rnd() % hm.size()] = (uint8_t)rnd();
				else if (how == 3) for (int k = 0; k < 8; ++k) hm[rnd() % hm.size()] = (uint8_t)"\n0 9:"[rnd() % 5];
				else { std::vector<uint8_t> t2, m2; make_pair((int)(rnd() % 5), n, t2, m2); hm = m2; }
				if (!hostile(member, hm, &text, refused, decoded)) ++wrong;
				std::vector<uint8_t> m = member;
				const uint32_t crc = hm.empty() ? 0 : mcom_crc32(0, hm.data(), hm.size());
				m[88] = (uint8_t)crc; m[89] = (uint8_t)(crc >> 8); m[90] = (uint8_t)(crc >> 16); m[91] = (uint8_t)(crc >> 24);
				if (!hostile(m, hm, &text, refused, decoded)) ++wrong;                                    // (what decodes passed the text's crc)
			}
		}
	}
	printf("fuzz_mate_names: %llu round trips (%llu failed, %llu of kind 2), %llu hostile calls refused, %llu decoded (%llu to another text)\n", (unsigned long long)trips,
	       (unsigned long long)failed, (unsigned long long)kind2, (unsigned long long)refused, (unsigned long long)decoded, (unsigned long long)wrong);
	return failed || wrong ? 1 : 0;
}
