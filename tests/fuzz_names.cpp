// tests/fuzz_names.cpp -- the host twin of the read-name coder alone (host/mcom_names.cpp over mcom_bwt.cpp and mcom_entropy.cpp) under
// AddressSanitizer and UBSan: `make -C minicom_amd/host fuzz_names && minicom_amd/lib/fuzz_names [DIR]`.  A stand-alone CPU program,
// run by hand; never on a GPU machine and never loaded into Python.
//   1. round trips of generated name texts (instrument-style names, degenerate ones, every kind of third line)
//   2. hostile members: every truncation of a member, seeded bit flips, and every file of DIR (written by a test run from
//      tests/name_cases.py; may be absent) -- each must be refused or decode to something, never crash
// Prints the counts; exit status 1 when a round trip fails.
#include "../include/mcom_host.h"
#include <cstdio>
#include <cstring>
#include <dirent.h>
#include <string>
#include <vector>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

static std::string make_name(int style, uint64_t i, uint32_t &x)
{
	char b[320];
	switch (style) {
	case 0: x += rnd() % 40; snprintf(b, sizeof b, "A00123:45:HXXXXDSXX:%u:%u:%u:%u 1:N:0:ACGTACGT+TTGCAAGC", 1 + (unsigned)(i / 900), 1101 + (unsigned)(i / 300 % 20), x, 1000 + rnd() % 199001); return b;
	case 1: snprintf(b, sizeof b, "SRR001666.%llu 071112_SLXA-EAS1_s_7:5:%llu:%u:%u length=36", (unsigned long long)i + 1, (unsigned long long)(i / 5000 + 1), rnd() % 1000, rnd() % 1000); return b;
	case 2: { std::string s; const uint32_t len = rnd() % 256; for (uint32_t j = 0; j < len; ++j) { uint8_t c = (uint8_t)rnd(); if (c == '\n') c = '0'; s.push_back((char)c); } return s; }
	case 3: { std::string s; const uint32_t runs = rnd() % 40; for (uint32_t j = 0; j < runs && s.size() < 240; ++j) { snprintf(b, sizeof b, "%u%c", rnd() % 3 ? rnd() % 1000 : rnd(), "._:/ "[rnd() % 5]); s += b; } return s; }
	default: { static const char *edge[] = {"", "0", "007", "999999999", "1000000000", "a999999998", "a999999999", "a", "00", "4294967295"}; return edge[rnd() % 10]; }
	}
}

static bool round_trip(const std::vector<uint8_t> &text, uint64_t n, std::vector<uint8_t> &member)
{
	member.resize(mcomh_name_bound(text.size()));
	uint64_t len = 0, bad = 0;
	if (mcomh_name_encode(text.data(), text.size(), n, member.data(), member.size(), &len, &bad)) return false;
	member.resize(len);
	uint64_t gn = 0, gt = 0;
	if (mcomh_name_info(member.data(), member.size(), &gn, &gt) || gn != n || gt != text.size()) return false;
	std::vector<uint8_t> back(gt + 1);
	if (mcomh_name_decode(member.data(), member.size(), back.data(), gt, &gt, &gn)) return false;
	return gt == text.size() && (gt == 0 || !memcmp(back.data(), text.data(), gt));
}

static void hostile(const std::vector<uint8_t> &m, uint64_t &refused, uint64_t &decoded)
{
	uint64_t n = 0, t = 0;
	if (mcomh_name_info(m.data(), m.size(), &n, &t) || t > ((uint64_t)1 << 26)) { ++refused; return; }
	std::vector<uint8_t> out(t + 1);
	if (mcomh_name_decode(m.data(), m.size(), out.data(), t, &t, &n)) ++refused; else ++decoded;
}

int main(int argc, char **argv)
{
	uint64_t trips = 0, failed = 0, refused = 0, decoded = 0;
	std::vector<uint8_t> keep;
	for (int round = 0; round < 600; ++round) {
		const int style = round % 5;
		const uint64_t n = round < 10 ? (uint64_t)round : rnd() % (round % 50 == 0 ? 3000 : 700);
		std::vector<uint8_t> text, member;
		uint32_t x = 1000;
		for (uint64_t i = 0; i < n; ++i) {
			const std::string nm = make_name(round % 7 == 6 ? (int)(rnd() % 5) : style, i, x);
			text.insert(text.end(), nm.begin(), nm.end()); text.push_back('\n');
			const uint32_t k = rnd() % 4;
			if (k == 1) text.insert(text.end(), nm.begin(), nm.end());
			else if (k == 2) { const std::string p = make_name(4, i, x); text.insert(text.end(), p.begin(), p.end()); }
			text.push_back('\n');
		}
		++trips;
		if (!round_trip(text, n, member)) { ++failed; fprintf(stderr, "round %d (%llu records) failed\n", round, (unsigned long long)n); }
		if (round == 3 || round == 120) {
			// kind 0 and whatever the choice took: every truncation, then bit flips
			for (size_t cut = 0; cut < member.size(); cut += member.size() > 4000 ? 37 : 1) { std::vector<uint8_t> m(member.begin(), member.begin() + cut); hostile(m, refused, decoded); }
			for (int f = 0; f < 3000; ++f) { std::vector<uint8_t> m = member; m[rnd() % m.size()] ^= (uint8_t)(1u << (rnd() % 8)); hostile(m, refused, decoded); }
		}
	}
	if (argc > 1) {
		if (DIR *d = opendir(argv[1])) {
			while (dirent *e = readdir(d)) {
				if (e->d_name[0] == '.') continue;
				const std::string path = std::string(argv[1]) + "/" + e->d_name;
				std::vector<uint8_t> m;
				if (FILE *f = fopen(path.c_str(), "rb")) { uint8_t buf[4096]; size_t got; while ((got = fread(buf, 1, sizeof buf, f)) > 0) m.insert(m.end(), buf, buf + got); fclose(f); }
				const uint64_t before = decoded;
				hostile(m, refused, decoded);
				if (decoded != before) { fprintf(stderr, "%s decoded: it must be refused\n", path.c_str()); ++failed; }
			}
			closedir(d);
		}
	}
	printf("fuzz_names: %llu round trips (%llu failed), %llu hostile members refused, %llu decoded\n", (unsigned long long)trips, (unsigned long long)failed,
	       (unsigned long long)refused, (unsigned long long)decoded);
	return failed ? 1 : 0;
}
