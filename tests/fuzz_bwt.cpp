// tests/fuzz_bwt.cpp -- the host twin of the block-sorting coder (host/mcom_bwt.cpp) as a stand-alone program, built with AddressSanitizer
// and UBSan by `make -C minicom_amd/host fuzz_bwt` (CPU only).  fuzz_bwt DIR: every file DIR/*.raw is coded and decoded back; every file
// DIR/*.bad must be refused; every file DIR/*.good must decode; then every truncation and 2000 seeded bit flips of the first .good member
// are decoded -- whatever the verdict, no read or write may leave a buffer, and what is accepted must be the original.
#include "../include/mcom_host.h"
#include <dirent.h>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static std::vector<uint8_t> slurp(const std::string &p)
{
	std::vector<uint8_t> v;
	FILE *f = fopen(p.c_str(), "rb");
	if (!f) return v;
	uint8_t buf[65536]; size_t n;
	while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
	fclose(f);
	return v;
}
static bool ends_with(const std::string &s, const char *e) { const size_t n = strlen(e); return s.size() >= n && !s.compare(s.size() - n, n, e); }

// 0 and the bytes, or -1
static int decode(const std::vector<uint8_t> &m, std::vector<uint8_t> &out)
{
	uint64_t raw_len = 0, got = 0;
	if (mcomh_bwt_raw_len(m.data(), m.size(), &raw_len) || raw_len > ((uint64_t)1 << 30)) return -1;
	out.assign(raw_len, 0);                                                     // exactly the room asked for: ASan guards its ends
	if (mcomh_bwt_decode(m.data(), m.size(), out.data(), out.size(), &got) || got != raw_len) return -1;
	return 0;
}

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: fuzz_bwt DIR\n"); return 2; }
	const std::string dir = argv[1];
	std::vector<std::string> names;
	DIR *d = opendir(dir.c_str());
	if (!d) return 2;
	while (dirent *e = readdir(d)) names.push_back(e->d_name);
	closedir(d);
	size_t n_raw = 0, n_bad = 0, n_good = 0, n_hostile = 0, n_accepted = 0;
	std::vector<uint8_t> first_good, first_raw, out;
	for (const std::string &nm : names) {
		const std::vector<uint8_t> v = slurp(dir + "/" + nm);
		if (ends_with(nm, ".raw")) {
			std::vector<uint8_t> m(mcomh_bwt_bound(v.size()));
			uint64_t len = 0;
			if (mcomh_bwt_encode(v.data(), v.size(), m.data(), m.size(), &len)) { fprintf(stderr, "%s: encode failed\n", nm.c_str()); return 1; }
			m.resize(len);
			if (decode(m, out) || out != v) { fprintf(stderr, "%s: round trip failed\n", nm.c_str()); return 1; }
			++n_raw;
		} else if (ends_with(nm, ".bad")) {
			if (!decode(v, out)) { fprintf(stderr, "%s: accepted\n", nm.c_str()); return 1; }
			++n_bad;
		} else if (ends_with(nm, ".good")) {
			if (decode(v, out)) { fprintf(stderr, "%s: refused\n", nm.c_str()); return 1; }
			if (first_good.empty() || nm < "b") { first_good = v; first_raw = out; }
			++n_good;
		}
	}
	if (!first_good.empty()) {
		for (size_t cut = 0; cut < first_good.size(); ++cut, ++n_hostile) {
			std::vector<uint8_t> m(first_good.begin(), first_good.begin() + cut);
			if (!decode(m, out)) { fprintf(stderr, "cut@%zu accepted\n", cut); return 1; }
		}
		uint64_t x = 88172645463325252ull;
		for (int k = 0; k < 2000; ++k, ++n_hostile) {
			x ^= x << 13; x ^= x >> 7; x ^= x << 17;
			std::vector<uint8_t> m = first_good;
			const uint64_t bit = x % (8 * m.size());
			m[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
			if (!decode(m, out)) { ++n_accepted; if (out != first_raw) { fprintf(stderr, "flip@%llu accepted with other bytes\n", (unsigned long long)bit); return 1; } }
		}
	}
	printf("fuzz_bwt ok: %zu round trips, %zu refused, %zu decoded, %zu hostile (%zu harmless)\n", n_raw, n_bad, n_good, n_hostile, n_accepted);
	return 0;
}
