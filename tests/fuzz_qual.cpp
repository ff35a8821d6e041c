// tests/fuzz_qual.cpp -- the host twin of the quality-value coder (host/mcom_qual.cpp) as a stand-alone program, built with
// AddressSanitizer and UBSan by `make -C minicom_amd/host fuzz_qual` (CPU only).  fuzz_qual DIR: generated matrices of many shapes
// are coded under every hint, at two pitches, and decoded back into tables of exactly the room asked for; every file DIR/*.mcq must
// be refused; then every truncation and 4000 seeded bit flips of two small members (a coded one and one with an embedded `.rans`
// member) are decoded -- whatever the verdict, no read or write may leave a buffer, and what is accepted must be the original.
#include "../include/mcom_host.h"
#include <dirent.h>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static uint64_t g_x = 88172645463325252ull;
static uint64_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return g_x; }

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

// rows that drift like quality strings over `alphabet` values from 33 upwards
static std::vector<uint8_t> matrix(uint64_t n, uint32_t L, uint32_t alphabet, uint64_t pitch)
{
	std::vector<uint8_t> m(n * pitch, 0xEE);
	for (uint64_t r = 0; r < n; ++r) {
		uint32_t cur = (uint32_t)(rnd() % alphabet);
		for (uint32_t j = 0; j < L; ++j) {
			const uint64_t t = rnd() % 16;
			if (t == 0) cur = (uint32_t)(rnd() % alphabet); else if (t < 4 && cur) --cur; else if (t < 6 && cur + 1 < alphabet) ++cur;
			m[r * pitch + j] = (uint8_t)(33 + cur);
		}
	}
	return m;
}

// 0 and the rows back to back, or -1
static int decode(const std::vector<uint8_t> &m, std::vector<uint8_t> &out, uint64_t &n, uint32_t &L)
{
	n = 0; L = 0;
	if (mcomh_qual_info(m.data(), m.size(), &n, &L) || n * L > ((uint64_t)1 << 28)) return -1;
	out.assign(n * L, 0);                                                        // exactly the room asked for: ASan guards its ends
	uint64_t gn = 0; uint32_t gL = 0;
	if (mcomh_qual_decode(m.data(), m.size(), out.data(), L, n, &gn, &gL) || gn != n || gL != L) return -1;
	return 0;
}

static int hostile(const std::vector<uint8_t> &good, const std::vector<uint8_t> &raw, uint64_t n0, uint32_t L0, size_t &n_hostile, size_t &n_accepted)
{
	std::vector<uint8_t> out; uint64_t n; uint32_t L;
	for (size_t cut = 0; cut < good.size(); ++cut, ++n_hostile) {
		std::vector<uint8_t> m(good.begin(), good.begin() + cut);
		if (!decode(m, out, n, L)) { fprintf(stderr, "cut@%zu accepted\n", cut); return 1; }
	}
	for (int k = 0; k < 4000; ++k, ++n_hostile) {
		std::vector<uint8_t> m = good;
		const uint64_t bit = rnd() % (8 * m.size());
		m[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
		if (!decode(m, out, n, L)) { ++n_accepted; if (n != n0 || L != L0 || out != raw) { fprintf(stderr, "flip@%llu accepted with other bytes\n", (unsigned long long)bit); return 1; } }
	}
	return 0;
}

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: fuzz_qual DIR\n"); return 2; }
	size_t n_trips = 0, n_bad = 0, n_hostile = 0, n_accepted = 0;
	const int hints[7] = {0, 0x100, 0x101, 0x102, 0x103, 0x104, 0x180};
	const uint32_t Ls[7] = {1, 2, 3, 37, 100, 150, 256}, alphabets[5] = {1, 2, 4, 41, 94};
	std::vector<uint8_t> out;
	for (uint32_t L : Ls) for (uint32_t a : alphabets) for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)(2048 / L ? 2048 / L : 1), (uint64_t)(3 * (2048 / L ? 2048 / L : 1) + 1)}) {
		for (uint64_t pitch : {(uint64_t)L, (uint64_t)L + 3}) {
			const std::vector<uint8_t> rows = matrix(n, L, a, pitch);
			std::vector<uint8_t> flat(n * L);
			for (uint64_t r = 0; r < n; ++r) memcpy(flat.data() + r * L, rows.data() + r * pitch, L);
			for (int hint : hints) {
				std::vector<uint8_t> m(mcomh_qual_bound(n, L));
				uint64_t len = 0, gn; uint32_t gL;
				if (mcomh_qual_encode(rows.data(), n, L, pitch, m.data(), m.size(), &len, hint)) { fprintf(stderr, "encode failed: n %llu L %u A %u hint %x\n", (unsigned long long)n, L, a, hint); return 1; }
				m.resize(len);
				if (decode(m, out, gn, gL) || gn != n || gL != L || out != flat) { fprintf(stderr, "round trip failed: n %llu L %u A %u hint %x\n", (unsigned long long)n, L, a, hint); return 1; }
				std::vector<uint8_t> tight(len > 0 ? len - 1 : 0);                   // one byte too little room: refused, nothing written beyond it
				uint64_t l2 = 0;
				if (len && mcomh_qual_encode(rows.data(), n, L, pitch, tight.data(), tight.size(), &l2, hint) == 0) { fprintf(stderr, "encode into too little room succeeded\n"); return 1; }
				++n_trips;
			}
		}
	}
	const std::string dir = argv[1];
	if (DIR *d = opendir(dir.c_str())) {
		while (dirent *e = readdir(d)) {
			const std::string nm = e->d_name;
			if (nm.size() < 4 || nm.compare(nm.size() - 4, 4, ".mcq")) continue;
			uint64_t n; uint32_t L;
			if (!decode(slurp(dir + "/" + nm), out, n, L)) { fprintf(stderr, "%s: accepted\n", nm.c_str()); return 1; }
			++n_bad;
		}
		closedir(d);
	} else return 2;
	for (int hint : {0x102, 0x104, 0x180}) {
		const uint64_t n = 9; const uint32_t L = 37;
		const std::vector<uint8_t> rows = matrix(n, L, 4, L);
		std::vector<uint8_t> m(mcomh_qual_bound(n, L));
		uint64_t len = 0;
		if (mcomh_qual_encode(rows.data(), n, L, L, m.data(), m.size(), &len, hint)) return 1;
		m.resize(len);
		if (hostile(m, rows, n, L, n_hostile, n_accepted)) return 1;
	}
	printf("fuzz_qual ok: %zu round trips, %zu refused, %zu hostile (%zu harmless)\n", n_trips, n_bad, n_hostile, n_accepted);
	return 0;
}
