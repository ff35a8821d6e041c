// tests/fuzz_range.cpp -- the host side of `minicom -d -R` as a stand-alone program, built with AddressSanitizer
// and UBSan by `make -C minicom_amd/host fuzz_range` (CPU only, run by hand: `../lib/fuzz_range [DIR]`; not part of the suite).
//   1. mcomh_qual_decode_rows over members of every model id and of kind 1, in output buffers of exactly count * L bytes: every range of
//      the member as made equals the slice of the full decode; truncated members are refused; a member with a flipped bit is refused or
//      gives rows -- the full decode's rows whenever the full decoder takes the member too -- and never writes outside the buffer.
//   2. with DIR, a -p archive folder (stream files, and qual.mcq / name.mcn when it keeps them: what `minicom -d` unpacks): the range twins
//      (device -1) over the folder as made -- tilings concatenate to the full decode -- and with every file of it cut short, grown and
//      changed at seeded places: a refused folder leaves no output file, an accepted one leaves one.
#include "../include/mcom_host.h"
#include <dirent.h>
#include <sys/stat.h>
#include <unistd.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static uint64_t g_x = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return g_x; }
typedef std::vector<uint8_t> Bytes;

static bool exists(const std::string &p) { struct stat st; return stat(p.c_str(), &st) == 0; }
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

// ---- 1. quality rows ------------------------------------------------------------------------------------------------------------------------
// rows [first, first + count) into a buffer of exactly the clipped count * L bytes: 0 and the rows, or 1 refused
static int rows_of(const Bytes &m, uint64_t n, uint32_t L, uint64_t first, uint64_t count, Bytes &out)
{
	const uint64_t c = first > n ? 0 : count < n - first ? count : n - first;
	out.assign((size_t)(c * L), 0xEE);
	uint64_t gn = 0; uint32_t gL = 0;
	if (mcomh_qual_decode_rows(m.data(), m.size(), first, count, out.empty() ? nullptr : out.data(), L, &gn, &gL)) return 1;
	return gn == n && gL == L ? 0 : -1;
}

static int qual_fuzz(size_t &n_ranges, size_t &n_hostile, size_t &n_hostile_refused)
{
	const int hints[6] = {0x100, 0x101, 0x102, 0x103, 0x104, 0x180};
	const uint32_t Ls[5] = {1, 7, 100, 150, 256};
	for (uint32_t L : Ls) for (int alpha = 0; alpha < 3; ++alpha) {
		const uint32_t rps = 2048 / L ? 2048 / L : 1, A = alpha == 0 ? 1 : alpha == 1 ? 4 : 94;
		const uint64_t n = 2 * rps + 3;
		Bytes q((size_t)(n * L));
		for (uint8_t &v : q) v = (uint8_t)(33 + (rnd() % 5 ? rnd() % 3 : rnd()) % A);
		for (int hint : hints) {
			Bytes m((size_t)mcomh_qual_bound(n, L));
			uint64_t len = 0;
			if (mcomh_qual_encode(q.data(), n, L, L, m.data(), m.size(), &len, hint)) { fprintf(stderr, "encode failed (L %u, hint %#x)\n", L, hint); return 1; }
			m.resize((size_t)len);
			Bytes out;
			const uint64_t firsts[7] = {0, 1, rps - 1, rps, rps + 1, n - 1, n}, counts[6] = {0, 1, rps, rps + 1, n, n + 5};
			for (uint64_t first : firsts) for (uint64_t count : counts) {
				if (rows_of(m, n, L, first, count, out) != 0 || (!out.empty() && memcmp(out.data(), q.data() + first * L, out.size()))) { fprintf(stderr, "rows %llu + %llu of a member as made differ (L %u, hint %#x)\n", (unsigned long long)first, (unsigned long long)count, L, hint); return 1; }
				++n_ranges;
			}
			if (rows_of(m, n, L, n + 1, 1, out) != 1) { fprintf(stderr, "first > n is taken\n"); return 1; }
			for (size_t cut = 0; cut < m.size(); cut += 1 + m.size() / 23) {
				const Bytes t(m.begin(), m.begin() + cut);
				if (rows_of(t, n, L, rps, 2, out) != 1) { fprintf(stderr, "a truncated member is taken (L %u, hint %#x, %zu bytes)\n", L, hint, cut); return 1; }
			}
			for (int k = 0; k < 40; ++k) {
				Bytes b = m;
				const uint64_t bit = rnd() % (b.size() * 8);
				b[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
				uint64_t hn = 0; uint32_t hL = 0;
				// a header that states other sizes: the buffer follows it, as a caller's does (one that is no header is refused whatever the buffer)
				if (mcomh_qual_info(b.data(), b.size(), &hn, &hL)) { hn = n; hL = L; }
				if (hn > 4 * n) continue;
				const uint64_t first = rnd() % (hn + 1), count = rnd() % (rps + 3);
				const int r = rows_of(b, hn, hL, first, count, out);
				++n_hostile; n_hostile_refused += r == 1;
				if (r) continue;
				Bytes full((size_t)(hn * hL) + 1);
				uint64_t gn = 0; uint32_t gL = 0;
				if (!mcomh_qual_decode(b.data(), b.size(), full.data(), hL, hn, &gn, &gL) && !out.empty() && memcmp(out.data(), full.data() + first * hL, out.size())) { fprintf(stderr, "a member both decoders take gives other rows\n"); return 1; }
			}
		}
	}
	return 0;
}

// ---- 2. the range twins over a folder ---------------------------------------------------------------------------------------------------------
int main(int argc, char **argv)
{
	size_t n_ranges = 0, n_hostile = 0, n_hostile_refused = 0, n_folders = 0, n_folder_refused = 0;
	if (qual_fuzz(n_ranges, n_hostile, n_hostile_refused)) return 1;
	if (argc < 2) { printf("fuzz_range ok: %zu ranges of members as made, %zu hostile members (%zu refused); no folder given\n", n_ranges, n_hostile, n_hostile_refused); return 0; }
	const std::string dir = argv[1], out = dir + "/fuzz_range_out";
	const bool fastq = exists(dir + "/qual.mcq");
	auto decode = [&](uint64_t first, uint64_t count, Bytes *got, uint64_t *n_written) {   // 0 decoded, 1 refused and nothing left, -1 a refusal that left a file
		unlink(out.c_str());
		uint64_t n = 0;
		const int rc = fastq ? mcomh_decompress_fastq_range(dir.c_str(), out.c_str(), first, count, &n, -1) : mcomh_decompress_order_range(dir.c_str(), out.c_str(), first, count, &n, -1);
		if (rc) return exists(out) ? -1 : 1;
		if (!exists(out)) return -1;
		if (got) slurp(out, *got);
		if (n_written) *n_written = n;
		return 0;
	};
	Bytes whole, part, joined;
	uint64_t n = 0, w = 0;
	if (decode(0, ~(uint64_t)0 >> 1, &whole, &n) != 0 || !n) { fprintf(stderr, "%s does not decode as a -p archive\n", dir.c_str()); return 1; }
	for (int round = 0; round < 6; ++round) {
		joined.clear();
		for (uint64_t at = 0; at < n; at += w) {
			const uint64_t count = 1 + rnd() % (n / 3 + 1);
			if (decode(at, count, &part, &w) != 0 || !w) { fprintf(stderr, "range %llu + %llu of the folder as made is refused\n", (unsigned long long)at, (unsigned long long)count); return 1; }
			joined.insert(joined.end(), part.begin(), part.end());
		}
		if (joined != whole) { fprintf(stderr, "a tiling does not concatenate to the full decode\n"); return 1; }
	}
	if (decode(n, 3, &part, &w) != 0 || w || !part.empty() || decode(n + 1, 3, nullptr, nullptr) != 1) { fprintf(stderr, "first == n must give an empty file, first > n a refusal\n"); return 1; }
	std::vector<std::string> files;
	if (DIR *dp = opendir(dir.c_str())) {
		while (dirent *e = readdir(dp)) { const std::string name = e->d_name; if (name != "." && name != ".." && name != "fuzz_range_out") files.push_back(name); }
		closedir(dp);
	}
	for (const std::string &name : files) {
		const std::string path = dir + "/" + name;
		Bytes good;
		if (!slurp(path, good)) continue;
		auto attempt = [&](const Bytes &b) {
			if (!spill(path, b)) return 2;
			const uint64_t first = rnd() % (n + 2), count = rnd() % (n / 2 + 2);
			const int r = decode(first, count, nullptr, nullptr);
			if (r < 0) { fprintf(stderr, "%s: a refusal left an output file, or a success left none\n", name.c_str()); return 1; }
			++n_folders; n_folder_refused += r;
			return 0;
		};
		for (size_t cut = 0; cut < good.size(); cut += 1 + good.size() / 12) { const Bytes b(good.begin(), good.begin() + cut); if (int r = attempt(b)) return r; }
		{ Bytes b = good; b.push_back(good.empty() ? 0 : good.back()); if (int r = attempt(b)) return r; }
		for (int k = 0; k < 24 && !good.empty(); ++k) {
			Bytes b = good;
			b[rnd() % b.size()] = (uint8_t)rnd();
			if (int r = attempt(b)) return r;
		}
		if (!spill(path, good)) return 2;
	}
	if (decode(0, n, &part, nullptr) != 0 || part != whole) { fprintf(stderr, "the restored folder does not decode as before\n"); return 1; }
	unlink(out.c_str());
	printf("fuzz_range ok: %zu ranges of members as made, %zu hostile members (%zu refused); %zu damaged folders decoded (%zu refused)\n", n_ranges, n_hostile, n_hostile_refused,
	       n_folders, n_folder_refused);
	return 0;
}
