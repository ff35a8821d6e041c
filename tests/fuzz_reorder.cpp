// tests/fuzz_reorder.cpp -- the host side of `minicom -q` as a stand-alone program, built with AddressSanitizer
// and UBSan by `make -C minicom_amd/host fuzz_reorder` (CPU only) and run by hand.  fuzz_reorder [TMPDIR]:
//   1. mcomh_qual_gather_rows over tables of many shapes and pitches, in buffers of exactly the room needed, with orders that are
//      permutations (the result is checked) and with hostile ones (entries beyond the table, rows named twice: the flags must say so, the
//      rows of good entries must still be right, nothing may be touched beside them);
//   2. mcomh_decompress_fastq_reordered and mcomh_decompress_fastq_pe over a small hand-made default and paired-end folder: every
//      truncation and seeded bit flips of every file in it.  Whatever the verdict, no read or write may leave a buffer, and a refused
//      folder leaves no output file.
#include "../include/mcom_host.h"
#include <dirent.h>
#include <sys/stat.h>
#include <unistd.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

static uint64_t g_x = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return g_x; }
typedef std::vector<uint8_t> Bytes;
typedef std::map<std::string, Bytes> Folder;

static Bytes str(const char *s) { return Bytes(s, s + strlen(s)); }
static Bytes u32s(std::initializer_list<uint32_t> v) { Bytes b; for (uint32_t x : v) for (int k = 0; k < 4; ++k) b.push_back((uint8_t)(x >> (8 * k))); return b; }
static bool exists(const std::string &p) { struct stat st; return stat(p.c_str(), &st) == 0; }

static bool write_folder(const std::string &dir, const Folder &f)
{
	mkdir(dir.c_str(), 0700);
	if (DIR *d = opendir(dir.c_str())) { while (dirent *e = readdir(d)) if (e->d_name[0] != '.') unlink((dir + "/" + e->d_name).c_str()); closedir(d); } else return false;
	for (const auto &kv : f) {
		FILE *o = fopen((dir + "/" + kv.first).c_str(), "wb");
		if (!o) return false;
		if (!kv.second.empty() && fwrite(kv.second.data(), 1, kv.second.size(), o) != kv.second.size()) { fclose(o); return false; }
		fclose(o);
	}
	return true;
}

static Bytes member(uint64_t n, uint32_t L)
{
	Bytes rows(n * L);
	for (uint8_t &b : rows) b = (uint8_t)(33 + rnd() % 41);
	Bytes m(mcomh_qual_bound(n, L));
	uint64_t len = 0;
	if (mcomh_qual_encode(rows.data(), n, L, L, m.data(), m.size(), &len, 0)) { fprintf(stderr, "encode failed\n"); exit(1); }
	m.resize(len);
	return m;
}

// twelve reads of eight bases: 2 all-A, 1 all-T, 1 all-N, one near-A, one near-T, one with N, two packed singles, one contig of three members
static Folder streams(bool paired)
{
	Folder f;
	f["info.txt"] = str(paired ? "8 1\n6\n2 1 1\n" : "8 1\n2 1 1\n");
	f["AA.txt"] = str("3C\n"); f["TT.txt"] = str("0\n"); f["NN.txt"] = Bytes();
	f["single_N.seq"] = str("ACGTNACG\n");
	f["single.seq"] = Bytes{0x1B, 0xE4, 0x27, 0x8D};
	f["ref.bin.0"] = Bytes{0x1B, 0xB1, 0x4E};
	Bytes pos = u32s({3});
	for (uint16_t d : {0, 2, 2}) { pos.push_back((uint8_t)d); pos.push_back((uint8_t)(d >> 8)); }
	f["beg_pos.bin.0"] = pos;
	f["dir.bin.0"] = Bytes{0x02};
	f["dif_char.txt.0"] = str("0\n2G\n0\n");
	if (paired) {
		f["file.bin.sp"] = Bytes{0xAA, 0x00}; f["peids.bin.sp"] = u32s({3, 0, 5, 1});
		f["file.bin.0"] = Bytes{0x06}; f["peids.bin.0"] = u32s({4, 2});
		f["rqual_1.mcq"] = member(6, 8); f["rqual_2.mcq"] = member(6, 8);
	} else f["rqual.mcq"] = member(12, 8);
	return f;
}

// 0 decoded, 1 refused (and no output file left), -1 a refusal that left a file behind, -2 decoded but not `want` four-line records
static int decode(const std::string &dir, bool paired, const std::string &o1, const std::string &o2, uint64_t want)
{
	unlink(o1.c_str()); unlink(o2.c_str());
	uint64_t n = 0;
	const int rc = paired ? mcomh_decompress_fastq_pe(dir.c_str(), o1.c_str(), o2.c_str(), &n) : mcomh_decompress_fastq_reordered(dir.c_str(), o1.c_str(), &n);
	if (rc) return exists(o1) || exists(o2) ? -1 : 1;
	if (!exists(o1) || (paired && !exists(o2))) return -1;
	if (n != want) return -2;                                                // what decodes holds the records the folder was made of: the member states their number
	for (const std::string *o : {&o1, &o2}) {
		if (o == &o2 && !paired) break;
		FILE *f = fopen(o->c_str(), "rb");
		if (!f) return -2;
		uint64_t lines = 0; int c;
		while ((c = fgetc(f)) != EOF) if (c == '\n') ++lines;
		fclose(f);
		if (lines != 4 * want) return -2;
	}
	return 0;
}

static int gather_fuzz(size_t &n_good, size_t &n_hostile)
{
	const uint32_t Ls[7] = {1, 2, 15, 16, 17, 100, 256};
	for (uint32_t L : Ls) for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)17, (uint64_t)300}) for (uint64_t pi : {(uint64_t)L, (uint64_t)L + 1, (uint64_t)L + 13}) for (uint64_t po : {(uint64_t)L, (uint64_t)L + 5}) {
		Bytes src(n ? (n - 1) * pi + L : 0);                                 // exactly the bytes of the table: ASan guards its ends
		for (uint8_t &b : src) b = (uint8_t)rnd();
		std::vector<uint32_t> order(n);
		for (uint64_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
		for (uint64_t i = n; i > 1; --i) std::swap(order[i - 1], order[rnd() % i]);
		Bytes out(n ? (n - 1) * po + L : 0, 0xA5);
		uint32_t flag = 0;
		if (mcomh_qual_gather_rows(src.data(), n, L, pi, order.data(), n, out.data(), po, &flag) || flag) { fprintf(stderr, "gather refused a permutation (n %llu L %u)\n", (unsigned long long)n, L); return 1; }
		for (uint64_t j = 0; j < n; ++j) {
			if (memcmp(out.data() + j * po, src.data() + order[j] * pi, L)) { fprintf(stderr, "gather: row %llu wrong\n", (unsigned long long)j); return 1; }
			for (uint64_t k = L; k < po && j + 1 < n; ++k) if (out[j * po + k] != 0xA5) { fprintf(stderr, "gather wrote between rows\n"); return 1; }
		}
		++n_good;
		if (!n) continue;
		for (int round = 0; round < 8; ++round, ++n_hostile) {
			std::vector<uint32_t> bad = order;
			uint32_t want = 0;
			std::vector<uint8_t> skipped(n, 0);
			const int kinds = 1 + (int)(rnd() % 3);
			if (kinds & 1) { const uint64_t j = rnd() % n; bad[j] = (uint32_t)(n + rnd() % 3 + (rnd() % 2 ? 0xFFFF0000u : 0u)); skipped[j] = 1; want |= MCOMH_GATHER_F_BOUNDS; }
			if ((kinds & 2) && n > 1) {
				uint64_t a = rnd() % n, b = rnd() % n;
				if (a == b) b = (a + 1) % n;
				if (!skipped[a] && !skipped[b]) { bad[a] = bad[b]; want |= MCOMH_GATHER_F_DUP; }
			}
			std::fill(out.begin(), out.end(), 0xA5);
			flag = 0;
			if (mcomh_qual_gather_rows(src.data(), n, L, pi, bad.data(), n, out.data(), po, &flag) || flag != want) { fprintf(stderr, "gather: flags %u, %u expected\n", flag, want); return 1; }
			for (uint64_t j = 0; j < n; ++j) {
				if (skipped[j]) { for (uint32_t k = 0; k < L; ++k) if (out[j * po + k] != 0xA5) { fprintf(stderr, "gather followed a bad index\n"); return 1; } }
				else if (memcmp(out.data() + j * po, src.data() + bad[j] * pi, L)) { fprintf(stderr, "gather: good row %llu wrong beside a bad one\n", (unsigned long long)j); return 1; }
			}
		}
		// fewer rows out than in, and arguments that must be refused
		if (mcomh_qual_gather_rows(src.data(), n, L, pi, order.data(), n / 2, out.data(), po, &flag)) return 1;
		if (!mcomh_qual_gather_rows(src.data(), n, L, L - 1, order.data(), n, out.data(), po, &flag) || !mcomh_qual_gather_rows(src.data(), n, L, pi, order.data(), n, out.data(), L - 1, &flag) ||
		    !mcomh_qual_gather_rows(src.data(), n, L, pi, order.data(), n, out.data(), po, nullptr) || !mcomh_qual_gather_rows(src.data(), n, 257, 300, order.data(), n, out.data(), 300, &flag)) {
			fprintf(stderr, "gather accepted bad arguments\n"); return 1;
		}
	}
	return 0;
}

int main(int argc, char **argv)
{
	size_t n_good = 0, n_hostile = 0, n_folders = 0, n_refused = 0, n_harmless = 0;
	if (gather_fuzz(n_good, n_hostile)) return 1;
	char tmpl[512];
	snprintf(tmpl, sizeof tmpl, "%s/fuzz_reorder_XXXXXX", argc > 1 ? argv[1] : "/tmp");
	if (!mkdtemp(tmpl)) { fprintf(stderr, "no temporary directory under %s\n", argc > 1 ? argv[1] : "/tmp"); return 2; }
	const std::string base = tmpl, dir = base + "/arch", o1 = base + "/o1.fastq", o2 = base + "/o2.fastq";
	for (int paired = 0; paired < 2; ++paired) {
		const Folder good = streams(paired != 0);
		if (!write_folder(dir, good)) return 2;
		if (decode(dir, paired, o1, o2, paired ? 6 : 12) != 0) { fprintf(stderr, "the %s folder is refused as made\n", paired ? "paired-end" : "default"); return 1; }
		for (const auto &kv : good) {
			auto attempt = [&](const Bytes &b, bool drop) {
				Folder f = good;
				if (drop) f.erase(kv.first); else f[kv.first] = b;
				if (!write_folder(dir, f)) return 2;
				const int r = decode(dir, paired, o1, o2, paired ? 6 : 12);
				if (r < 0) { fprintf(stderr, r == -2 ? "%s: accepted with another number of records\n" : "%s: a refusal left an output file, or a success left none\n", kv.first.c_str()); return 1; }
				++n_folders; if (r) ++n_refused; else ++n_harmless;
				return 0;
			};
			if (int r = attempt(Bytes(), true)) return r;
			for (size_t cut = 0; cut < kv.second.size(); cut += kv.second.size() > 200 ? 7 : 1)
				if (int r = attempt(Bytes(kv.second.begin(), kv.second.begin() + cut), false)) return r;
			for (int k = 0; k < 120 && !kv.second.empty(); ++k) {
				Bytes b = kv.second;
				const uint64_t bit = rnd() % (8 * b.size());
				b[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
				if (int r = attempt(b, false)) return r;
			}
		}
	}
	write_folder(dir, Folder());
	rmdir(dir.c_str()); unlink(o1.c_str()); unlink(o2.c_str()); rmdir(base.c_str());
	printf("fuzz_reorder ok: %zu gathers through permutations, %zu through hostile orders, %zu damaged folders decoded (%zu refused, %zu harmless)\n", n_good, n_hostile, n_folders, n_refused, n_harmless);
	return 0;
}
