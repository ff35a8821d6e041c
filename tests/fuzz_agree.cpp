// tests/fuzz_agree.cpp -- the host side of `minicom -a Q[:C]` as a stand-alone program, built with AddressSanitizer
// and UBSan by `make -C minicom_amd/host fuzz_agree` (CPU only; tests/test_agree.py builds and runs it).  fuzz_agree DIR, where DIR/arch0,
// DIR/arch1, ... are folders of stream files the mask twin takes (the test makes them, default mode and -p):
//   1. mcomh_qual_agree over hostile pitches, mask pitches, first rows and row counts, the rows and the mask in buffers of exactly the
//      room needed: refused with nothing touched, or exactly the bytes of a loop written here, the bytes between two rows untouched;
//   2. mcomh_agree_mask (device -1) over the folders with every stream file cut short, grown and with seeded byte changes: every folder
//      is refused and leaves no mask file, or gives a file of n rows of (L + 7) / 8 bytes whose bit count is the one returned;
//   3. mcomh_qual_agree_marker over hostile marker files.
#include "../include/mcom_host.h"
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

// ---- 1. the transform twin ------------------------------------------------------------------------------------------------------------------
static int transform_fuzz(size_t &n_ok, size_t &n_refused)
{
	for (int round = 0; round < 600; ++round) {
		uint32_t L = 1 + (uint32_t)(rnd() % 256), Q = (uint32_t)(rnd() % 94);
		uint64_t n = round % 7 == 0 ? 0 : rnd() % 19, first = rnd() % 5;
		const uint64_t mb = (L + 7) / 8;
		uint64_t pitch = L + (rnd() % 3 ? 0 : rnd() % 9), mask_pitch = mb + (rnd() % 3 ? 0 : rnd() % 4);
		const int hostile = round % 3 == 0 ? 1 + (int)(rnd() % 4) : 0;
		if (hostile == 1) Q = 94 + (uint32_t)(rnd() % 1000);
		if (hostile == 2) L = rnd() % 2 ? 0 : 257 + (uint32_t)(rnd() % 100);
		if (hostile == 3) pitch = L ? rnd() % L : 0;
		if (hostile == 4) mask_pitch = mb ? rnd() % mb : 0;
		// exactly the room: the last row has no slack behind its L bytes, the mask none behind its last row's (L + 7) / 8 bytes
		const bool sane = L >= 1 && L <= 256;
		Bytes rows(n && sane ? (size_t)((n - 1) * (hostile == 3 ? L : pitch) + L) : 0), mask(sane ? (size_t)((first + n ? first + n - 1 : 0) * (hostile == 4 ? mb : mask_pitch) + (first + n ? mb : 0)) : 0);
		for (uint8_t &b : rows) b = (uint8_t)(33 + rnd() % 94);
		for (uint8_t &b : mask) b = (uint8_t)rnd();
		const Bytes before = rows;
		mcomh_qual_agree_report r;
		memset(&r, 0xEE, sizeof r);
		const int rc = mcomh_qual_agree(rows.empty() ? nullptr : rows.data(), n, L, pitch, mask.empty() ? nullptr : mask.data(), mask_pitch, first, Q, &r);
		if (hostile) {
			if (rc == 0) { fprintf(stderr, "transform took hostile arguments (round %d, kind %d)\n", round, hostile); return 1; }
			if (rows != before) { fprintf(stderr, "a refused transform touched the rows (round %d)\n", round); return 1; }
			++n_refused; continue;
		}
		if (rc) { fprintf(stderr, "transform refused sane arguments (round %d: n %llu L %u pitch %llu mask pitch %llu)\n", round, (unsigned long long)n, L, (unsigned long long)pitch, (unsigned long long)mask_pitch); return 1; }
		Bytes want = before;
		uint64_t bits = 0, changed = 0;
		for (uint64_t j = 0; j < n; ++j) for (uint32_t i = 0; i < L; ++i)
			if ((mask[(size_t)((first + j) * mask_pitch + (i >> 3))] >> (i & 7)) & 1) { ++bits; changed += want[(size_t)(j * pitch + i)] != 33 + Q; want[(size_t)(j * pitch + i)] = (uint8_t)(33 + Q); }
		if (rows != want || r.mask_bits != bits || r.changed != changed) { fprintf(stderr, "transform: other bytes or another report than the loop (round %d)\n", round); return 1; }
		++n_ok;
	}
	return 0;
}

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: fuzz_agree DIR (DIR/arch0, DIR/arch1, ...: folders of stream files)\n"); return 2; }
	size_t n_ok = 0, n_refused = 0, n_folders = 0, n_folder_refused = 0, n_markers = 0;
	if (transform_fuzz(n_ok, n_refused)) return 1;
	const std::string base = argv[1], out = base + "/fuzz.mask";
	// ---- 2. the mask twin over damaged stream files ----
	for (int a = 0; ; ++a) {
		const std::string dir = base + "/arch" + std::to_string(a);
		if (!exists(dir + "/info.txt")) { if (!a) { fprintf(stderr, "no %s\n", dir.c_str()); return 2; } break; }
		auto mask_of = [&](int C) {                                             // 0 made, 1 refused and nothing left, -1 an inconsistent answer
			unlink(out.c_str());
			uint64_t n = 0, bits = 0; int L = 0;
			if (mcomh_agree_mask(dir.c_str(), C, out.c_str(), -1, &n, &L, &bits)) return exists(out) ? -1 : 1;
			Bytes m;
			if (!slurp(out, m) || L < 1 || L > 256 || m.size() != n * (uint64_t)((L + 7) / 8)) return -1;
			uint64_t got = 0;
			for (uint8_t b : m) got += (uint64_t)__builtin_popcount(b);
			return got == bits ? 0 : -1;
		};
		if (mask_of(2) != 0) { fprintf(stderr, "%s as made has no mask\n", dir.c_str()); return 1; }
		if (mask_of(0) != 1 || mask_of(256) != 1) { fprintf(stderr, "a coverage outside 1 .. 255 was taken\n"); return 1; }
		std::vector<std::string> names = {"info.txt", "beg_pos.bin.0", "ref.bin.0", "dir.bin.0", "dif_char.txt.0", "single.seq", "single_N.seq", "AA.txt", "TT.txt"};
		for (const char *nm : {"ids.bin.0", "singleFile.ids.bin", "Nfile.ids.bin", "AA.ids.bin", "allA.ids.bin"}) if (exists(dir + "/" + nm)) names.push_back(nm);
		for (const std::string &name : names) {
			const std::string path = dir + "/" + name;
			Bytes good;
			if (!slurp(path, good)) { fprintf(stderr, "no %s\n", path.c_str()); return 2; }
			auto attempt = [&](const Bytes &b) {
				if (!spill(path, b)) return 2;
				const int r = mask_of(1 + (int)(rnd() % 4));
				if (r < 0) { fprintf(stderr, "%s damaged: a refusal left a mask file, or a mask of another size or bit count than stated\n", name.c_str()); return 1; }
				++n_folders; n_folder_refused += (size_t)r;
				return 0;
			};
			for (size_t cut = 0; cut < good.size(); cut += 1 + good.size() / 24) { Bytes b(good.begin(), good.begin() + cut); if (int r = attempt(b)) return r; }
			{ Bytes b = good; b.push_back(good.empty() ? 0 : good.back()); if (int r = attempt(b)) return r; }
			for (int k = 0; k < 48 && !good.empty(); ++k) {
				Bytes b = good;
				const size_t at = rnd() % b.size();
				b[at] = (uint8_t)(k % 4 == 0 ? 0xFF : k % 4 == 1 ? '9' : k % 4 == 2 ? b[at] ^ (1u << (rnd() % 8)) : rnd());
				if (int r = attempt(b)) return r;
			}
			if (!spill(path, good)) return 2;
		}
		if (mask_of(2) != 0) { fprintf(stderr, "%s restored has no mask\n", dir.c_str()); return 1; }
		// ---- 3. the marker ----
		const std::string marker = dir + "/qual_agree.txt";
		const char *good_markers[] = {"0 1\n", "40 3\n", "93 255\n"}, *bad_markers[] = {"", "x", "40 3", "40  3\n", "040 3\n", "40 03\n", "94 3\n", "40 0\n", "40 256\n", "40 3\n\n", " 40 3\n", "40 3 \n", "-1 3\n", "40:3\n", "4000000000 3\n"};
		for (const char *t : good_markers) { uint32_t Q = 999, C = 999; spill(marker, Bytes(t, t + strlen(t))); if (mcomh_qual_agree_marker(dir.c_str(), &Q, &C) != 1 || Q > 93 || C < 1 || C > 255) { fprintf(stderr, "the marker %s is not read\n", t); return 1; } ++n_markers; }
		for (const char *t : bad_markers) { uint32_t Q = 0, C = 0; spill(marker, Bytes(t, t + strlen(t))); if (mcomh_qual_agree_marker(dir.c_str(), &Q, &C) != -1) { fprintf(stderr, "the marker `%s` is taken\n", t); return 1; } ++n_markers; }
		for (int k = 0; k < 200; ++k) { Bytes b(rnd() % 12); for (uint8_t &c : b) c = (uint8_t)(rnd() % 3 ? "0123456789 \n"[rnd() % 12] : rnd()); spill(marker, b); uint32_t Q = 0, C = 0; const int rc = mcomh_qual_agree_marker(dir.c_str(), &Q, &C); if (rc == 1 && (Q > 93 || C < 1 || C > 255)) { fprintf(stderr, "a marker out of range is taken\n"); return 1; } ++n_markers; }
		unlink(marker.c_str());
		if (mcomh_qual_agree_marker(dir.c_str(), nullptr, nullptr) != 0) { fprintf(stderr, "a marker where there is none\n"); return 1; }
	}
	unlink(out.c_str());
	printf("fuzz_agree ok: %zu matrices transformed, %zu refused; %zu damaged folders masked (%zu refused); %zu markers\n", n_ok, n_refused, n_folders, n_folder_refused, n_markers);
	return 0;
}
