// tests/fuzz_ragged.cpp -- the host side of `minicom -p -V` as a stand-alone program, built with AddressSanitizer
// and UBSan by `make -C minicom_amd/host fuzz_ragged` (CPU only; tests/test_ragged.py builds and runs it).  fuzz_ragged DIR, where DIR/arch
// is a ragged archive folder that decodes to DIR/in.fastq (the test makes both):
//   1. mcomh_fastq_emit_ragged over small tables in buffers of exactly the room needed, as made and with hostile slots, lengths and name
//      offsets: refused or laid out, never outside a buffer;
//   2. mcomh_decompress_fastq and mcomh_decompress_order over the folder with len.bin, odd.seq and odd.qual dropped, cut short, grown and
//      with seeded byte changes: every folder is refused (and leaves no output file) or decodes;
//   3. the host split (mcomh_fastq_lengths_file, mcomh_fastq_ragged_files, mcomh_fastq_quality_member_ragged, device -1) over seeded
//      mutations of the FASTQ text: a text the lengths pass takes is taken by the other two, one it refuses leaves no length file.
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
static const uint64_t ODD = (uint64_t)1 << 63;

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

// ---- 1. the emit twin -----------------------------------------------------------------------------------------------------------------------
static int emit_fuzz(size_t &n_ok, size_t &n_refused)
{
	for (int round = 0; round < 400; ++round) {
		const uint32_t L = 1 + (uint32_t)(rnd() % 40);
		const uint64_t n = rnd() % 24;
		Bytes len(n), reads, quals, odd_seq, odd_qual, names;
		std::vector<uint64_t> slot(n), off(1, 0);
		uint64_t n_even = 0;
		for (uint64_t i = 0; i < n; ++i) {
			const uint32_t l = rnd() % 3 ? L : 1 + (uint32_t)(rnd() % 60);
			len[i] = (uint8_t)(l - 1);
			if (l == L) { slot[i] = n_even++; for (uint32_t j = 0; j < L; ++j) { reads.push_back("ACGTN"[rnd() % 5]); quals.push_back((uint8_t)(33 + rnd() % 94)); } }
			else { slot[i] = ODD | odd_seq.size(); for (uint32_t j = 0; j < l; ++j) { odd_seq.push_back("ACGTN"[rnd() % 5]); odd_qual.push_back((uint8_t)(33 + rnd() % 94)); } }
			for (int k = 0; k < 2; ++k) { for (uint64_t j = rnd() % 9; j > 0; --j) names.push_back((uint8_t)('a' + rnd() % 26)); names.push_back('\n'); }
			off.push_back(names.size());
		}
		const int mode = round % 3;                                            // 0 reads only, 1 numbered records, 2 named records
		const int hostile = round % 2 ? 1 + (int)(rnd() % 5) : 0;
		if (hostile && n) {
			const uint64_t k = rnd() % n;
			if (hostile == 1) slot[k] = rnd() % 2 ? rnd() : (ODD | rnd());
			if (hostile == 2) len[k] = (uint8_t)rnd();
			if (hostile == 3) off[rnd() % (n + 1)] = rnd() % 2 ? rnd() : rnd() % (names.size() + 3);
			if (hostile == 4) slot[k] ^= ODD;
			if (hostile == 5 && !names.empty()) names[rnd() % names.size()] = (uint8_t)(rnd() % 2 ? '\n' : 'x');
		}
		mcomh_ragged_src S;
		memset(&S, 0, sizeof S);
		S.reads = reads.data(); S.read_pitch = L; S.n_even = n_even; S.L = L; S.odd_seq = odd_seq.data(); S.odd_bytes = odd_seq.size();
		S.slot = slot.data(); S.len = len.data(); S.n = n;
		if (mode) { S.quals = quals.empty() ? (const uint8_t*)"" : quals.data(); S.qual_pitch = L; S.odd_qual = odd_qual.data(); }
		if (mode == 2) { S.names = names.empty() ? (const uint8_t*)"" : names.data(); S.names_bytes = names.size(); S.rec_off = off.data(); }
		uint64_t bytes = 0, again = 0;
		const int rc = mcomh_fastq_emit_ragged(&S, 0, n, nullptr, 0, &bytes);
		if (rc) { if (!hostile) { fprintf(stderr, "emit refused tables as made (round %d)\n", round); return 1; } ++n_refused; continue; }
		Bytes out(bytes);                                                      // exactly the room: ASan guards its end
		if (mcomh_fastq_emit_ragged(&S, 0, n, out.data(), bytes, &again) || again != bytes) { fprintf(stderr, "emit: the second call disagrees with the first (round %d)\n", round); return 1; }
		uint64_t lines = 0;
		for (uint8_t b : out) lines += b == '\n';
		if (!hostile && lines != (mode ? 4 : 1) * n) { fprintf(stderr, "emit: %llu lines for %llu records (round %d)\n", (unsigned long long)lines, (unsigned long long)n, round); return 1; }
		if (bytes && n && mcomh_fastq_emit_ragged(&S, 0, n, out.data(), bytes - 1, &again) != -2) { fprintf(stderr, "emit wrote into too small a buffer\n"); return 1; }
		++n_ok;
	}
	return 0;
}

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: fuzz_ragged DIR (DIR/arch: a ragged archive folder, DIR/in.fastq: what it decodes to)\n"); return 2; }
	size_t n_ok = 0, n_refused = 0, n_folders = 0, n_folder_refused = 0, n_texts = 0, n_text_refused = 0;
	if (emit_fuzz(n_ok, n_refused)) return 1;
	const std::string base = argv[1], dir = base + "/arch", out = base + "/fuzz_out.fastq";
	Bytes want;
	if (!slurp(base + "/in.fastq", want)) { fprintf(stderr, "no %s/in.fastq\n", base.c_str()); return 2; }
	// ---- 2. the decoders over damaged side members ----
	auto decode = [&](bool fastq, Bytes *got) {                                // 0 decoded, 1 refused and nothing left, -1 a refusal that left a file
		unlink(out.c_str());
		uint64_t n = 0;
		const int rc = fastq ? mcomh_decompress_fastq(dir.c_str(), out.c_str(), &n) : mcomh_decompress_order(dir.c_str(), out.c_str(), &n);
		if (rc) return exists(out) ? -1 : 1;
		if (!exists(out)) return -1;
		if (got) slurp(out, *got);
		return 0;
	};
	Bytes got;
	if (decode(true, &got) != 0 || got != want) { fprintf(stderr, "the folder as made does not decode to in.fastq\n"); return 1; }
	if (decode(false, &got) != 0) { fprintf(stderr, "the folder as made does not decode to reads\n"); return 1; }
	for (const char *name : {"len.bin", "odd.seq", "odd.qual"}) {
		const std::string path = dir + "/" + name;
		Bytes good;
		if (!slurp(path, good)) { fprintf(stderr, "no %s\n", path.c_str()); return 2; }
		auto attempt = [&](const Bytes *b) {
			if (b) { if (!spill(path, *b)) return 2; } else unlink(path.c_str());
			for (int fastq = 0; fastq < 2; ++fastq) {
				const int r = decode(fastq != 0, nullptr);
				if (r < 0) { fprintf(stderr, "%s: a refusal left an output file, or a success left none\n", name); return 1; }
				++n_folders; n_folder_refused += r;
			}
			return 0;
		};
		if (int r = attempt(nullptr)) return r;
		for (size_t cut = 0; cut < good.size(); cut += 1 + good.size() / 40) { Bytes b(good.begin(), good.begin() + cut); if (int r = attempt(&b)) return r; }
		{ Bytes b = good; b.push_back(good.empty() ? 0 : good.back()); if (int r = attempt(&b)) return r; }
		for (int k = 0; k < 60 && !good.empty(); ++k) {
			Bytes b = good;
			b[rnd() % b.size()] = (uint8_t)(k % 3 ? rnd() : 99);              // (99: the modal length's byte)
			if (int r = attempt(&b)) return r;
		}
		if (!spill(path, good)) return 2;
	}
	if (decode(true, &got) != 0 || got != want) { fprintf(stderr, "the restored folder does not decode to in.fastq\n"); return 1; }
	// ---- 3. the host split over damaged FASTQ texts ----
	const std::string fq = base + "/fuzz_in.fastq", lenf = base + "/fuzz_len.bin", rows = base + "/fuzz_rows.bin", oddf = base + "/fuzz_odd.bin", mcq = base + "/fuzz.mcq";
	size_t whole = 0, lines = 0;                                              // the whole records in the first 60 000 bytes
	for (size_t i = 0; i < want.size() && i < 60000; ++i) if (want[i] == '\n' && (++lines & 3) == 0) whole = i + 1;
	const Bytes text(want.begin(), want.begin() + whole);
	if (text.empty()) { fprintf(stderr, "in.fastq holds no record\n"); return 2; }
	for (int k = 0; k < 160; ++k) {
		Bytes t = text;
		if (k) {
			const size_t at = rnd() % t.size();
			switch (k % 5) {
			case 0: t.resize(at); break;
			case 1: t[at] = (uint8_t)rnd(); break;
			case 2: t[at] = '\n'; break;
			case 3: t.erase(t.begin() + at); break;
			default: t.insert(t.begin() + at, (uint8_t)(rnd() % 2 ? 'A' : '\n')); break;
			}
		}
		if (!spill(fq, t)) return 2;
		unlink(lenf.c_str());
		char err[320] = ""; uint64_t n = 0, n_odd = 0, ne = 0; int L = 0;
		++n_texts;
		if (mcomh_fastq_lengths_file(fq.c_str(), -1, 0, lenf.c_str(), &n, &L, &n_odd, err, sizeof err)) {
			if (exists(lenf) || !err[0]) { fprintf(stderr, "a refused text left a length file, or no message\n"); return 1; }
			if (!k) { fprintf(stderr, "the text as made is refused: %s\n", err); return 1; }
			++n_text_refused; continue;
		}
		for (int which = 1; which <= 3; which += 2)
			if (mcomh_fastq_ragged_files(fq.c_str(), which, L, -1, lenf.c_str(), 0, rows.c_str(), oddf.c_str(), &ne, err, sizeof err) || ne != n - n_odd) {
				fprintf(stderr, "the lengths pass took a text that the split of line %d refuses: %s\n", which, err); return 1;
			}
		if (mcomh_fastq_quality_member_ragged(fq.c_str(), L, -1, lenf.c_str(), mcq.c_str(), oddf.c_str(), &ne, err, sizeof err) || ne != n - n_odd) { fprintf(stderr, "the quality member is refused: %s\n", err); return 1; }
		// ... and with a length file that is not this text's: refused or split, never outside a buffer
		Bytes lb;
		slurp(lenf, lb);
		if (!lb.empty()) { lb[rnd() % lb.size()] = (uint8_t)rnd(); if (k % 2) lb.pop_back(); spill(lenf, lb); }
		(void)mcomh_fastq_ragged_files(fq.c_str(), 1, L, -1, lenf.c_str(), 0, rows.c_str(), oddf.c_str(), &ne, err, sizeof err);
	}
	for (const std::string &p : {out, fq, lenf, rows, oddf, mcq}) unlink(p.c_str());
	printf("fuzz_ragged ok: %zu tables laid out, %zu refused; %zu damaged folders decoded (%zu refused); %zu texts split (%zu refused)\n", n_ok, n_refused, n_folders, n_folder_refused,
	       n_texts, n_text_refused);
	return 0;
}
