// tests/fuzz_digest.cpp -- the host twin of the digest calls and the parser of digest.txt under the sanitizers (CPU only):
//   make -C minicom_amd/host fuzz_digest && minicom_amd/lib/fuzz_digest [TMPDIR]
// Mutated FASTQ texts in heap buffers of their exact size go through mcomh_fastq_record_hashes with hash arrays of their exact size: a
// record that the checks let through must stay inside the text, a flagged one must leave its words alone.  Damaged digest files go
// through mcomh_digest_parse: whatever it accepts must print back to the same bytes.  Mutated files go through mcomh_fastq_digest_files
// and mcomh_digest_check: no output file is left behind by a refusal.  Prints `fuzz_digest ok`.
#include "../include/mcom_host.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include <sys/stat.h>
#include <unistd.h>

static uint64_t rng_state = 0x1234567887654321ull;
static uint64_t rnd()
{
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
	return rng_state;
}
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "fuzz_digest: %s failed at line %d\n", #c, __LINE__); exit(1); } } while (0)

static std::string make_text(int records, bool fastq)
{
	static const char base[] = "ACGTN";
	static const int lens[] = {1, 7, 8, 9, 15, 16, 17, 100, 255, 256};
	std::string t;
	for (int r = 0; r < records; ++r) {
		const int l = lens[below(10)], nl = below(4) == 0 ? (int)below(256) : (int)below(20), pl = below(3) ? 0 : (int)below(256);
		if (fastq) { t += '@'; for (int k = 0; k < nl; ++k) t += (char)(33 + below(94)); t += '\n'; }
		for (int k = 0; k < l; ++k) t += base[below(5)];
		t += '\n';
		if (fastq) {
			t += '+'; for (int k = 0; k < pl; ++k) t += (char)(33 + below(94)); t += '\n';
			for (int k = 0; k < l; ++k) t += (char)(33 + below(94));
			t += '\n';
		}
	}
	return t;
}

static void mutate(std::string &t)
{
	const int edits = 1 + (int)below(4);
	for (int e = 0; e < edits && !t.empty(); ++e) {
		const size_t at = below((uint32_t)t.size());
		switch (below(6)) {
		case 0: t[at] = '\n'; break;
		case 1: t[at] = (char)below(256); break;
		case 2: t.erase(at, 1 + below(300)); break;
		case 3: t.insert(at, 1 + below(300), 'A'); break;
		case 4: t[at] = '@'; break;
		default: t.insert(at, "\n\n"); break;
		}
	}
}

// the text in a buffer of its exact size, its line starts in one of theirs, the hashes in arrays of theirs
static void hash_exact(const std::string &t, int lpr)
{
	std::unique_ptr<uint8_t[]> text(new uint8_t[t.size() ? t.size() : 1]);
	memcpy(text.get(), t.data(), t.size());
	std::vector<uint64_t> st(1, 0);
	for (size_t k = 0; k < t.size(); ++k) if (t[k] == '\n') st.push_back(k + 1);
	std::unique_ptr<uint64_t[]> start(new uint64_t[st.size()]);
	memcpy(start.get(), st.data(), st.size() * 8);
	const uint64_t records = (st.size() - 1) / (uint64_t)lpr, first = below(3);
	const uint64_t n_total = first + records;
	std::unique_ptr<uint64_t[]> hS(new uint64_t[2 * n_total + 1]), hQ(new uint64_t[2 * n_total + 1]), hN(new uint64_t[2 * n_total + 1]);
	const uint64_t mark = 0xA5A5A5A5A5A5A5A5ull;
	for (uint64_t k = 0; k < 2 * n_total; ++k) hS[k] = hQ[k] = hN[k] = mark;
	uint32_t flag[2] = {0, 0xFFFFFFFFu};
	CHECK(mcomh_fastq_record_hashes(text.get(), t.size(), start.get(), first, records, lpr, n_total, hS.get(), below(2) ? hQ.get() : nullptr, below(2) ? hN.get() : nullptr, flag) == 0);
	for (uint64_t k = 0; k < 2 * first; ++k) CHECK(hS[k] == mark && hQ[k] == mark && hN[k] == mark);       // the rows in front are not this call's
	if (flag[0]) { CHECK(flag[1] >= first && flag[1] < n_total); CHECK(hS[2 * flag[1]] == mark && hS[2 * flag[1] + 1] == mark); }
	else CHECK(flag[1] == 0xFFFFFFFFu);
	// the reduction over what is there
	uint64_t sums[16];
	CHECK(mcomh_digest_reduce(hS.get(), hQ.get(), hN.get(), nullptr, nullptr, nullptr, n_total, sums) == 0);
	CHECK(mcomh_digest_reduce(hS.get(), hQ.get(), nullptr, hN.get(), hS.get(), nullptr, n_total, sums) == 0);
	CHECK(mcomh_digest_reduce(hS.get(), hQ.get(), nullptr, hN.get(), nullptr, nullptr, n_total, sums) != 0);       // the second file without the first one's arrays
}

static void parse_exact(const std::string &t, bool must_parse)
{
	std::unique_ptr<char[]> buf(new char[t.size() ? t.size() : 1]);
	memcpy(buf.get(), t.data(), t.size());
	mcomh_digest d;
	char why[8];                                                               // (a small buffer on purpose: the reason is cut, never overrun)
	const int rc = mcomh_digest_parse(buf.get(), t.size(), &d, why, sizeof why);
	if (must_parse) CHECK(rc == 0);
	if (rc) return;
	char out[1024]; size_t len = 0;
	CHECK(mcomh_digest_print(&d, out, sizeof out, &len) == 0);
	CHECK(len == t.size() && !memcmp(out, t.data(), len));                       // accepted: exactly what the printer writes
}

static bool file_exists(const std::string &p) { struct stat sb; return stat(p.c_str(), &sb) == 0; }
static void write_text(const std::string &p, const std::string &t) { FILE *f = fopen(p.c_str(), "wb"); CHECK(f); CHECK(fwrite(t.data(), 1, t.size(), f) == t.size()); fclose(f); }

int main(int argc, char **argv)
{
	// 1. the record hashes over mutated texts
	for (int it = 0; it < 3000; ++it) {
		const bool fastq = it % 3 != 0;
		std::string t = make_text(1 + (int)below(6), fastq);
		if (it % 5) mutate(t);
		if (it % 7 == 0 && !t.empty()) t.resize(below((uint32_t)t.size()));
		hash_exact(t, fastq ? 4 : 1);
		hash_exact(t, fastq ? 1 : 4);
	}
	// 2. the parser over damaged digests
	mcomh_digest d;
	memset(&d, 0, sizeof d);
	char text[1024]; size_t len = 0;
	int good = 0;
	for (uint32_t files = 1; files <= 2; ++files)
		for (int qual = 0; qual < 2; ++qual)
			for (int names = 0; names < 2; ++names) {
				d.files = files; d.n = rnd() >> 33; d.present = 1u << 0 | 1u << 6;
				if (files == 2) d.present |= 1u << 3;
				if (qual) d.present |= files == 2 ? (1u << 1 | 1u << 4 | 1u << 7) : (1u << 1 | 1u << 7);
				if (names) d.present |= files == 2 ? (1u << 2 | 1u << 5) : 1u << 2;
				for (int k = 0; k < 16; ++k) d.sums[k] = rnd();
				CHECK(mcomh_digest_print(&d, text, sizeof text, &len) == 0);
				const std::string t(text, len);
				parse_exact(t, true); ++good;
				parse_exact(t.substr(0, t.size() - 1), false);
				for (int it = 0; it < 1500; ++it) { std::string m = t; mutate(m); if (m != t) parse_exact(m, false); }
				// a key given twice, an unknown key, a digit too few, upper case, the last newline gone, leading zeros
				const size_t last = t.rfind('\n', t.size() - 2) + 1;
				mcomh_digest o; char why[96];
				CHECK(mcomh_digest_parse((t + t.substr(last)).data(), t.size() + t.size() - last, &o, why, sizeof why) != 0);
				CHECK(mcomh_digest_parse((t + "seq.sorted 0000000000000000 0000000000000000\n").data(), t.size() + 45, &o, why, sizeof why) != 0);
				std::string m = t; m.erase(m.size() - 2, 1);
				CHECK(mcomh_digest_parse(m.data(), m.size(), &o, why, sizeof why) != 0);
				m = t; m[m.size() - 2] = 'A';
				CHECK(mcomh_digest_parse(m.data(), m.size(), &o, why, sizeof why) != 0);
				m = t; m.insert(m.find("\nn ") + 3, "0");
				CHECK(mcomh_digest_parse(m.data(), m.size(), &o, why, sizeof why) != 0);
				d.present ^= 1u << 6;
				CHECK(mcomh_digest_print(&d, text, sizeof text, &len) != 0);           // not a set of keys the printer writes
			}
	CHECK(good == 8);
	// 3. the file calls: a refusal leaves no file
	const std::string dir = std::string(argc > 1 ? argv[1] : "/tmp") + "/fuzz_digest." + std::to_string((long)getpid());
	CHECK(mkdir(dir.c_str(), 0700) == 0);
	const std::string in = dir + "/in.fastq", in2 = dir + "/in2.fastq", out = dir + "/digest.txt", reads = dir + "/out_dec.reads";
	int taken = 0, refused = 0;
	for (int it = 0; it < 300; ++it) {
		std::string t = make_text(1 + (int)below(5), true);
		if (it % 4) mutate(t);
		write_text(in, t);
		char err[64]; uint64_t n = 0;
		remove(out.c_str());
		const int rc = mcomh_fastq_digest_files(in.c_str(), nullptr, 4, it & 1, -1, 0, out.c_str(), &n, err, sizeof err);
		if (rc) { ++refused; CHECK(!file_exists(out)); continue; }
		++taken;
		CHECK(file_exists(out) && n > 0);
		// the check of a folder that holds this digest: against the file itself (a folder without quality or name members reads one read per line, so refused or different, never a crash)
		mcomh_digest_report rep;
		(void)mcomh_digest_check(dir.c_str(), in.c_str(), nullptr, -1, &rep);
		write_text(in2, t + make_text(1, true));
		remove(out.c_str());
		CHECK(mcomh_fastq_digest_files(in.c_str(), in2.c_str(), 4, 1, -1, 0, out.c_str(), &n, err, sizeof err) != 0 && !file_exists(out));   // another record count
	}
	CHECK(taken > 50 && refused > 50);
	// a reads file against the digest of its FASTQ: identical by seq.multiset; one base changed: different
	{
		const std::string t = make_text(40, true);
		std::string r;
		size_t at = 0;
		for (int line = 0; at < t.size(); ++line) { const size_t e = t.find('\n', at); if (line % 4 == 1) r += t.substr(at, e + 1 - at); at = e + 1; }
		write_text(in, t); write_text(reads, r);
		char err[64]; uint64_t n = 0;
		CHECK(mcomh_fastq_digest_files(in.c_str(), nullptr, 4, 1, -1, 0, out.c_str(), &n, err, sizeof err) == 0 && n == 40);
		mcomh_digest_report rep;
		CHECK(mcomh_digest_check(dir.c_str(), reads.c_str(), nullptr, -1, &rep) == 0 && rep.identical && rep.compared == 1u << 6);
		r[0] = r[0] == 'A' ? 'C' : 'A';
		write_text(reads, r);
		CHECK(mcomh_digest_check(dir.c_str(), reads.c_str(), nullptr, -1, &rep) == 0 && !rep.identical && rep.first_diff == 6);
		write_text(out, "minicom-digest 1\nfiles 1\nn 40\n");
		CHECK(mcomh_digest_check(dir.c_str(), reads.c_str(), nullptr, -1, &rep) != 0 && rep.message[0]);
	}
	for (const std::string &p : {in, in2, out, reads}) remove(p.c_str());
	rmdir(dir.c_str());
	printf("fuzz_digest ok\n");
	return 0;
}
