// tests/fuzz_inflate_model.cpp -- the inflate model's host twin (host/mcom_gzip_gpu.cpp over csrc/inflate_model.hpp, DESIGN.md section
// 3.15) under ASan / UBSan, against the project's own inflater (host/mcom_inflate.cpp): `make -C minicom_amd/host fuzz_inflate_model`,
// then `fuzz_inflate_model DIR` with DIR holding BGZF members, one per file (tests/test_inflate.py writes them from tests/inflate_cases.py).
// Every member of the corpus and several thousand seeded mutations of them -- bit flips anywhere and in the payload alone, payloads cut
// short behind a header that says so, the first bytes of one payload spliced in front of another -- go through the twin with the payload
// and the output each in a heap block of exactly its size, so a byte read or written outside either is caught.  Every result is held
// against mcom_gunzip_member: the same accept / refuse verdict, and the same bytes where both accept.  No loop of the model may run on: a
// mutation that made one do so would hang this program, and the test that runs it has a time limit.
#include "../include/mcom_host.h"
#include "../minicom_amd/csrc/inflate_model.hpp"
#include "mcom_inflate.hpp"
#include <dirent.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace mcom_inflate_model;

namespace {

typedef std::vector<uint8_t> Bytes;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
uint64_t rnd(uint64_t n) { return n ? rnd() % n : 0; }

struct Heap {                                                     // a block of exactly n bytes (n = 0: one byte that nobody may touch)
	uint8_t *p; size_t n;
	explicit Heap(size_t n_) : p((uint8_t*)malloc(n_ ? n_ : 1)), n(n_) { if (!p) { fprintf(stderr, "no memory\n"); exit(2); } }
	~Heap() { free(p); }
	Heap(const Heap &) = delete;
	Heap &operator=(const Heap &) = delete;
};

unsigned long n_run = 0, n_compared = 0, n_accepted = 0, n_status[5] = {0, 0, 0, 0, 0};

// a member: header with the BC field, payload, trailer
Bytes wrap(const Bytes &payload, uint32_t crc, uint32_t isize)
{
	Bytes m = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0, 0};
	const size_t size = 18 + payload.size() + 8;
	m[16] = (uint8_t)((size - 1) & 255); m[17] = (uint8_t)((size - 1) >> 8);
	m.insert(m.end(), payload.begin(), payload.end());
	for (int k = 0; k < 4; ++k) m.push_back((uint8_t)(crc >> (8 * k)));
	for (int k = 0; k < 4; ++k) m.push_back((uint8_t)(isize >> (8 * k)));
	return m;
}

bool drive(const Bytes &member, const char *what)
{
	++n_run;
	Heap in(member.size());
	if (!member.empty()) memcpy(in.p, member.data(), member.size());
	Member M;
	uint64_t cnt = 0, text = 0, used = 0;
	const bool whole = walk_members(in.p, in.n, &M, 1, &cnt, &text, &used) && cnt == 1 && used == in.n;
	{	// the buffer form never faults, whatever it says
		uint64_t len = 0;
		Heap out(whole && M.isize <= (4u << 20) ? M.isize : 0);
		(void)mcomh_gzip_inflate(in.p, in.n, out.p, out.n, &len);
	}
	if (!whole || M.isize > (4u << 20)) return true;
	Heap pay((size_t)M.in_bytes), out(M.isize), ref(M.isize);
	if (pay.n) memcpy(pay.p, in.p + M.in_off, pay.n);
	memset(out.p, 0xAA, out.n ? out.n : 1);
	mcomh_gzip_member T;
	T.in_off = 0; T.in_bytes = M.in_bytes; T.out_off = 0; T.isize = M.isize; T.crc = M.crc;
	uint8_t st = 0xFF; uint64_t bad = 0, first = 0;
	if (mcomh_gzip_inflate_members(pay.p, pay.n, &T, 1, out.p, out.n, &st, &bad, &first) != 0 || st > 4 || bad != (st ? 1u : 0u)) {
		fprintf(stderr, "%s: the twin's own return values disagree (status %u, bad %llu)\n", what, st, (unsigned long long)bad);
		return false;
	}
	++n_status[st];
	size_t in_used = 0, out_n = 0;
	const int rc = mcom_gunzip_member(in.p, in.n, ref.p, ref.n, &in_used, &out_n);
	const bool ref_ok = rc == MCOM_INFLATE_OK && in_used == in.n;
	++n_compared;
	if ((st == 0) != ref_ok) {
		fprintf(stderr, "%s: the twin says %u, mcom_gunzip_member %d (used %zu of %zu)\n", what, st, rc, in_used, in.n);
		return false;
	}
	if (ref_ok) {
		++n_accepted;
		if (out_n != out.n || memcmp(out.p, ref.p, out.n)) { fprintf(stderr, "%s: both accept, the bytes differ\n", what); return false; }
	}
	return true;
}

}  // namespace

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: fuzz_inflate_model DIR\n"); return 2; }
	std::vector<std::string> names;
	if (DIR *d = opendir(argv[1])) {
		while (dirent *e = readdir(d)) if (e->d_name[0] != '.') names.push_back(e->d_name);
		closedir(d);
	}
	std::sort(names.begin(), names.end());
	struct Item { Bytes member, payload; uint32_t crc, isize; };
	std::vector<Item> corpus;
	for (const std::string &nm : names) {
		FILE *f = fopen((std::string(argv[1]) + "/" + nm).c_str(), "rb");
		if (!f) continue;
		Item it;
		uint8_t buf[65536]; size_t got;
		while ((got = fread(buf, 1, sizeof buf, f)) > 0) it.member.insert(it.member.end(), buf, buf + got);
		fclose(f);
		Member M; uint64_t cnt = 0, text = 0, used = 0;
		if (!walk_members(it.member.data(), it.member.size(), &M, 1, &cnt, &text, &used) || cnt != 1 || used != it.member.size()) { fprintf(stderr, "%s is not one BGZF member\n", nm.c_str()); return 1; }
		it.payload.assign(it.member.begin() + (size_t)M.in_off, it.member.begin() + (size_t)(M.in_off + M.in_bytes));
		it.crc = M.crc; it.isize = M.isize;
		corpus.push_back(it);
	}
	if (corpus.empty()) { fprintf(stderr, "no corpus in %s\n", argv[1]); return 1; }
	for (size_t i = 0; i < corpus.size(); ++i) if (!drive(corpus[i].member, names[i].c_str())) return 1;
	for (size_t i = 0; i < corpus.size(); ++i) {
		const Item &it = corpus[i];
		const size_t rounds = std::max<size_t>(8, std::min<size_t>(60, 400000 / (it.member.size() + 1)));
		for (size_t r = 0; r < rounds; ++r) {
			Bytes m;
			char what[96];
			const unsigned kind = (unsigned)rnd(5);
			if (kind == 0) {                                          // bit flips anywhere: headers, sizes and trailers too
				m = it.member;
				for (uint64_t k = 1 + rnd(3); k; --k) m[(size_t)rnd(m.size())] ^= (uint8_t)(1u << rnd(8));
			} else if (kind == 1 || it.payload.empty()) {             // bit flips in the payload alone: the walk still takes the member
				Bytes p = it.payload;
				for (uint64_t k = 1 + rnd(3); k && !p.empty(); --k) p[(size_t)rnd(std::min<size_t>(p.size(), r & 1 ? 64 : p.size()))] ^= (uint8_t)(1u << rnd(8));
				m = wrap(p, it.crc, it.isize);
			} else if (kind == 2) {                                   // a payload cut short, behind a header that says so
				Bytes p(it.payload.begin(), it.payload.begin() + (size_t)rnd(it.payload.size()));
				m = wrap(p, it.crc, it.isize);
			} else if (kind == 3) {                                   // the front of another payload (its block header) spliced in
				const Item &o = corpus[(size_t)rnd(corpus.size())];
				const size_t h = (size_t)rnd(std::min<size_t>(std::min(o.payload.size(), it.payload.size()), 120) + 1);
				Bytes p(o.payload.begin(), o.payload.begin() + h);
				p.insert(p.end(), it.payload.begin() + h, it.payload.end());
				if (p.size() + 26 > 65536) continue;
				m = wrap(p, it.crc, it.isize);
			} else {                                                  // a slot one byte short or long, a byte behind the last block
				Bytes p = it.payload;
				const unsigned sub = (unsigned)rnd(3);
				if (sub == 2) { p.push_back((uint8_t)rnd(256)); if (p.size() + 26 > 65536) continue; }
				m = wrap(p, it.crc, sub == 0 && it.isize ? it.isize - 1 : sub == 1 ? it.isize + 1 : it.isize);
			}
			snprintf(what, sizeof what, "%s mutation %zu (kind %u)", names[i].c_str(), r, kind);
			if (!drive(m, what)) return 1;
		}
	}
	printf("fuzz_inflate_model ok: %lu inputs, %lu held against mcom_gunzip_member (%lu accepted by both); statuses ok %lu corrupt %lu truncated %lu room %lu check %lu\n",
	       n_run, n_compared, n_accepted, n_status[0], n_status[1], n_status[2], n_status[3], n_status[4]);
	return 0;
}
