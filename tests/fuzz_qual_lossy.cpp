// tests/fuzz_qual_lossy.cpp -- the host twin of the lossy quality transform and its spec parser under the sanitizers (CPU only, by hand:
// `make -C minicom_amd/host fuzz_qual_lossy && minicom_amd/lib/fuzz_qual_lossy [rounds]`).  Random and mutated spec texts go through
// mcomh_qual_lossy_parse (whatever it takes must print back to the same text); random matrices at random pitches go through
// mcomh_qual_transform under every kind of spec: the bytes between the rows and around the matrix stay, a byte map applied twice
// changes nothing, a P-block moves no byte by more than P, the report is the difference of the two matrices, and a refused spec
// touches nothing.  Exit status 1 and a message at the first broken rule.
#include "../include/mcom_host.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

static int broken(const char *what, const std::string &detail)
{
	fprintf(stderr, "fuzz_qual_lossy: %s (%s)\n", what, detail.c_str());
	return 1;
}

int main(int argc, char **argv)
{
	const long rounds = argc > 1 ? atol(argv[1]) : 20000;
	std::mt19937_64 rng(12345);
	auto pick = [&](uint64_t n) { return (uint64_t)(rng() % n); };
	const char *seeds[] = {"ill8", "thr:20:6:37", "pblock:2", "pblock:47", "thr:1:0:93", "thr:93:92:93", "", "ill9", "pblock:0", "pblock:48", "thr:94:0:0", "pblock:01", "thr:20:6:37x"};
	const char alphabet[] = "0123456789:illthrpbock8 \n-+x";
	long taken = 0;
	for (long r = 0; r < rounds; ++r) {
		std::string t = seeds[pick(sizeof seeds / sizeof *seeds)];
		for (int m = (int)pick(4); m > 0; --m) {
			const int op = (int)pick(3);
			const size_t at = t.empty() ? 0 : pick(t.size() + 1);
			const char c = alphabet[pick(sizeof alphabet - 1)];
			if (op == 0) t.insert(t.begin() + at, c);
			else if (op == 1 && at < t.size()) t[at] = c;
			else if (op == 2 && at < t.size()) t.erase(t.begin() + at);
		}
		std::vector<char> text(t.begin(), t.end()); text.push_back(0);   // exactly as long as it is: a read past the NUL is the sanitizer's
		mcomh_qual_lossy_spec sp; memset(&sp, 0xEE, sizeof sp);
		if (mcomh_qual_lossy_parse(text.data(), &sp) == 0) {
			++taken;
			char back[32];
			if (mcomh_qual_lossy_print(&sp, back, sizeof back) || t != back) return broken("a spec that does not print back to its text", t);
			char small[4];
			if (t.size() + 1 > sizeof small && mcomh_qual_lossy_print(&sp, small, sizeof small) == 0) return broken("print into a buffer that is too small", t);
		}
	}
	for (long r = 0; r < rounds / 20 + 1; ++r) {
		const uint32_t L = 1 + (uint32_t)pick(256);
		const uint64_t n = pick(40), pitch = L + pick(5);
		std::vector<uint8_t> buf(16 + n * pitch + 16), before;
		for (auto &b : buf) b = (uint8_t)(pick(3) ? 33 + pick(94) : pick(256));
		before = buf;
		mcomh_qual_lossy_spec sp; memset(&sp, 0, sizeof sp);
		const int kind = 1 + (int)pick(4);
		sp.kind = (uint32_t)kind;
		if (kind == MCOMH_QUAL_LOSSY_THR) { sp.p[0] = (uint32_t)pick(96); sp.p[1] = (uint32_t)pick(96); sp.p[2] = (uint32_t)pick(96); }
		if (kind == MCOMH_QUAL_LOSSY_PBLOCK) sp.p[0] = (uint32_t)pick(50);
		if (kind == MCOMH_QUAL_LOSSY_LUT) { const uint32_t step = 1 + (uint32_t)pick(40); for (int v = 0; v < 256; ++v) sp.lut[v] = (uint8_t)(pick(8) ? v / step * step : pick(256)); }
		mcomh_qual_lossy_report rep = {7, 7, 7, 7};
		const int rc = mcomh_qual_transform(buf.data() + 16, n, L, pitch, &sp, &rep);
		if (rc) {
			if (buf != before || rep.changed != 7 || rep.max_abs != 7) return broken("a refused spec touched something", std::to_string(kind));
			continue;
		}
		mcomh_qual_lossy_report want = {0, 0, 0, 0};
		for (size_t i = 0; i < buf.size(); ++i) {
			const bool inside = i >= 16 && i < 16 + n * pitch && (i - 16) % pitch < L;
			if (!inside && buf[i] != before[i]) return broken("a byte outside the rows changed", std::to_string(i));
			const uint64_t d = buf[i] > before[i] ? buf[i] - before[i] : before[i] - buf[i];
			want.changed += d != 0; want.sum_abs += d; want.sum_sq += d * d; if (d > want.max_abs) want.max_abs = d;
		}
		if (memcmp(&want, &rep, sizeof rep)) return broken("the report is not the difference", std::to_string(kind));
		if (kind == MCOMH_QUAL_LOSSY_PBLOCK && rep.max_abs > sp.p[0]) return broken("a P-block moved a byte by more than P", std::to_string(sp.p[0]));
		if (kind != MCOMH_QUAL_LOSSY_PBLOCK) {
			std::vector<uint8_t> once = buf;
			if (mcomh_qual_transform(buf.data() + 16, n, L, pitch, &sp, &rep) || buf != once || rep.changed) return broken("a byte map applied twice changed something", std::to_string(kind));
		}
	}
	printf("fuzz_qual_lossy: %ld rounds, %ld spec texts taken, no rule broken\n", rounds, taken);
	return 0;
}
