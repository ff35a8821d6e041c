// tests/fuzz_bgzf.cpp -- the BGZF writer's host twin (host/mcom_bgzf.cpp over csrc/deflate_model.hpp) under the sanitizers: random and
// mutated texts of random lengths around the block and tile boundaries go through mcomh_bgzf_encode, every member comes back through the
// project's own inflater (mcom_gunzip_member) and is compared.  Built by `make fuzz_bgzf` in minicom_amd/host, run by hand on the CPU:
//   ../lib/fuzz_bgzf [rounds] [seed]
#include "../include/mcom_host.h"
#include "mcom_inflate.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

static const uint32_t BLOCK = 65280;

// a text of n bytes: one of several shapes, then a few mutations
static void make_text(std::vector<uint8_t> &t, size_t n)
{
	t.resize(n);
	const uint32_t shape = below(6);
	const uint32_t alpha = shape == 0 ? 256 : shape == 1 ? 4 : shape == 2 ? 2 : 1 + below(40);
	for (size_t i = 0; i < n; ++i) t[i] = (uint8_t)(shape == 1 ? "ACGT"[below(4)] : 33 + below(alpha));
	if (shape >= 3 && n > 8) {                                               // copies of earlier stretches at all distances, and runs
		for (size_t i = 0; i < n; ) {
			const uint32_t len = 1 + below(shape == 5 ? 600 : 60);
			if (i > 0 && below(3)) {
				const size_t dist = 1 + (size_t)below((uint32_t)(i < 40000 ? i : 40000));
				for (uint32_t k = 0; k < len && i < n; ++k, ++i) t[i] = t[i - dist];
			} else i += len;
		}
	}
	for (uint32_t m = below(4); m && n; --m) t[below((uint32_t)n)] = (uint8_t)rnd();
}

static size_t pick_length()
{
	static const uint32_t edges[] = {0, 1, 2, 3, 4, 5, 8, 255, 256, 257, 258, 259, 260, 511, 512, 513, 516, 32767, 32768, 32769, 65023, 65024, 65025, 65279, 65280, 65281, 65536, 2 * 65280, 2 * 65280 + 1};
	const uint32_t kind = below(4);
	if (kind == 0) return below(3000);
	if (kind == 1) return below(3 * BLOCK);
	const uint32_t e = edges[below(sizeof edges / sizeof edges[0])];
	const int d = (int)below(7) - 3;
	return (size_t)((int)e + d < 0 ? 0 : (int)e + d);
}

int main(int argc, char **argv)
{
	const long rounds = argc > 1 ? atol(argv[1]) : 400;
	if (argc > 2) g_state ^= strtoull(argv[2], nullptr, 10) * 0x2545F4914F6CDD1Dull + 1;
	std::vector<uint8_t> text, coded, back(BLOCK + 16);
	for (long r = 0; r < rounds; ++r) {
		const size_t n = pick_length();
		make_text(text, n);
		const int flags = below(4) ? MCOMH_BGZF_EOF : 0;
		const uint64_t cap = mcomh_bgzf_bound(n);
		coded.assign((size_t)cap, 0);
		uint64_t len = 0;
		if (mcomh_bgzf_encode(text.data(), n, coded.data(), cap, &len, flags) || len > cap) { fprintf(stderr, "round %ld: encode of %zu bytes failed\n", r, n); return 1; }
		size_t at = 0, raw = 0;
		while (at < len) {
			size_t used = 0, got = 0;
			const int rc = mcom_gunzip_member(coded.data() + at, (size_t)len - at, back.data(), BLOCK, &used, &got);
			if (rc != MCOM_INFLATE_OK || used > 65536 || used != (size_t)(coded[at + 16] | coded[at + 17] << 8) + 1) { fprintf(stderr, "round %ld: member at %zu of %zu bytes: rc %d\n", r, at, n, rc); return 1; }
			if (raw + got > n || memcmp(back.data(), text.data() + raw, got) || (got != BLOCK && raw + got != n)) { fprintf(stderr, "round %ld: member at %zu differs\n", r, at); return 1; }
			if (got == 0 && !((flags & MCOMH_BGZF_EOF) && at + used == len && used == 28)) { fprintf(stderr, "round %ld: an empty member inside\n", r); return 1; }
			at += used; raw += got;
		}
		if (raw != n || ((flags & MCOMH_BGZF_EOF) && len < 28)) { fprintf(stderr, "round %ld: %zu bytes back for %zu\n", r, raw, n); return 1; }
		// a buffer one byte short is refused
		if (len && mcomh_bgzf_encode(text.data(), n, coded.data(), len - 1, &len, flags) != -4) { fprintf(stderr, "round %ld: a short buffer was not refused\n", r); return 1; }
	}
	printf("fuzz_bgzf: %ld rounds ok\n", rounds);
	return 0;
}
