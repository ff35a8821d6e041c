// tests/fuzz_entropy.cpp -- the host twin of the entropy stage (host/mcom_entropy.cpp, -DMCOM_ENTROPY_HOST_ONLY) under AddressSanitizer + UBSan
// (tests/test_entropy.py builds it with `make -C minicom_amd/host fuzz_entropy` and runs it on the CPU).
//   fuzz_entropy RAW_FILE CORPUS_FILE
// RAW_FILE is coded under every model hint and decoded again; then every record of CORPUS_FILE -- the member of the default choice cut at
// every length and hit by seeded single-bit flips, the corpus of the Python test -- is decoded.  Every hostile member lives in a heap block of exactly its size and decodes into a block of exactly
// the raw size, so a read or write one byte outside either is reported.  A hostile member must be refused or give the exact original.
#include "../include/mcom_host.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static std::vector<uint8_t> slurp(const char *path)
{
	std::vector<uint8_t> v;
	FILE *f = fopen(path, "rb");
	if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
	uint8_t buf[65536]; size_t got;
	while ((got = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + got);
	fclose(f);
	return v;
}

// 0 refused, 1 accepted and equal to raw; exits when accepted and different
static int judge(const uint8_t *member, size_t len, const std::vector<uint8_t> &raw, const char *what, unsigned long long at)
{
	uint8_t *m = (uint8_t*)malloc(len ? len : 1), *out = (uint8_t*)malloc(raw.size() ? raw.size() : 1);
	if (len) memcpy(m, member, len);
	uint64_t got = 0;
	const int rc = mcomh_rans_decode(m, len, out, raw.size(), &got);
	const bool same = !rc && got == raw.size() && (raw.empty() || !memcmp(out, raw.data(), raw.size()));
	free(m); free(out);
	if (!rc && !same) { fprintf(stderr, "WRONG OUTPUT WITH SUCCESS: %s at %llu\n", what, at); exit(1); }
	return rc ? 0 : 1;
}

int main(int argc, char **argv)
{
	if (argc != 3) { fprintf(stderr, "usage: fuzz_entropy RAW_FILE CORPUS_FILE\n"); return 2; }
	const std::vector<uint8_t> raw = slurp(argv[1]);
	std::vector<uint8_t> member(mcomh_rans_bound(raw.size()));
	const int hints[7] = {0x101, 0x111, 0x112, 0x114, 0x121, 0x122, 0x124};
	for (int h = 0; h < 7; ++h) {
		uint64_t len = 0;
		if (mcomh_rans_encode(raw.data(), raw.size(), member.data(), member.size(), &len, hints[h])) { fprintf(stderr, "encode failed, hint 0x%x\n", hints[h]); return 1; }
		if (!judge(member.data(), len, raw, "round trip, hint", (unsigned long long)hints[h])) { fprintf(stderr, "round trip refused, hint 0x%x\n", hints[h]); return 1; }
	}
	// the hostile corpus: records of { u32 length, bytes } (tests/entropy_cases.py hostile_corpus over the default member)
	const std::vector<uint8_t> corpus = slurp(argv[2]);
	long refused = 0, accepted = 0;
	for (size_t at = 0; at + 4 <= corpus.size(); ) {
		uint32_t len; memcpy(&len, &corpus[at], 4); at += 4;
		if (len > corpus.size() - at) { fprintf(stderr, "corpus file cut short\n"); return 2; }
		if (judge(corpus.data() + at, len, raw, "corpus record at byte", (unsigned long long)at)) ++accepted; else ++refused;
		at += len;
	}
	printf("fuzz_entropy ok: %zu raw bytes, %ld refused, %ld accepted\n", raw.size(), refused, accepted);
	return 0;
}
