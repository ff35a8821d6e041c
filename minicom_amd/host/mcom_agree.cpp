// minicom_amd/host/mcom_agree.cpp -- `minicom -a Q[:C]`: consensus-guided lossy quality values.
//
// mcomh_agree_mask         the agreement mask of a folder of stream files as a file: the mode is recognised as the decoders recognise it,
//                          then the matching decoder runs -- the host one with its member loop reporting to a McomAgreeSink
//                          (mcom_decompress.cpp), or the GPU one with coverage and mask between its phases B and C (mcom_decompress_gpu.cpp).
// mcomh_qual_agree         the plain C++ twin of mcom_qual_agree: the specification of the transform and its report.
// mcomh_qual_agree_marker  FOLDER/qual_agree.txt, `Q C` and a newline.
#include "../../include/mcom_host.h"
#include "mcom_agree.hpp"
#include "mcom_ragged.hpp"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {
bool exists(const std::string &path) { FILE *f = fopen(path.c_str(), "rb"); if (!f) return false; fclose(f); return true; }

// a canonical decimal number (no sign, no leading zero but "0" itself) of at most three digits at p; the byte behind it in *end
bool number(const char *p, const char **end, uint32_t &v)
{
	if (*p < '0' || *p > '9' || (*p == '0' && p[1] >= '0' && p[1] <= '9')) return false;
	v = 0;
	int digits = 0;
	while (*p >= '0' && *p <= '9') { if (++digits > 3) return false; v = v * 10 + (uint32_t)(*p - '0'); ++p; }
	*end = p;
	return true;
}
}  // namespace

extern "C" int mcomh_qual_agree(uint8_t *rows, uint64_t n_rows, uint32_t L, uint64_t pitch, const uint8_t *mask, uint64_t mask_pitch, uint64_t first_mask_row, uint32_t Q,
                                mcomh_qual_agree_report *report)
{
	if ((n_rows && (!rows || !mask)) || Q > 93 || L < 1 || L > 256 || pitch < L || mask_pitch < (uint64_t)((L + 7) / 8) || n_rows >= ((uint64_t)1 << 32)) return -1;
	mcomh_qual_agree_report r;
	memset(&r, 0, sizeof r);
	const uint8_t to = (uint8_t)(33 + Q);
	for (uint64_t j = 0; j < n_rows; ++j) {
		uint8_t *row = rows + j * pitch;
		const uint8_t *m = mask + (first_mask_row + j) * mask_pitch;
		for (uint32_t i = 0; i < L; ++i) {
			if (!((m[i >> 3] >> (i & 7)) & 1u)) continue;
			const uint64_t d = row[i] > to ? (uint64_t)(row[i] - to) : (uint64_t)(to - row[i]);
			++r.mask_bits; r.changed += d != 0; r.sum_abs += d; r.sum_sq += d * d; if (d > r.max_abs) r.max_abs = d;
			row[i] = to;
		}
	}
	if (report) *report = r;
	return 0;
}

extern "C" int mcomh_qual_agree_marker(const char *folder, uint32_t *Q, uint32_t *C)
{
	if (!folder) return -1;
	FILE *f = fopen((std::string(folder) + "/qual_agree.txt").c_str(), "rb");
	if (!f) return 0;
	char buf[16];
	const size_t got = fread(buf, 1, sizeof buf - 1, f);
	fclose(f);
	buf[got] = 0;
	if (got < 4 || got > 8 || strlen(buf) != got) return -1;               // "0 1\n" .. "93 255\n", no NUL inside
	const char *p = buf;
	uint32_t q = 0, c = 0;
	if (!number(p, &p, q) || *p != ' ' || !number(p + 1, &p, c) || p[0] != '\n' || p[1] != 0) return -1;
	if (q > 93 || c < 1 || c > 255) return -1;
	if (Q) *Q = q;
	if (C) *C = c;
	return 1;
}

extern "C" int mcomh_agree_mask(const char *folder, int C, const char *out_path, int device, uint64_t *n_rows, int *L, uint64_t *bits_set)
{
	if (!folder || !out_path) return -1;
	if (C < 1 || C > 255) { fprintf(stderr, "minicom agree mask: a coverage of %d (1 .. 255)\n", C); return -1; }
	try {
		const std::string dir(folder);
		if (mcom_ragged_present(folder)) { fprintf(stderr, "minicom agree mask: %s is a ragged archive (-V): its odd records lie in no contig\n", folder); return -1; }
		const bool order = exists(dir + "/ids.bin.0");
		if (!order && (exists(dir + "/file.bin.0") || exists(dir + "/file.bin.sp"))) {
			fprintf(stderr, "minicom agree mask: %s is a paired-end archive in the default mode: the row order of its decoder is not covered (use -p)\n", folder);
			return -1;
		}
		std::vector<uint8_t> mask;
		uint64_t n = 0; int len = 0;
		int rc;
		if (device < 0) rc = mcom_agree_mask_host(folder, order, C, mask, &n, &len);
		else {
#ifdef MCOM_ENTROPY_HOST_ONLY
			rc = -1;
#else
			rc = mcom_agree_mask_gpu(folder, order, C, device, mask, &n, &len);
#endif
		}
		if (rc) { if (device < 0) fprintf(stderr, "minicom agree mask: %s refused by the %s decoder\n", folder, order ? "-p" : "default"); return -1; }
		uint64_t bits = 0;
		for (uint8_t b : mask) bits += (uint64_t)__builtin_popcount(b);
		FILE *f = fopen(out_path, "wb");
		if (!f) return -1;
		const bool ok = mask.empty() || fwrite(mask.data(), 1, mask.size(), f) == mask.size();
		if (fclose(f) != 0 || !ok) { remove(out_path); return -1; }
		if (n_rows) *n_rows = n;
		if (L) *L = len;
		if (bits_set) *bits_set = bits;
		return 0;
	} catch (...) { return -1; }                                            // no C++ exception crosses the C boundary
}
