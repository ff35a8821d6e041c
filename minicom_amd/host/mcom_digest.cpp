// minicom_amd/host/mcom_digest.cpp -- self-checking archives (`minicom -K`, `minicom -d`, `minicom -d -T`).
//
// The digest of a FASTQ file is sixteen 64-bit sums over per-record hashes of its lines (csrc/digest_model.hpp); digest.txt states them
// as text and travels in the archive as it is.  After a decode the output FILES are digested exactly as the input was and the keys that
// the archive's kind can answer are compared.
//   mcomh_fastq_record_hashes, mcomh_digest_reduce   plain C++ twins of the two device calls of csrc/digest.hip over the same model
//   mcomh_fastq_digest_files                         one or two files -> digest.txt; on GPU `device` through the piece loop that the quality,
//                                                    name and length passes use (plain, .gz; BGZF inflated on the card), device -1: the twins
//   mcomh_digest_parse, mcomh_digest_print           digest.txt <-> mcomh_digest; the parser refuses whatever the printer would not write
//   mcomh_digest_check                               the decoder's output files against folder/digest.txt
#include "../../include/mcom_host.h"
#include "../../include/mcom.h"
#include "../csrc/digest_model.hpp"
#include <dirent.h>
#include <zlib.h>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#ifndef MCOM_ENTROPY_HOST_ONLY
#include "mcom_ragged.hpp"
#include <hip/hip_runtime.h>
#endif

namespace dg = mcom_digest_model;

namespace {

const char *const KEY_NAME[dg::N_KEYS] = {"seq.ordered.1", "qual.ordered.1", "name.ordered.1", "seq.ordered.2", "qual.ordered.2", "name.ordered.2", "seq.multiset", "rec.multiset"};
const char HEADER[] = "minicom-digest 1\n";

int fail(char *err, size_t cap, const char *fmt, unsigned long long a = 0, unsigned long long b = 0)
{
	if (err && cap) snprintf(err, cap, fmt, a, b);
	return -1;
}
int bad_record(char *err, size_t cap, int lpr, unsigned long long record1)
{
	return lpr == 4 ? fail(err, cap, "record %llu is not a four-line FASTQ record: an '@' line, 1 .. 256 bases, a '+' line, as many quality values, at most 255 bytes behind the '@' and the '+'", record1)
	                : fail(err, cap, "record %llu is not a line of 1 .. 256 bases", record1);
}

bool write_file(const char *path, const void *p, size_t n)
{
	FILE *f = fopen(path, "wb");
	if (!f) return false;
	const bool ok = !n || fwrite(p, 1, n, f) == n;
	if (fclose(f) || !ok) { remove(path); return false; }
	return true;
}
bool slurp_file(const char *path, std::string &out, size_t at_most)
{
	FILE *f = fopen(path, "rb");
	if (!f) return false;
	char buf[4096]; size_t got;
	out.clear();
	while ((got = fread(buf, 1, sizeof buf, f)) > 0) { out.append(buf, got); if (out.size() > at_most) break; }
	const bool ok = !ferror(f) && out.size() <= at_most;
	fclose(f);
	return ok;
}
bool exists(const std::string &path)
{
	FILE *f = fopen(path.c_str(), "rb");
	if (!f) return false;
	fclose(f);
	return true;
}

// H of the line [p, p + m) of the text, for both seeds
void host_line(const uint8_t *p, size_t m, uint64_t h[2])
{
	uint64_t sum[2] = {0, 0};
	for (size_t j = 0; 8 * j < m; ++j) {
		uint64_t w = 0;
		const size_t nb = m - 8 * j < 8 ? m - 8 * j : 8;
		for (size_t q = 0; q < nb; ++q) w |= (uint64_t)p[8 * j + q] << (8 * q);
		for (int s = 0; s < 2; ++s) sum[s] += dg::word_term(w, j, dg::seed(s));
	}
	for (int s = 0; s < 2; ++s) h[s] = dg::line_hash(sum[s], m);
}

// the hash arrays of one file
struct Hashes { std::vector<uint64_t> S, Q, N; };

// the file inflated and held whole (a missing last newline is accepted), its line starts
int host_text(const char *path, std::vector<uint8_t> &text, std::vector<uint64_t> &start, char *err, size_t err_cap)
{
	gzFile f = gzopen(path, "rb");
	if (!f) return fail(err, err_cap, "cannot open the file");
	std::vector<uint8_t> buf((size_t)1 << 20);
	int got;
	text.clear();
	while ((got = gzread(f, buf.data(), (unsigned)buf.size())) > 0) text.insert(text.end(), buf.begin(), buf.begin() + got);
	gzclose(f);
	if (got < 0) return fail(err, err_cap, "cannot read the file (a damaged gzip stream?)");
	if (!text.empty() && text.back() != '\n') text.push_back('\n');
	start.assign(1, 0);
	for (size_t at = 0; at < text.size(); ) {
		const uint8_t *nl = (const uint8_t*)memchr(text.data() + at, '\n', text.size() - at);
		at = (size_t)(nl - text.data()) + 1;                                    // (there is one: the text ends with a newline)
		start.push_back(at);
	}
	return 0;
}

int host_hashes(const char *path, int lpr, bool with_qual, Hashes &H, uint64_t *n, char *err, size_t err_cap)
{
	std::vector<uint8_t> text;
	std::vector<uint64_t> start;
	if (host_text(path, text, start, err, err_cap)) return -1;
	const uint64_t lines = start.size() - 1, records = lines / (uint64_t)lpr;
	if (records >= ((uint64_t)1 << 32)) return fail(err, err_cap, "more than 2^32 records");
	H.S.assign(2 * records, 0);
	if (lpr == 4 && with_qual) H.Q.assign(2 * records, 0);
	if (lpr == 4) H.N.assign(2 * records, 0);
	uint32_t flag[2] = {0, 0xFFFFFFFFu};
	if (mcomh_fastq_record_hashes(text.data(), text.size(), start.data(), 0, records, lpr, records, H.S.data(), H.Q.empty() ? nullptr : H.Q.data(), H.N.empty() ? nullptr : H.N.data(), flag))
		return fail(err, err_cap, "the record hashes cannot be made");
	if (flag[0]) return bad_record(err, err_cap, lpr, (unsigned long long)flag[1] + 1);
	if (lines % (uint64_t)lpr) return fail(err, err_cap, "the file ends inside record %llu", (unsigned long long)(records + 1));   // (behind the records in front of it)
	*n = records;
	return 0;
}

#ifndef MCOM_ENTROPY_HOST_ONLY
struct DevHashes {                                          // the hash arrays of one file in HBM: they grow by doubling, the number of records is not known in advance
	uint64_t *h[3] = {nullptr, nullptr, nullptr};
	bool want[3] = {true, false, false};
	size_t cap = 0, held = 0;
	~DevHashes() { for (uint64_t *p : h) if (p) (void)hipFree(p); }
	bool room(size_t rows)
	{
		if (rows <= cap) return true;
		size_t to = cap ? cap : 65536;
		while (to < rows) to *= 2;
		for (int k = 0; k < 3; ++k) {
			if (!want[k]) continue;
			uint64_t *p = nullptr;
			if (hipMalloc((void**)&p, to * 16 + 16) != hipSuccess) return false;
			if (held && hipMemcpy(p, h[k], held * 16, hipMemcpyDeviceToDevice) != hipSuccess) { (void)hipFree(p); return false; }
			if (h[k]) (void)hipFree(h[k]);
			h[k] = p;
		}
		cap = to;
		return true;
	}
};

int device_hashes(mcom_ctx *ctx, const char *path, int device, int lpr, size_t piece_bytes, DevHashes &A, uint64_t *n, char *err, size_t err_cap)
{
	return mcom_fastq_for_each_piece(path, ctx, device, lpr, piece_bytes, [&](const uint8_t *d_text, uint64_t bytes, uint64_t records, const uint64_t *d_line_start, uint64_t first, uint32_t *d_flag) {
		if (first + records >= ((uint64_t)1 << 32)) return fail(err, err_cap, "more than 2^32 records");
		if (!A.room(first + records)) return fail(err, err_cap, "no room on the card");
		if (mcom_fastq_record_hashes(ctx, d_text, bytes, d_line_start, first, records, lpr, A.cap, A.h[0], A.h[1], A.h[2], d_flag)) {
			if (err && err_cap) snprintf(err, err_cap, "device call failed: %s", mcom_last_error(ctx));
			return -1;
		}
		uint32_t fl[4];
		if (hipMemcpy(fl, d_flag, 16, hipMemcpyDeviceToHost) != hipSuccess) return fail(err, err_cap, "cannot read the flag word");
		if (fl[0] || fl[2]) return bad_record(err, err_cap, lpr, (unsigned long long)fl[1] + 1);
		A.held = first + records;
		return 0;
	}, [&]() { A.held = 0; return true; }, n, err, err_cap);
}
#endif

// the sums of one or two files: which keys they answer is decided by what was hashed
int digest_of(const char *fastq1, const char *fastq2, int lpr, bool with_qual, int device, size_t piece_bytes, mcomh_digest &D, char *err, size_t err_cap)
{
	const char *path[2] = {fastq1, fastq2};
	const int files = fastq2 ? 2 : 1;
	uint64_t n[2] = {0, 0};
	memset(&D, 0, sizeof D);
	const bool qual = lpr == 4 && with_qual, names = lpr == 4;
	if (device < 0) {
		Hashes H[2];
		for (int f = 0; f < files; ++f) {
			char why[320] = "";
			if (host_hashes(path[f], lpr, with_qual, H[f], &n[f], why, sizeof why)) { if (err && err_cap) snprintf(err, err_cap, "%s: %s", path[f], why); return -1; }
		}
		if (files == 2 && n[0] != n[1]) return fail(err, err_cap, "the two files hold different numbers of records: %llu and %llu", (unsigned long long)n[0], (unsigned long long)n[1]);
		if (mcomh_digest_reduce(H[0].S.data(), qual ? H[0].Q.data() : nullptr, names ? H[0].N.data() : nullptr, files == 2 ? H[1].S.data() : nullptr,
		                        files == 2 && qual ? H[1].Q.data() : nullptr, files == 2 && names ? H[1].N.data() : nullptr, n[0], D.sums)) return fail(err, err_cap, "the sums cannot be made");
	} else {
#ifndef MCOM_ENTROPY_HOST_ONLY
		struct Ctx { mcom_ctx *c = nullptr; ~Ctx() { if (c) { (void)mcom_sync(c); mcom_destroy(c); } } } X;
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev) return fail(err, err_cap, "no GPU %llu (%llu visible)", (unsigned long long)device, (unsigned long long)n_dev);
		if (hipSetDevice(device) != hipSuccess || mcom_create(&X.c, device, nullptr) != MCOM_OK) { X.c = nullptr; return fail(err, err_cap, "cannot create a context on the GPU"); }
		DevHashes A[2];
		for (int f = 0; f < files; ++f) {
			char why[320] = "";
			A[f].want[1] = qual; A[f].want[2] = names;
			if (device_hashes(X.c, path[f], device, lpr, piece_bytes, A[f], &n[f], why, sizeof why)) { if (err && err_cap) snprintf(err, err_cap, "%s: %s", path[f], why); return -1; }
		}
		if (files == 2 && n[0] != n[1]) return fail(err, err_cap, "the two files hold different numbers of records: %llu and %llu", (unsigned long long)n[0], (unsigned long long)n[1]);
		if (mcom_digest_reduce(X.c, A[0].h[0], A[0].h[1], A[0].h[2], files == 2 ? A[1].h[0] : nullptr, files == 2 ? A[1].h[1] : nullptr, files == 2 ? A[1].h[2] : nullptr, n[0], D.sums)) {
			if (err && err_cap) snprintf(err, err_cap, "device call failed: %s", mcom_last_error(X.c));
			return -1;
		}
#else
		(void)piece_bytes;
		return fail(err, err_cap, "built without the device route");
#endif
	}
	D.files = (uint32_t)files; D.n = n[0];
	for (int f = 0; f < files; ++f) {
		D.present |= 1u << (dg::SEQ_ORDERED_1 + 3 * f);
		if (qual) D.present |= 1u << (dg::QUAL_ORDERED_1 + 3 * f);
		if (names) D.present |= 1u << (dg::NAME_ORDERED_1 + 3 * f);
	}
	D.present |= 1u << dg::SEQ_MULTISET;
	if (qual) D.present |= 1u << dg::REC_MULTISET;
	return 0;
}

// which sets of keys the printer writes: the sequence keys always, the quality keys together, the name keys together
bool present_ok(uint32_t files, uint32_t present)
{
	if (files != 1 && files != 2) return false;
	uint32_t must = 1u << dg::SEQ_ORDERED_1 | 1u << dg::SEQ_MULTISET, qual = 1u << dg::QUAL_ORDERED_1 | 1u << dg::REC_MULTISET, names = 1u << dg::NAME_ORDERED_1;
	if (files == 2) { must |= 1u << dg::SEQ_ORDERED_2; qual |= 1u << dg::QUAL_ORDERED_2; names |= 1u << dg::NAME_ORDERED_2; }
	if ((present & must) != must || (present & ~(must | qual | names))) return false;
	if ((present & qual) && (present & qual) != qual) return false;
	if ((present & names) && (present & names) != names) return false;
	return true;
}

// a canonical decimal number below 2^32 at [p, e), or -1
long long decimal(const char *p, const char *e)
{
	if (p >= e || e - p > 10 || (*p == '0' && e - p > 1)) return -1;
	long long v = 0;
	for (; p < e; ++p) { if (*p < '0' || *p > '9') return -1; v = v * 10 + (*p - '0'); }
	return v < ((long long)1 << 32) ? v : -1;
}
bool hex16(const char *p, uint64_t *v)
{
	*v = 0;
	for (int k = 0; k < 16; ++k) {
		const char c = p[k];
		if (c >= '0' && c <= '9') *v = *v << 4 | (uint64_t)(c - '0');
		else if (c >= 'a' && c <= 'f') *v = *v << 4 | (uint64_t)(c - 'a' + 10);
		else return false;
	}
	return true;
}

int refuse(char *why, size_t cap, const char *text) { if (why && cap) snprintf(why, cap, "%s", text); return -1; }

}  // namespace

extern "C" int mcomh_fastq_record_hashes(const uint8_t *text, uint64_t n_bytes, const uint64_t *line_start, uint64_t first_record, uint64_t n_records, int lines_per_record,
                                         uint64_t n_total, uint64_t *hS, uint64_t *hQ, uint64_t *hN, uint32_t *flag)
{
	if (!flag || (n_records && (!text || !line_start || !hS))) return -1;
	if ((lines_per_record != 4 && lines_per_record != 1) || n_total >= ((uint64_t)1 << 32) || first_record > n_total || n_records > n_total - first_record) return -1;
	const uint64_t *start = line_start;
	for (uint64_t r = 0; r < n_records; ++r) {
		uint32_t bad = 0;
		uint64_t a = 0, b = 0, c = 0, d = 0, sl = 0;
		if (lines_per_record == 4) {
			a = start[4 * r]; b = start[4 * r + 1]; c = start[4 * r + 2]; d = start[4 * r + 3];
			const uint64_t e = start[4 * r + 4];
			if (!(a < b && b < c && c < d && d < e && e <= n_bytes)) bad = MCOM_FASTQ_F_LENGTH;
			else {
				if (b - 1 - a < 1 || text[a] != '@') bad |= MCOM_FASTQ_F_NAME;
				if (d - 1 - c < 1 || text[c] != '+') bad |= MCOM_FASTQ_F_PLUS;
				sl = c - 1 - b;
				if (e - 1 - d != sl || sl < 1 || sl > dg::LINE_BYTES) bad |= MCOM_FASTQ_F_LENGTH;
				if (!bad && (b - 2 - a > dg::NAME_BYTES || d - 2 - c > dg::NAME_BYTES)) bad |= MCOM_FASTQ_F_LONG;
			}
		} else {
			b = start[r];
			const uint64_t e = start[r + 1];
			if (!(b < e && e <= n_bytes)) bad = MCOM_FASTQ_F_LENGTH;
			else { sl = e - 1 - b; if (sl < 1 || sl > dg::LINE_BYTES) bad = MCOM_FASTQ_F_LENGTH; }
		}
		if (bad) { flag[0] |= bad; if ((uint32_t)(first_record + r) < flag[1]) flag[1] = (uint32_t)(first_record + r); continue; }
		const uint64_t at = 2 * (first_record + r);
		host_line(text + b, (size_t)sl, hS + at);
		if (lines_per_record != 4) continue;
		if (hQ) host_line(text + d, (size_t)sl, hQ + at);
		if (hN) {
			uint64_t h[2], g[2];
			host_line(text + a + 1, (size_t)(b - 2 - a), h);
			host_line(text + c + 1, (size_t)(d - 2 - c), g);
			for (int s = 0; s < 2; ++s) hN[at + s] = dg::combine(h[s], g[s], dg::seed(s));
		}
	}
	return 0;
}

extern "C" int mcomh_digest_reduce(const uint64_t *hS1, const uint64_t *hQ1, const uint64_t *hN1, const uint64_t *hS2, const uint64_t *hQ2, const uint64_t *hN2, uint64_t n, uint64_t sums[16])
{
	if (!sums || (n && !hS1)) return -1;
	for (int k = 0; k < dg::N_SUMS; ++k) sums[k] = 0;
	if (n >= ((uint64_t)1 << 32)) return -1;
	if ((!hS2 && (hQ2 || hN2)) || (hS2 && ((hQ1 != nullptr) != (hQ2 != nullptr) || (hN1 != nullptr) != (hN2 != nullptr)))) return -1;
	for (uint64_t i = 0; i < n; ++i)
		for (int s = 0; s < 2; ++s) {
			const uint64_t K = dg::seed(s), s1 = hS1[2 * i + s];
			uint64_t rs = s1, rr = 0;
			sums[2 * dg::SEQ_ORDERED_1 + s] += dg::ordered_term(s1, i, K);
			if (hQ1) { const uint64_t q1 = hQ1[2 * i + s]; sums[2 * dg::QUAL_ORDERED_1 + s] += dg::ordered_term(q1, i, K); rr = dg::combine(s1, q1, K); }
			if (hN1) sums[2 * dg::NAME_ORDERED_1 + s] += dg::ordered_term(hN1[2 * i + s], i, K);
			if (hS2) {
				const uint64_t s2 = hS2[2 * i + s];
				sums[2 * dg::SEQ_ORDERED_2 + s] += dg::ordered_term(s2, i, K);
				rs = dg::combine(s1, s2, K);
				if (hQ2) { const uint64_t q2 = hQ2[2 * i + s]; sums[2 * dg::QUAL_ORDERED_2 + s] += dg::ordered_term(q2, i, K); rr = dg::combine(rr, dg::combine(s2, q2, K), K); }
				if (hN2) sums[2 * dg::NAME_ORDERED_2 + s] += dg::ordered_term(hN2[2 * i + s], i, K);
			}
			sums[2 * dg::SEQ_MULTISET + s] += dg::multiset_term(rs);
			if (hQ1) sums[2 * dg::REC_MULTISET + s] += dg::multiset_term(rr);
		}
	return 0;
}

extern "C" int mcomh_digest_print(const mcomh_digest *d, char *out, size_t cap, size_t *len)
{
	if (!d || !len || !present_ok(d->files, d->present) || d->n >= ((uint64_t)1 << 32)) return -1;
	std::string t(HEADER);
	char line[96];
	snprintf(line, sizeof line, "files %u\nn %llu\n", d->files, (unsigned long long)d->n);
	t += line;
	for (int k = 0; k < dg::N_KEYS; ++k) {
		if (!(d->present >> k & 1)) continue;
		snprintf(line, sizeof line, "%s %016llx %016llx\n", KEY_NAME[k], (unsigned long long)d->sums[2 * k], (unsigned long long)d->sums[2 * k + 1]);
		t += line;
	}
	*len = t.size();
	if (!out) return 0;
	if (t.size() > cap) return -2;
	memcpy(out, t.data(), t.size());
	return 0;
}

extern "C" int mcomh_digest_parse(const char *text, size_t bytes, mcomh_digest *out, char *why, size_t why_cap)
{
	if (!text || !out) return refuse(why, why_cap, "null pointer");
	memset(out, 0, sizeof *out);
	if (bytes > 1024) return refuse(why, why_cap, "longer than any digest");
	if (!bytes || text[bytes - 1] != '\n') return refuse(why, why_cap, "no newline at the end");
	if (memchr(text, 0, bytes)) return refuse(why, why_cap, "a zero byte");
	const char *p = text, *const end = text + bytes;
	auto next_line = [&](const char *&b, const char *&e) { b = p; e = (const char*)memchr(p, '\n', (size_t)(end - p)); p = e + 1; };   // (there is one: the text ends with a newline)
	const char *b, *e;
	next_line(b, e);
	if ((size_t)(e + 1 - b) != sizeof HEADER - 1 || memcmp(b, HEADER, sizeof HEADER - 1)) return refuse(why, why_cap, "the first line is not `minicom-digest 1`");
	if (p >= end) return refuse(why, why_cap, "no `files` line");
	next_line(b, e);
	if (e - b != 7 || memcmp(b, "files ", 6) || (b[6] != '1' && b[6] != '2')) return refuse(why, why_cap, "the second line is not `files 1` or `files 2`");
	out->files = (uint32_t)(b[6] - '0');
	if (p >= end) return refuse(why, why_cap, "no `n` line");
	next_line(b, e);
	const long long n = e - b > 2 && !memcmp(b, "n ", 2) ? decimal(b + 2, e) : -1;
	if (n < 0) return refuse(why, why_cap, "the third line is not `n` and a decimal number below 2^32 without leading zeros");
	out->n = (uint64_t)n;
	int last = -1;
	while (p < end) {
		next_line(b, e);
		const char *sp = (const char*)memchr(b, ' ', (size_t)(e - b));
		int key = -1;
		for (int k = 0; sp && k < dg::N_KEYS; ++k) if ((size_t)(sp - b) == strlen(KEY_NAME[k]) && !memcmp(b, KEY_NAME[k], (size_t)(sp - b))) key = k;
		if (key < 0) return refuse(why, why_cap, "an unknown key");
		if (out->present >> key & 1) return refuse(why, why_cap, "a key given twice");
		if (key < last) return refuse(why, why_cap, "the keys are not in their order");
		if (e - sp != 34 || sp[17] != ' ' || !hex16(sp + 1, &out->sums[2 * key]) || !hex16(sp + 18, &out->sums[2 * key + 1])) return refuse(why, why_cap, "a value is not two words of sixteen lower-case hexadecimal digits");
		out->present |= 1u << key; last = key;
	}
	if (!present_ok(out->files, out->present)) return refuse(why, why_cap, "the keys are not those of a digest of this many files");
	return 0;
}

extern "C" int mcomh_fastq_digest_files(const char *fastq1, const char *fastq2, int lines_per_record, int with_qual, int device, size_t piece_bytes, const char *out_path, uint64_t *n,
                                        char *err, size_t err_cap)
{
	if (!fastq1 || !out_path || !n) return fail(err, err_cap, "null pointer");
	*n = 0;
	if (lines_per_record != 4 && lines_per_record != 1) return fail(err, err_cap, "records of %llu lines (4, or 1 for a file of one read per line)", (unsigned long long)lines_per_record);
	try {
		mcomh_digest D;
		if (digest_of(fastq1, fastq2, lines_per_record, with_qual != 0, device, piece_bytes, D, err, err_cap)) return -1;
		if (!D.n) return fail(err, err_cap, "the file holds no record");
		char text[1024]; size_t len = 0;
		if (mcomh_digest_print(&D, text, sizeof text, &len)) return fail(err, err_cap, "the digest cannot be written");
		if (!write_file(out_path, text, len)) return fail(err, err_cap, "cannot write the digest file");
		*n = D.n;
		return 0;
	} catch (...) { return fail(err, err_cap, "out of memory"); }
}

extern "C" int mcomh_digest_check(const char *folder, const char *out1, const char *out2, int device, mcomh_digest_report *rep)
{
	if (!rep) return -1;
	memset(rep, 0, sizeof *rep);
	rep->first_diff = -1;
	auto refused = [&](const char *text) { snprintf(rep->message, sizeof rep->message, "%s", text); return -1; };
	if (!folder || !out1) return refused("null pointer");
	try {
		const std::string dir(folder);
		std::string text;
		if (!slurp_file((dir + "/digest.txt").c_str(), text, 1024)) return refused("the archive holds no digest.txt (made without -K), or it cannot be read");
		mcomh_digest want, got;
		char why[128] = "";
		if (mcomh_digest_parse(text.data(), text.size(), &want, why, sizeof why)) { snprintf(rep->message, sizeof rep->message, "digest.txt is not a digest: %s", why); return -1; }
		const int files = out2 ? 2 : 1;
		if ((int)want.files != files) return refused(files == 2 ? "digest.txt is that of one file, the archive gave two" : "digest.txt is that of a pair, the archive gave one file");
		// the archive's kind: the list of ids of the order-preserving modes (packed, as a tar or taken out of it), the quality members in the archive's own order, a name member
		bool input_order = false;
		if (DIR *dp = opendir(folder)) {
			while (const dirent *de = readdir(dp)) {
				const std::string nm(de->d_name);
				if (nm.rfind("idsbin.tar", 0) == 0 || nm.rfind("ids.bin.", 0) == 0 || (nm.size() >= 8 && nm.compare(nm.size() - 8, 8, ".ids.bin") == 0)) input_order = true;
			}
			closedir(dp);
		} else return refused("the folder cannot be read");
		const bool own_qual = exists(dir + "/rqual.mcq") || exists(dir + "/rqual_1.mcq");
		const bool names = exists(dir + "/name.mcn") || exists(dir + "/name_1.mcn");
		// the decoders write FASTQ exactly when the archive holds quality values or names, one read per line otherwise
		bool fastq = own_qual || names;
		for (const char *m : {"/qual.mcq", "/qual_1.mcq", "/qual_2.mcq", "/rqual_2.mcq", "/name_2.mcn"}) fastq = fastq || exists(dir + m);
		const int lpr = fastq ? 4 : 1;
		char err[400] = "";
		if (digest_of(out1, out2, lpr, true, device, 0, got, err, sizeof err)) { snprintf(rep->message, sizeof rep->message, "%.*s", (int)sizeof rep->message - 1, err); return -1; }
		rep->files = (uint32_t)files; rep->n_stored = want.n; rep->n_output = got.n;
		uint32_t ask = 0;
		if (input_order)
			for (int f = 0; f < files; ++f) {
				ask |= 1u << (dg::SEQ_ORDERED_1 + 3 * f);
				if (lpr == 4) ask |= 1u << (dg::QUAL_ORDERED_1 + 3 * f);
				if (lpr == 4 && names) ask |= 1u << (dg::NAME_ORDERED_1 + 3 * f);
			}
		else ask = own_qual && lpr == 4 && (want.present >> dg::REC_MULTISET & 1) ? 1u << dg::REC_MULTISET : 1u << dg::SEQ_MULTISET;
		ask &= want.present & got.present;
		rep->compared = ask;
		rep->identical = want.n == got.n;
		if (!rep->identical) rep->first_diff = -2;
		for (int k = 0; k < dg::N_KEYS; ++k) {
			if (!(ask >> k & 1)) continue;
			if (want.sums[2 * k] == got.sums[2 * k] && want.sums[2 * k + 1] == got.sums[2 * k + 1]) continue;
			rep->differing |= 1u << k;
			if (rep->identical) rep->first_diff = k;
			rep->identical = 0;
		}
		return 0;
	} catch (...) { return refused("out of memory"); }
}
