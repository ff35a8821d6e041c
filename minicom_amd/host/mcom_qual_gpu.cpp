// minicom_amd/host/mcom_qual_gpu.cpp -- the quality lines of a FASTQ file as rows in HBM, and the check of an archive's qual.mcq
// against them.
//
// mcomh_fastq_qualities_to_device: the text (plain or gzip: zlib's reader takes both) goes up through two page-locked pieces; while
// piece i is on its way, piece i + 1 is read.  Where a piece ends inside a record, the record's beginning is carried in front of the
// next piece: the host counts the piece's newlines for that (four lines are a record), nothing else is parsed on the host.  On the
// card mcom_decode_line_index finds the lines and mcom_fastq_quality_rows checks every record and gathers its quality line.  A file
// the kernel flags is an error that names the first bad record; it is not handed to another parser.
// A BGZF file is not inflated on the host at all: its members go up compressed and mcom_gz_device_route (mcom_gzip_gpu.cpp, DESIGN.md section
// 3.15) inflates them on the card in front of the same two kernels; whatever is off there starts the file again through the route above.
// mcomh_verify_quality_gpu: qual.mcq decoded by mcom_qual_decode, the file's rows as above, mcom_verify_ordered over both.
// `minicom -b SPEC`: the `_lossy` file calls send the rows through mcom_qual_transform (device -1: its host twin,
// host/mcom_qual_lossy.cpp) in front of the coder, and the verifiers send the file's rows through it when the folder holds qual_lossy.txt.
#include "../../include/mcom_host.h"
#include "../../include/mcom.h"
#include "mcom_fastq.hpp"
#include "mcom_gzip_gpu.hpp"
#include "mcom_agree.hpp"
#include <hip/hip_runtime.h>
#include <zlib.h>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

const size_t DEFAULT_PIECE = (size_t)32 << 20;
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Job {                                                // what one call holds, released however it ends
	mcom_ctx *ctx = nullptr; hipStream_t copy = nullptr; hipEvent_t ev[2] = {nullptr, nullptr};
	uint8_t *pin[2] = {nullptr, nullptr}, *d_text[2] = {nullptr, nullptr}, *d_rows = nullptr;
	uint64_t *d_start = nullptr; uint32_t *d_flag = nullptr;
	gzFile f = nullptr;
	~Job()
	{
		if (copy) (void)hipStreamSynchronize(copy);
		if (ctx) (void)mcom_sync(ctx);
		if (f) gzclose(f);
		for (int k = 0; k < 2; ++k) { if (pin[k]) (void)hipHostFree(pin[k]); if (d_text[k]) (void)hipFree(d_text[k]); if (ev[k]) (void)hipEventDestroy(ev[k]); }
		if (d_start) (void)hipFree(d_start);
		if (d_flag) (void)hipFree(d_flag);
		if (d_rows) (void)hipFree(d_rows);
		if (copy) (void)hipStreamDestroy(copy);
		if (ctx) mcom_destroy(ctx);
	}
};

int fail(char *err, size_t cap, const char *fmt, unsigned long long a = 0, unsigned long long b = 0)
{
	if (err && cap) snprintf(err, cap, fmt, a, b);
	return -1;
}

// is it a spec the transform takes?  Asked before a file is read: a refused spec does no work and writes nothing
bool spec_ok(const mcomh_qual_lossy_spec *spec)
{
	uint8_t none = 0;
	return mcomh_qual_transform(&none, 0, 1, 1, spec, nullptr) == 0;
}

void record_message(char *err, size_t cap, unsigned long long record1, int L, uint32_t bits)
{
	if (err && cap) snprintf(err, cap, "record %llu is not a four-line FASTQ record of %d bases and %d quality values in 33 .. 126:%s%s%s%s", record1, L, L,
	                         bits & MCOM_FASTQ_F_NAME ? " no '@' line" : "", bits & MCOM_FASTQ_F_PLUS ? " no '+' line" : "",
	                         bits & MCOM_FASTQ_F_LENGTH ? " a line of another length (a CR before the newline counts)" : "", bits & MCOM_FASTQ_F_CHAR ? " a quality byte outside 33 .. 126" : "");
}

int qualities(const char *path, int device, int L, size_t piece_bytes, uint8_t **d_rows_out, size_t *n_out, char *err, size_t err_cap)
{
	if (!path || !d_rows_out || !n_out) return fail(err, err_cap, "null pointer");
	*d_rows_out = nullptr; *n_out = 0;
	if (L < 1 || L > 256) return fail(err, err_cap, "reads of %llu characters (1 .. 256)", (unsigned long long)L);
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return fail(err, err_cap, "no GPU %llu (%llu visible)", (unsigned long long)device, (unsigned long long)n_dev);
	if (hipSetDevice(device) != hipSuccess) return fail(err, err_cap, "cannot select the GPU");
	size_t piece = piece_bytes ? piece_bytes : DEFAULT_PIECE;
	const size_t least = 4 * (2 * (size_t)L + 64);                        // a piece holds a few records at least (names of up to ~50 characters):
	if (piece < least) piece = least;                                      // the documented minimum (include/mcom_host.h), 552 bytes at L = 37
	Job J;
	J.f = gzopen(path, "rb");
	if (!J.f) return fail(err, err_cap, "cannot open the file");
	if (mcom_create(&J.ctx, device, nullptr) != MCOM_OK) { J.ctx = nullptr; return fail(err, err_cap, "cannot create a context on the GPU"); }
	if (hipStreamCreate(&J.copy) != hipSuccess) return fail(err, err_cap, "no stream");
	if (hipMalloc((void**)&J.d_flag, 16) != hipSuccess) return fail(err, err_cap, "no room on the card");
	size_t cap_rows = 0, n = 0, cap_lines = 0;
	auto room_for = [&](size_t rows) {                                     // the table grows by doubling: the number of records is not known in advance
		if (rows <= cap_rows) return true;
		size_t want = cap_rows ? cap_rows : 4096;
		while (want < rows) want *= 2;
		uint8_t *p = nullptr;
		if (hipMalloc((void**)&p, want * (size_t)L + 16) != hipSuccess) return false;
		if (n && hipMemcpy(p, J.d_rows, n * (size_t)L, hipMemcpyDeviceToDevice) != hipSuccess) { (void)hipFree(p); return false; }
		if (J.d_rows) (void)hipFree(J.d_rows);
		J.d_rows = p; cap_rows = want;
		return true;
	};
	// fill: `have` carried bytes are in front already; *eof when the file ended (a missing last newline is added)
	auto fill = [&](uint8_t *buf, size_t have, size_t &len, bool &eof) {
		len = have; eof = false;
		while (len < piece) {
			const int got = gzread(J.f, buf + len, (unsigned)(piece - len < ((size_t)1 << 30) ? piece - len : (size_t)1 << 30));
			if (got < 0) return false;
			if (got == 0) { eof = true; break; }
			len += (size_t)got;
		}
		if (eof && len && buf[len - 1] != '\n') buf[len++] = '\n';        // (room: the buffers are piece + 1 bytes)
		return true;
	};
	// the bytes of the whole records in buf[0 .. len) and their number
	auto whole_records = [&](const uint8_t *buf, size_t len, size_t &bytes, size_t &records, size_t &lines) {
		lines = 0; bytes = 0; records = 0;
		const uint8_t *p = buf, *const e = buf + len;
		while (p < e) { const uint8_t *q = (const uint8_t*)memchr(p, '\n', (size_t)(e - p)); if (!q) break; p = q + 1; if ((++lines & 3) == 0) { bytes = (size_t)(p - buf); records = lines / 4; } }
	};
	// A BGZF file goes up compressed and is inflated on the card (mcom_gzip_gpu.cpp): the same kernels over the same
	// records.  Whatever is off there -- also a record the kernel flags -- sends the file to zlib's reader below, from its beginning.
	const bool on_device = mcom_gz_device_route(path, J.ctx, piece, [&](const uint8_t *d_text, uint64_t bytes, uint64_t records, const uint64_t *d_line_start) {
		if (n + records >= ((size_t)1 << 32) || !room_for(n + records)) return false;
		const uint32_t init[4] = {0, 0xFFFFFFFFu, 0, 0};
		uint32_t fl[4];
		if (hipMemcpy(J.d_flag, init, 16, hipMemcpyHostToDevice) != hipSuccess ||
		    mcom_fastq_quality_rows(J.ctx, d_text, bytes, d_line_start, n, records, (uint32_t)L, J.d_rows, (uint64_t)L, J.d_flag) ||
		    hipMemcpy(fl, J.d_flag, 16, hipMemcpyDeviceToHost) != hipSuccess || fl[0] || fl[2]) return false;
		n += records;
		return true;
	});
	if (!on_device) n = 0;
	auto zlib_route = [&]() -> int {
	for (int k = 0; k < 2; ++k)
		if (hipHostMalloc((void**)&J.pin[k], piece + 1, hipHostMallocDefault) != hipSuccess || hipMalloc((void**)&J.d_text[k], piece + 16) != hipSuccess ||
		    hipEventCreateWithFlags(&J.ev[k], hipEventDisableTiming) != hipSuccess) return fail(err, err_cap, "no room for the pieces");
	size_t len = 0; bool eof = false;
	if (!fill(J.pin[0], 0, len, eof)) return fail(err, err_cap, "cannot read the file (a damaged gzip stream?)");
	for (int k = 0; ; k ^= 1) {
		size_t bytes, records, lines;
		whole_records(J.pin[k], len, bytes, records, lines);
		if (eof && bytes != len) return fail(err, err_cap, "the file ends inside record %llu", (unsigned long long)(n + records + 1));
		if (!eof && !records) return fail(err, err_cap, "record %llu is longer than a piece of %llu bytes", (unsigned long long)(n + 1), (unsigned long long)piece);
		if (n + records >= ((size_t)1 << 32)) return fail(err, err_cap, "more than 2^32 records");
		if (bytes && (hipMemcpyAsync(J.d_text[k], J.pin[k], bytes, hipMemcpyHostToDevice, J.copy) != hipSuccess || hipEventRecord(J.ev[k], J.copy) != hipSuccess)) return fail(err, err_cap, "upload failed");
		// the next piece is read while this one travels: its front is this piece's unfinished record
		size_t next_len = 0; bool next_eof = true;
		if (!eof) {
			memcpy(J.pin[k ^ 1], J.pin[k] + bytes, len - bytes);
			if (!fill(J.pin[k ^ 1], len - bytes, next_len, next_eof)) return fail(err, err_cap, "cannot read the file (a damaged gzip stream?)");
		}
		if (records) {
			if (hipEventSynchronize(J.ev[k]) != hipSuccess) return fail(err, err_cap, "upload failed");
			if (4 * records + 1 > cap_lines) {
				if (J.d_start) (void)hipFree(J.d_start);
				J.d_start = nullptr; cap_lines = 4 * records + 1;
				if (hipMalloc((void**)&J.d_start, cap_lines * 8 + 16) != hipSuccess) return fail(err, err_cap, "no room on the card");
			}
			if (!room_for(n + records)) return fail(err, err_cap, "no room on the card for %llu rows", (unsigned long long)(n + records));
			const uint32_t init[4] = {0, 0xFFFFFFFFu, 0, 0};
			if (hipMemcpy(J.d_flag, init, 16, hipMemcpyHostToDevice) != hipSuccess) return fail(err, err_cap, "upload failed");
			uint64_t got_lines = 0;
			if (mcom_decode_line_index(J.ctx, J.d_text[k], bytes, J.d_start, 4 * records, &got_lines, J.d_flag + 2) || got_lines != 4 * records ||
			    mcom_fastq_quality_rows(J.ctx, J.d_text[k], bytes, J.d_start, n, records, (uint32_t)L, J.d_rows, (uint64_t)L, J.d_flag)) {
				if (err && err_cap) snprintf(err, err_cap, "device call failed: %s", mcom_last_error(J.ctx));
				return -1;
			}
			uint32_t fl[4];
			if (hipMemcpy(fl, J.d_flag, 16, hipMemcpyDeviceToHost) != hipSuccess) return fail(err, err_cap, "cannot read the flag word");
			if (fl[0] || fl[2]) {
				record_message(err, err_cap, (unsigned long long)fl[1] + 1, L, fl[0]);
				return -1;
			}
			n += records;
		}
		if (eof) break;
		len = next_len; eof = next_eof;
	}
	return 0;
	};
	if (!on_device) { const int rc = zlib_route(); if (rc) return rc; }
	if (!n && !room_for(1)) return fail(err, err_cap, "no room on the card");
	*d_rows_out = J.d_rows; J.d_rows = nullptr;
	*n_out = n;
	return 0;
}

// member: the `.mcq` member of the folder that holds the file's quality rows in input order (qual.mcq; qual_1.mcq / qual_2.mcq of a pair)
int verify_quality(const char *folder, const char *member_name, const char *fastq, int device, mcomh_verify_report *rep)
{
	const double t_begin = now_ms();
	std::vector<uint8_t> member;
	{
		FILE *f = fopen((std::string(folder) + "/" + member_name).c_str(), "rb");
		if (!f) { fprintf(stderr, "minicom verify: %s has no %s\n", folder, member_name); return -1; }
		uint8_t buf[65536]; size_t got;
		while ((got = fread(buf, 1, sizeof buf, f)) > 0) member.insert(member.end(), buf, buf + got);
		fclose(f);
	}
	uint64_t qn = 0; uint32_t qL = 0;
	if (mcom_qual_info(member.data(), member.size(), &qn, &qL)) { fprintf(stderr, "minicom verify: %s/%s is not a .mcq member\n", folder, member_name); return -1; }
	struct Rows { uint8_t *d = nullptr; ~Rows() { mcomh_device_free(d); } } in;
	size_t n_in = 0;
	char err[320] = "";
	if (qualities(fastq, device, (int)qL, 0, &in.d, &n_in, err, sizeof err)) { fprintf(stderr, "minicom verify: cannot read the qualities of %s: %s\n", fastq, err); return -1; }
	// an archive made with -a holds the file's rows under its own agreement mask (section 3.17): rows [n, 2 n) of it for the second file of a pair
	if (mcom_qual_agree_apply_marker(folder, device, in.d, n_in, (int)qL, strcmp(member_name, "qual_2.mcq") ? 0 : qn)) return -1;
	if (mcom_qual_lossy_apply_marker(folder, device, in.d, n_in, (int)qL)) return -1;   // an archive made with -b holds T(file): section 3.13
	const double ingest = now_ms() - t_begin;
	struct Dev { mcom_ctx *ctx = nullptr; uint8_t *d_member = nullptr, *d_rows = nullptr; ~Dev() { if (ctx) (void)mcom_sync(ctx); if (d_member) (void)hipFree(d_member); if (d_rows) (void)hipFree(d_rows); if (ctx) mcom_destroy(ctx); } } D;
	if (mcom_create(&D.ctx, device, nullptr) != MCOM_OK) { D.ctx = nullptr; return -1; }
	if (hipMalloc((void**)&D.d_member, member.size() + 16) != hipSuccess || hipMalloc((void**)&D.d_rows, qn * qL + 16) != hipSuccess) { fprintf(stderr, "minicom verify: the card has no room for the quality rows\n"); return -1; }
	if (hipMemcpy(D.d_member, member.data(), member.size(), hipMemcpyHostToDevice) != hipSuccess) return -1;
	double t0 = now_ms();
	uint64_t gn = 0; uint32_t gL = 0;
	if (mcom_qual_decode(D.ctx, D.d_member, member.size(), D.d_rows, qL, qn, &gn, &gL)) { fprintf(stderr, "minicom verify: %s/%s refused: %s\n", folder, member_name, mcom_last_error(D.ctx)); return -1; }
	rep->times_ms[2] = now_ms() - t0;
	mcom_verify_table a, b;
	a.d_rows = in.d; a.pitch = qL; a.n = n_in; a.d_mates = nullptr;
	b.d_rows = D.d_rows; b.pitch = qL; b.n = qn; b.d_mates = nullptr;
	mcom_verify_report r;
	t0 = now_ms();
	if (mcom_verify_ordered(D.ctx, &a, &b, (int)qL, &r)) { fprintf(stderr, "minicom verify: %s\n", mcom_last_error(D.ctx)); return -1; }
	rep->times_ms[3] = now_ms() - t0;
	rep->mode = 1;
	rep->identical = r.identical; rep->n_input = r.n_a; rep->n_archive = r.n_b;
	rep->missing = r.missing; rep->extra = r.extra; rep->differing = r.differing; rep->first_diff = r.first_diff; rep->exact_runs = r.exact_runs;
	rep->times_ms[0] = ingest; rep->times_ms[4] = now_ms() - t_begin;
	return 0;
}

// The host twin of the route above, for a machine without a GPU (`minicom -Q` without -G): the same records accepted, the same refused,
// the same first bad record named.  The file is inflated and held whole; the rules are k_fastq_quality_rows' and the file rules above.
int host_qualities(const char *path, int L, std::vector<uint8_t> &rows, size_t &n, char *err, size_t err_cap)
{
	if (L < 1 || L > 256) return fail(err, err_cap, "reads of %llu characters (1 .. 256)", (unsigned long long)L);
	gzFile f = gzopen(path, "rb");
	if (!f) return fail(err, err_cap, "cannot open the file");
	std::vector<uint8_t> text;
	{
		std::vector<uint8_t> buf((size_t)1 << 20);
		int got;
		while ((got = gzread(f, buf.data(), (unsigned)buf.size())) > 0) text.insert(text.end(), buf.begin(), buf.begin() + got);
		gzclose(f);
		if (got < 0) return fail(err, err_cap, "cannot read the file (a damaged gzip stream?)");
	}
	if (!text.empty() && text.back() != '\n') text.push_back('\n');         // a missing last newline is accepted
	rows.clear(); n = 0;
	size_t at = 0, start[5];
	while (at < text.size()) {
		start[0] = at;
		for (int q = 1; q <= 4; ++q) {
			const uint8_t *nl = at < text.size() ? (const uint8_t*)memchr(text.data() + at, '\n', text.size() - at) : nullptr;
			if (!nl) return fail(err, err_cap, "the file ends inside record %llu", (unsigned long long)(n + 1));
			at = (size_t)(nl - text.data()) + 1; start[q] = at;
		}
		if (n + 1 >= ((size_t)1 << 32)) return fail(err, err_cap, "more than 2^32 records");
		const size_t a = start[0], b = start[1], c = start[2], d = start[3], e = start[4];
		uint32_t bad = 0;
		if (b - 1 - a < 1 || text[a] != '@') bad |= MCOM_FASTQ_F_NAME;
		if (d - 1 - c < 1 || text[c] != '+') bad |= MCOM_FASTQ_F_PLUS;
		if (c - 1 - b != (size_t)L || e - 1 - d != (size_t)L) bad |= MCOM_FASTQ_F_LENGTH;
		if (!bad) for (int j = 0; j < L; ++j) if (text[d + j] < 33 || text[d + j] > 126) bad |= MCOM_FASTQ_F_CHAR;
		if (bad) { record_message(err, err_cap, (unsigned long long)n + 1, L, bad); return -1; }
		rows.insert(rows.end(), text.begin() + d, text.begin() + d + L);
		++n;
	}
	return 0;
}

// ---- file forms (bin/mcomz e --qual L, d): a file of n * L raw quality bytes <-> a `.mcq` member; device -1 = the host twin ----------
bool slurp_file(const char *path, std::vector<uint8_t> &out)
{
	FILE *f = fopen(path, "rb");
	if (!f) return false;
	uint8_t buf[65536]; size_t got;
	while ((got = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + got);
	const bool ok = !ferror(f);
	fclose(f);
	return ok;
}
bool write_file(const char *path, const uint8_t *p, size_t n)
{
	FILE *f = fopen(path, "wb");
	if (!f) return false;
	const bool ok = !n || fwrite(p, 1, n, f) == n;
	if (fclose(f) || !ok) { remove(path); return false; }
	return true;
}
struct DevBuf { mcom_ctx *ctx = nullptr; uint8_t *a = nullptr, *b = nullptr; ~DevBuf() { if (ctx) (void)mcom_sync(ctx); if (a) (void)hipFree(a); if (b) (void)hipFree(b); if (ctx) mcom_destroy(ctx); } };
bool open_device(DevBuf &D, int device, size_t bytes_a, size_t bytes_b)
{
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev || hipSetDevice(device) != hipSuccess) return false;   // no such GPU: an error, never the host twin
	if (mcom_create(&D.ctx, device, nullptr) != MCOM_OK) { D.ctx = nullptr; return false; }
	return hipMalloc((void**)&D.a, bytes_a + 16) == hipSuccess && hipMalloc((void**)&D.b, bytes_b + 16) == hipSuccess;
}

int qual_file(const char *in_path, const char *out_path, int L, int device, bool pack, const mcomh_qual_lossy_spec *spec = nullptr, mcomh_qual_lossy_report *rep = nullptr)
{
	if (!in_path || !out_path) return -1;
	std::vector<uint8_t> in, out;
	if (!slurp_file(in_path, in)) return -1;
	if (pack) {
		if (L < 1 || L > 256 || in.size() % (size_t)L) { fprintf(stderr, "mcomz: %zu bytes are not rows of %d\n", in.size(), L); return -1; }
		const uint64_t n = in.size() / (size_t)L, cap = mcomh_qual_bound(n, (uint32_t)L);
		uint64_t len = 0;
		out.resize(cap);
		if (spec && !spec_ok(spec)) { fprintf(stderr, "mcomz: not a lossy spec the transform takes\n"); return -1; }
		if (device < 0) {
			if (spec && mcomh_qual_transform(in.data(), n, (uint32_t)L, (uint64_t)L, spec, rep)) return -1;
			if (mcomh_qual_encode(in.data(), n, (uint32_t)L, (uint64_t)L, out.data(), cap, &len, 0)) return -1;
		} else {
			DevBuf D;
			if (!open_device(D, device, in.size(), cap)) return -1;
			if (hipMemcpy(D.a, in.data(), in.size(), hipMemcpyHostToDevice) != hipSuccess) return -1;
			if (spec && mcom_qual_transform(D.ctx, D.a, n, (uint32_t)L, (uint64_t)L, (const mcom_qual_lossy_spec*)spec, (mcom_qual_lossy_report*)rep)) { fprintf(stderr, "mcomz: %s\n", mcom_last_error(D.ctx)); return -1; }
			if (mcom_qual_encode(D.ctx, D.a, n, (uint32_t)L, (uint64_t)L, D.b, cap, &len, 0)) { fprintf(stderr, "mcomz: %s\n", mcom_last_error(D.ctx)); return -1; }
			if (hipMemcpy(out.data(), D.b, len, hipMemcpyDeviceToHost) != hipSuccess) return -1;
		}
		return write_file(out_path, out.data(), len) ? 0 : -1;
	}
	uint64_t n = 0, gn = 0; uint32_t qL = 0, gL = 0;
	if (mcomh_qual_info(in.data(), in.size(), &n, &qL)) return -1;
	out.resize(n * qL + 1);
	if (device < 0) { if (mcomh_qual_decode(in.data(), in.size(), out.data(), qL, n, &gn, &gL)) return -1; }
	else {
		DevBuf D;
		if (!open_device(D, device, in.size(), n * qL)) return -1;
		if (hipMemcpy(D.a, in.data(), in.size(), hipMemcpyHostToDevice) != hipSuccess) return -1;
		if (mcom_qual_decode(D.ctx, D.a, in.size(), D.b, qL, n, &gn, &gL)) { fprintf(stderr, "mcomz: %s\n", mcom_last_error(D.ctx)); return -1; }
		if (n * qL && hipMemcpy(out.data(), D.b, n * qL, hipMemcpyDeviceToHost) != hipSuccess) return -1;
	}
	return write_file(out_path, out.data(), n * qL) ? 0 : -1;
}

// `minicom -a Q[:C]`: the agreement transform between the gather of the rows and the -b transform.  The mask file
// (mcomh_agree_mask) must hold rows first_row .. first_row + n - 1 of (L + 7) / 8 bytes each.
struct AgreeArgs { const char *mask_path; uint64_t first_row; uint32_t Q; mcomh_qual_agree_report *rep; };
int load_mask(const AgreeArgs &ag, size_t n, int L, std::vector<uint8_t> &mask, char *err, size_t err_cap)
{
	if (!ag.mask_path || ag.Q > 93) return fail(err, err_cap, "agree: a mask file and a Phred value 0 .. 93");
	if (!slurp_file(ag.mask_path, mask)) return fail(err, err_cap, "cannot read the mask file");
	const size_t mb = (size_t)(L + 7) / 8;
	if (mask.size() % mb || mask.size() / mb < ag.first_row || mask.size() / mb - ag.first_row < n)
		return fail(err, err_cap, "the mask file holds %llu bytes: not the rows [first, first + %llu) of this read length", (unsigned long long)mask.size(), (unsigned long long)n);
	return 0;
}
int agree_host(const AgreeArgs &ag, uint8_t *rows, size_t n, int L, char *err, size_t err_cap)
{
	std::vector<uint8_t> mask;
	if (load_mask(ag, n, L, mask, err, err_cap)) return -1;
	if (mcomh_qual_agree(rows, n, (uint32_t)L, (uint64_t)L, mask.data(), (uint64_t)((L + 7) / 8), ag.first_row, ag.Q, ag.rep)) return fail(err, err_cap, "the agreement transform failed");
	return 0;
}
int agree_device(const AgreeArgs &ag, mcom_ctx *ctx, uint8_t *d_rows, size_t n, int L, char *err, size_t err_cap)
{
	std::vector<uint8_t> mask;
	if (load_mask(ag, n, L, mask, err, err_cap)) return -1;
	const size_t mb = (size_t)(L + 7) / 8;
	struct Dev { uint8_t *d = nullptr; ~Dev() { if (d) (void)hipFree(d); } } M;
	if (hipMalloc((void**)&M.d, n * mb + 16) != hipSuccess) return fail(err, err_cap, "no room on the card for the mask");
	if (n && hipMemcpy(M.d, mask.data() + (size_t)ag.first_row * mb, n * mb, hipMemcpyHostToDevice) != hipSuccess) return fail(err, err_cap, "upload failed");
	if (mcom_qual_agree(ctx, d_rows, n, (uint32_t)L, (uint64_t)L, M.d, mb, 0, ag.Q, (mcom_qual_agree_report*)ag.rep)) { if (err && err_cap) snprintf(err, err_cap, "%s", mcom_last_error(ctx)); return -1; }
	return 0;
}

// FASTQ file -> `.mcq` member file (bin/mcomz e --fastq-qual L): on GPU `device` the quality lines are gathered by
// mcomh_fastq_qualities_to_device and coded by mcom_qual_encode; device -1 is the host twin of both.  The same bytes either way.
int fastq_member(const char *fastq, int L, int device, const char *out_path, uint64_t *n_out, char *err, size_t err_cap, const mcomh_qual_lossy_spec *spec = nullptr, mcomh_qual_lossy_report *rep = nullptr,
                 const AgreeArgs *agree = nullptr)
{
	if (!fastq || !out_path) return fail(err, err_cap, "null pointer");
	if (spec && !spec_ok(spec)) return fail(err, err_cap, "not a lossy spec the transform takes");
	std::vector<uint8_t> out;
	uint64_t len = 0; size_t n = 0;
	if (device < 0) {
		std::vector<uint8_t> rows;
		if (host_qualities(fastq, L, rows, n, err, err_cap)) return -1;
		if (agree && agree_host(*agree, rows.data(), n, L, err, err_cap)) return -1;
		if (spec && mcomh_qual_transform(rows.data(), n, (uint32_t)L, (uint64_t)L, spec, rep)) return fail(err, err_cap, "the lossy transform failed");
		out.resize(mcomh_qual_bound(n, (uint32_t)L));
		if (mcomh_qual_encode(rows.data(), n, (uint32_t)L, (uint64_t)L, out.data(), out.size(), &len, 0)) return fail(err, err_cap, "the quality coder failed");
	} else {
		struct Rows { uint8_t *d = nullptr; ~Rows() { mcomh_device_free(d); } } in;
		if (qualities(fastq, device, L, 0, &in.d, &n, err, err_cap)) return -1;
		const uint64_t cap = mcomh_qual_bound(n, (uint32_t)L);
		struct Dev { mcom_ctx *ctx = nullptr; uint8_t *d_out = nullptr; ~Dev() { if (ctx) (void)mcom_sync(ctx); if (d_out) (void)hipFree(d_out); if (ctx) mcom_destroy(ctx); } } D;
		if (mcom_create(&D.ctx, device, nullptr) != MCOM_OK) { D.ctx = nullptr; return fail(err, err_cap, "cannot create a context on the GPU"); }
		if (hipMalloc((void**)&D.d_out, cap + 16) != hipSuccess) return fail(err, err_cap, "no room on the card");
		if (agree && agree_device(*agree, D.ctx, in.d, n, L, err, err_cap)) return -1;
		if (spec && mcom_qual_transform(D.ctx, in.d, n, (uint32_t)L, (uint64_t)L, (const mcom_qual_lossy_spec*)spec, (mcom_qual_lossy_report*)rep)) { if (err && err_cap) snprintf(err, err_cap, "%s", mcom_last_error(D.ctx)); return -1; }
		if (mcom_qual_encode(D.ctx, in.d, n, (uint32_t)L, (uint64_t)L, D.d_out, cap, &len, 0)) { if (err && err_cap) snprintf(err, err_cap, "%s", mcom_last_error(D.ctx)); return -1; }
		out.resize(len);
		if (len && hipMemcpy(out.data(), D.d_out, len, hipMemcpyDeviceToHost) != hipSuccess) return fail(err, err_cap, "download failed");
	}
	if (!write_file(out_path, out.data(), len)) return fail(err, err_cap, "cannot write the member");
	if (n_out) *n_out = n;
	return 0;
}

// The same with the rows put into an archive's own order first (bin/mcomz e --fastq-qual L --order FILE; `minicom -q`, DESIGN.md section
// 3.11): FILE is read_order.bin, one little-endian u32 per row of the member -- row j of the member is record order[j] of the FASTQ file.
// The ingest and its per-record checks are those above; then mcom_qual_gather_rows (host: its twin), which is also the check that the
// order is a permutation of the records; then the coder.  No member is written when the order's size is no multiple of 4, its entry
// count differs from the record count, or a flag is raised.  On the GPU the matrix is held twice: refused when the card has no room.
int fastq_member_ordered(const char *fastq, int L, int device, const char *order_path, const char *out_path, uint64_t *n_out, char *err, size_t err_cap, const mcomh_qual_lossy_spec *spec = nullptr,
                         mcomh_qual_lossy_report *rep = nullptr, const AgreeArgs *agree = nullptr)
{
	if (!fastq || !out_path || !order_path) return fail(err, err_cap, "null pointer");
	if (spec && !spec_ok(spec)) return fail(err, err_cap, "not a lossy spec the transform takes");
	std::vector<uint8_t> ob;
	if (!slurp_file(order_path, ob)) return fail(err, err_cap, "cannot read the order file");
	if (ob.size() % 4) return fail(err, err_cap, "the order file holds %llu bytes: not a multiple of 4", (unsigned long long)ob.size());
	const uint64_t n_order = ob.size() / 4;
	std::vector<uint32_t> order((size_t)n_order);
	for (uint64_t j = 0; j < n_order; ++j) order[(size_t)j] = (uint32_t)ob[4 * j] | (uint32_t)ob[4 * j + 1] << 8 | (uint32_t)ob[4 * j + 2] << 16 | (uint32_t)ob[4 * j + 3] << 24;
	std::vector<uint8_t> out;
	uint64_t len = 0; size_t n = 0;
	uint32_t flag = 0;
	auto flagged = [&]() {
		if (err && err_cap) snprintf(err, err_cap, "the order file is not a permutation of the records:%s%s", flag & MCOM_GATHER_F_BOUNDS ? " an entry beyond the last record" : "",
		                             flag & MCOM_GATHER_F_DUP ? " a record named twice" : "");
		return -1;
	};
	if (device < 0) {
		std::vector<uint8_t> rows;
		if (host_qualities(fastq, L, rows, n, err, err_cap)) return -1;
		if (n_order != n) return fail(err, err_cap, "the order file holds %llu entries, the FASTQ file %llu records", (unsigned long long)n_order, (unsigned long long)n);
		std::vector<uint8_t> sorted(rows.size() + 1);
		if (mcomh_qual_gather_rows(rows.data(), n, (uint32_t)L, (uint64_t)L, order.data(), n, sorted.data(), (uint64_t)L, &flag)) return fail(err, err_cap, "the row gather failed");
		if (flag) return flagged();
		if (agree && agree_host(*agree, sorted.data(), n, L, err, err_cap)) return -1;
		if (spec && mcomh_qual_transform(sorted.data(), n, (uint32_t)L, (uint64_t)L, spec, rep)) return fail(err, err_cap, "the lossy transform failed");
		out.resize(mcomh_qual_bound(n, (uint32_t)L));
		if (mcomh_qual_encode(sorted.data(), n, (uint32_t)L, (uint64_t)L, out.data(), out.size(), &len, 0)) return fail(err, err_cap, "the quality coder failed");
	} else {
		struct Rows { uint8_t *d = nullptr; ~Rows() { mcomh_device_free(d); } } in;
		if (qualities(fastq, device, L, 0, &in.d, &n, err, err_cap)) return -1;
		if (n_order != n) return fail(err, err_cap, "the order file holds %llu entries, the FASTQ file %llu records", (unsigned long long)n_order, (unsigned long long)n);
		const uint64_t cap = mcomh_qual_bound(n, (uint32_t)L), raw = (uint64_t)n * (uint64_t)L;
		struct Dev { mcom_ctx *ctx = nullptr; uint8_t *d_out = nullptr, *d_sorted = nullptr; uint32_t *d_order = nullptr;
		             ~Dev() { if (ctx) (void)mcom_sync(ctx); if (d_out) (void)hipFree(d_out); if (d_sorted) (void)hipFree(d_sorted); if (d_order) (void)hipFree(d_order); if (ctx) mcom_destroy(ctx); } } D;
		if (mcom_create(&D.ctx, device, nullptr) != MCOM_OK) { D.ctx = nullptr; return fail(err, err_cap, "cannot create a context on the GPU"); }
		{
			size_t fr = 0, tot = 0;
			const uint64_t need = raw + 4 * (uint64_t)n + n / 8 + cap + ((uint64_t)64 << 20);   // the second matrix, the order and its marks, the member
			if (hipMemGetInfo(&fr, &tot) != hipSuccess || need > fr)
				return fail(err, err_cap, "the card has no room to hold the quality rows twice (%llu more bytes needed, %llu free)", (unsigned long long)need, (unsigned long long)fr);
		}
		if (hipMalloc((void**)&D.d_sorted, raw + 16) != hipSuccess || hipMalloc((void**)&D.d_order, 4 * (size_t)n + 16) != hipSuccess || hipMalloc((void**)&D.d_out, cap + 16) != hipSuccess)
			return fail(err, err_cap, "no room on the card");
		uint32_t *d_flag = D.d_order + n;                                     // (the word behind the order: 16 spare bytes were taken)
		if ((n && hipMemcpy(D.d_order, order.data(), 4 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) || hipMemset(d_flag, 0, 4) != hipSuccess) return fail(err, err_cap, "upload failed");
		if (mcom_qual_gather_rows(D.ctx, in.d, n, (uint32_t)L, (uint64_t)L, D.d_order, n, D.d_sorted, (uint64_t)L, d_flag)) { if (err && err_cap) snprintf(err, err_cap, "%s", mcom_last_error(D.ctx)); return -1; }
		if (hipMemcpy(&flag, d_flag, 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(err, err_cap, "cannot read the flag word");
		if (flag) return flagged();
		if (agree && agree_device(*agree, D.ctx, D.d_sorted, n, L, err, err_cap)) return -1;
		if (spec && mcom_qual_transform(D.ctx, D.d_sorted, n, (uint32_t)L, (uint64_t)L, (const mcom_qual_lossy_spec*)spec, (mcom_qual_lossy_report*)rep)) { if (err && err_cap) snprintf(err, err_cap, "%s", mcom_last_error(D.ctx)); return -1; }
		if (mcom_qual_encode(D.ctx, D.d_sorted, n, (uint32_t)L, (uint64_t)L, D.d_out, cap, &len, 0)) { if (err && err_cap) snprintf(err, err_cap, "%s", mcom_last_error(D.ctx)); return -1; }
		out.resize(len);
		if (len && hipMemcpy(out.data(), D.d_out, len, hipMemcpyDeviceToHost) != hipSuccess) return fail(err, err_cap, "download failed");
	}
	if (!write_file(out_path, out.data(), len)) return fail(err, err_cap, "cannot write the member");
	if (n_out) *n_out = n;
	return 0;
}

}  // namespace

extern "C" int mcomh_fastq_quality_member_ordered(const char *fastq, int L, int device, const char *order_path, const char *out_path, uint64_t *n, char *err, size_t err_cap)
{
	if (err && err_cap) err[0] = 0;
	try { return fastq_member_ordered(fastq, L, device, order_path, out_path, n, err, err_cap); } catch (...) { return -1; }
}

extern "C" int mcomh_fastq_quality_member(const char *fastq, int L, int device, const char *out_path, uint64_t *n, char *err, size_t err_cap)
{
	if (err && err_cap) err[0] = 0;
	try { return fastq_member(fastq, L, device, out_path, n, err, err_cap); } catch (...) { return -1; }
}
extern "C" int mcomh_fastq_quality_member_lossy(const char *fastq, int L, int device, const char *order_path, const mcomh_qual_lossy_spec *spec, const char *out_path, uint64_t *n,
                                                mcomh_qual_lossy_report *report, char *err, size_t err_cap)
{
	if (err && err_cap) err[0] = 0;
	try {
		return order_path ? fastq_member_ordered(fastq, L, device, order_path, out_path, n, err, err_cap, spec, report) : fastq_member(fastq, L, device, out_path, n, err, err_cap, spec, report);
	} catch (...) { return -1; }
}
extern "C" int mcomh_fastq_quality_member_agree(const char *fastq, int L, int device, const char *order_path, const char *mask_path, uint64_t first_mask_row, uint32_t Q,
                                                const mcomh_qual_lossy_spec *spec, const char *out_path, uint64_t *n, mcomh_qual_agree_report *agree_report,
                                                mcomh_qual_lossy_report *report, char *err, size_t err_cap)
{
	if (err && err_cap) err[0] = 0;
	if (agree_report) memset(agree_report, 0, sizeof *agree_report);
	try {
		const AgreeArgs ag = {mask_path, first_mask_row, Q, agree_report};
		if (!mask_path || Q > 93) return fail(err, err_cap, "agree: a mask file and a Phred value 0 .. 93");
		return order_path ? fastq_member_ordered(fastq, L, device, order_path, out_path, n, err, err_cap, spec, report, &ag) : fastq_member(fastq, L, device, out_path, n, err, err_cap, spec, report, &ag);
	} catch (...) { return -1; }
}
extern "C" int mcomh_qual_pack_file_lossy(const char *in_path, const char *out_path, int L, int device, const mcomh_qual_lossy_spec *spec, mcomh_qual_lossy_report *report)
{
	try { return qual_file(in_path, out_path, L, device, true, spec, report); } catch (...) { return -1; }
}
// FOLDER/qual_lossy.txt, when there, applied to the n x L rows at d_rows (mcom_fastq.hpp)
int mcom_qual_lossy_apply_marker(const char *folder, int device, uint8_t *d_rows, size_t n, int L)
{
	mcomh_qual_lossy_spec spec;
	const int have = mcomh_qual_lossy_marker(folder, &spec, nullptr, 0);
	if (have < 0) { fprintf(stderr, "minicom verify: %s/qual_lossy.txt does not hold a lossy spec (ill8, thr:T:LO:HI, pblock:P) and a newline\n", folder); return -1; }
	if (!have) return 0;
	struct Ctx { mcom_ctx *ctx = nullptr; ~Ctx() { if (ctx) { (void)mcom_sync(ctx); mcom_destroy(ctx); } } } C;
	if (hipSetDevice(device) != hipSuccess || mcom_create(&C.ctx, device, nullptr) != MCOM_OK) { C.ctx = nullptr; fprintf(stderr, "minicom verify: cannot create a context on the GPU\n"); return -1; }
	if (mcom_qual_transform(C.ctx, d_rows, n, (uint32_t)L, (uint64_t)L, (const mcom_qual_lossy_spec*)&spec, nullptr)) { fprintf(stderr, "minicom verify: %s\n", mcom_last_error(C.ctx)); return -1; }
	return 0;
}
// FOLDER/qual_agree.txt, when there: the mask rebuilt from the folder on the device, its rows [first_mask_row, + n) applied to the rows at d_rows (mcom_fastq.hpp)
int mcom_qual_agree_apply_marker(const char *folder, int device, uint8_t *d_rows, size_t n, int L, uint64_t first_mask_row)
{
	uint32_t Q = 0, C = 0;
	const int have = mcomh_qual_agree_marker(folder, &Q, &C);
	if (have < 0) { fprintf(stderr, "minicom verify: %s/qual_agree.txt does not hold `Q C` (0 .. 93, 1 .. 255) and a newline\n", folder); return -1; }
	if (!have) return 0;
	std::vector<uint8_t> mask;
	uint64_t m_rows = 0; int m_L = 0;
	FILE *f = fopen((std::string(folder) + "/ids.bin.0").c_str(), "rb");
	if (f) fclose(f);
	if (mcom_agree_mask_gpu(folder, f != nullptr, (int)C, device, mask, &m_rows, &m_L)) { fprintf(stderr, "minicom verify: the agreement mask of %s cannot be rebuilt\n", folder); return -1; }
	if (m_L != L) { fprintf(stderr, "minicom verify: the agreement mask of %s has rows of %d columns, the quality rows %d\n", folder, m_L, L); return -1; }
	// a file of more records than the mask has rows is not refused: the rows the mask knows go through it, and the comparison reports the other count
	if (first_mask_row > m_rows) first_mask_row = m_rows;
	if (n > m_rows - first_mask_row) n = (size_t)(m_rows - first_mask_row);
	const size_t mb = (size_t)(L + 7) / 8;
	struct Dev { mcom_ctx *ctx = nullptr; uint8_t *d = nullptr; ~Dev() { if (ctx) (void)mcom_sync(ctx); if (d) (void)hipFree(d); if (ctx) mcom_destroy(ctx); } } D;
	if (hipSetDevice(device) != hipSuccess || mcom_create(&D.ctx, device, nullptr) != MCOM_OK) { D.ctx = nullptr; fprintf(stderr, "minicom verify: cannot create a context on the GPU\n"); return -1; }
	if (hipMalloc((void**)&D.d, n * mb + 16) != hipSuccess || (n && hipMemcpy(D.d, mask.data() + (size_t)first_mask_row * mb, n * mb, hipMemcpyHostToDevice) != hipSuccess)) { fprintf(stderr, "minicom verify: the card has no room for the agreement mask\n"); return -1; }
	if (mcom_qual_agree(D.ctx, d_rows, n, (uint32_t)L, (uint64_t)L, D.d, mb, 0, Q, nullptr)) { fprintf(stderr, "minicom verify: %s\n", mcom_last_error(D.ctx)); return -1; }
	return 0;
}
extern "C" int mcomh_device_copy(void *d_dst, const void *d_src, size_t bytes)
{
	if (!bytes) return 0;
	return d_dst && d_src && hipMemcpy(d_dst, d_src, bytes, hipMemcpyDeviceToDevice) == hipSuccess ? 0 : -1;
}
extern "C" int mcomh_qual_pack_file(const char *in_path, const char *out_path, int L, int device) { try { return qual_file(in_path, out_path, L, device, true); } catch (...) { return -1; } }
extern "C" int mcomh_qual_unpack_file(const char *in_path, const char *out_path, int device) { try { return qual_file(in_path, out_path, 0, device, false); } catch (...) { return -1; } }

extern "C" int mcomh_fastq_qualities_to_device(const char *path, int device, int L, size_t piece_bytes, uint8_t **d_rows, size_t *n, char *err, size_t err_cap)
{
	if (err && err_cap) err[0] = 0;
	try { return qualities(path, device, L, piece_bytes, d_rows, n, err, err_cap); } catch (...) { return -1; }
}

extern "C" int mcomh_verify_quality_member_gpu(const char *folder, const char *member, const char *fastq, int device, mcomh_verify_report *rep)
{
	if (!folder || !member || !fastq || !rep) { fprintf(stderr, "minicom verify: bad arguments (a folder with qual.mcq and one FASTQ file)\n"); return -1; }
	memset(rep, 0, sizeof(*rep));
	rep->first_diff = ~(uint64_t)0;
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) { fprintf(stderr, "minicom verify: no GPU %d (%d visible); there is no host route\n", device, n_dev); return -1; }
	try { return verify_quality(folder, member, fastq, device, rep); } catch (...) { return -1; }
}
extern "C" int mcomh_verify_quality_gpu(const char *folder, const char *fastq, int device, mcomh_verify_report *rep) { return mcomh_verify_quality_member_gpu(folder, "qual.mcq", fastq, device, rep); }
