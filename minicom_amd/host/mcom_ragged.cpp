// minicom_amd/host/mcom_ragged.cpp -- FASTQ files whose reads differ in length (`minicom -p -V`).
//
// L is the modal sequence length (ties: the larger one).  Records of that length are EVEN and go to the core and to qual.mcq as rows of
// L; the others are ODD: their lines go to odd.seq / odd.qual back to back, and len.bin (length - 1 per record) says which is which.
//   mcomh_fastq_lengths_file            one pass: every record checked, len.bin written, L found from the histogram of the lengths
//   mcomh_fastq_to_device_ragged        the even reads as [n_even][L] in HBM for mcomh_create, odd.seq written
//   mcomh_fastq_ragged_files            either kind of line as files: the even rows raw and the odd text (what the two calls around it share)
//   mcomh_fastq_quality_member_ragged   qual.mcq over the even rows by the unchanged coder, odd.qual written
//   mcomh_fastq_emit_ragged             the host twin of mcom_fastq_emit_ragged: even rows + odd texts (+ names) -> records
// On GPU `device` the text goes up in pieces (plain or gzip through zlib's reader; a BGZF file is inflated on the card, section 3.15),
// lines by mcom_decode_line_index, then the kernels of csrc/ragged.hip; device -1 is the plain C++ twin of every call: the same rules,
// the same files refused, the same first bad record named, the same bytes written.
#include "../../include/mcom_host.h"
#include "../../include/mcom.h"
#include "mcom_ragged.hpp"
#include <zlib.h>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#ifndef MCOM_ENTROPY_HOST_ONLY
#include "mcom_gzip_gpu.hpp"
#include <hip/hip_runtime.h>
#endif

namespace {

const uint64_t ODD = MCOM_RAGGED_ODD;

int fail(char *err, size_t cap, const char *fmt, unsigned long long a = 0, unsigned long long b = 0)
{
	if (err && cap) snprintf(err, cap, fmt, a, b);
	return -1;
}
int bad_record(char *err, size_t cap, unsigned long long record1)
{
	return fail(err, cap, "record %llu is not a four-line FASTQ record of 1 .. 256 bases in ACGTN and as many quality values in 33 .. 126", record1);
}
int bad_table(char *err, size_t cap, unsigned long long record1)
{
	return fail(err, cap, "record %llu is not what the length file says (its length, or the file's modal length)", record1);
}

bool slurp_file(const char *path, std::vector<uint8_t> &out)
{
	FILE *f = fopen(path, "rb");
	if (!f) return false;
	uint8_t buf[65536]; size_t got;
	out.clear();
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

inline bool base_ok(uint8_t v) { return v == 'A' || v == 'C' || v == 'G' || v == 'T' || v == 'N'; }

// the modal length of a histogram of (length - 1), ties to the larger; 0: no record
int modal_length(const uint64_t *hist)
{
	int best = -1;
	for (int b = 0; b < 256; ++b) if (hist[b] && (best < 0 || hist[b] >= hist[best])) best = b;
	return best + 1;
}

// slots of all records (the twin of mcom_ragged_index)
void host_index(const std::vector<uint8_t> &len, int L, std::vector<uint64_t> &slot, uint64_t &n_even, uint64_t &odd_bytes)
{
	slot.resize(len.size()); n_even = 0; odd_bytes = 0;
	for (size_t r = 0; r < len.size(); ++r) {
		const uint32_t l = (uint32_t)len[r] + 1;
		if ((int)l == L) slot[r] = n_even++; else { slot[r] = ODD | odd_bytes; odd_bytes += l; }
	}
}

// ---- the host twins: the file inflated and held whole, record after record ---------------------------------------------------------------
int host_text(const char *path, std::vector<uint8_t> &text, char *err, size_t err_cap)
{
	gzFile f = gzopen(path, "rb");
	if (!f) return fail(err, err_cap, "cannot open the file");
	std::vector<uint8_t> buf((size_t)1 << 20);
	int got;
	text.clear();
	while ((got = gzread(f, buf.data(), (unsigned)buf.size())) > 0) text.insert(text.end(), buf.begin(), buf.begin() + got);
	gzclose(f);
	if (got < 0) return fail(err, err_cap, "cannot read the file (a damaged gzip stream?)");
	if (!text.empty() && text.back() != '\n') text.push_back('\n');         // a missing last newline is accepted
	return 0;
}
// fn(record number, the five line starts): 0 to go on
int host_records(const std::vector<uint8_t> &text, const std::function<int(uint64_t, const size_t*)> &fn, uint64_t &n, char *err, size_t err_cap)
{
	size_t at = 0, start[5];
	n = 0;
	while (at < text.size()) {
		start[0] = at;
		for (int q = 1; q <= 4; ++q) {
			const uint8_t *nl = at < text.size() ? (const uint8_t*)memchr(text.data() + at, '\n', text.size() - at) : nullptr;
			if (!nl) return fail(err, err_cap, "the file ends inside record %llu", (unsigned long long)(n + 1));
			at = (size_t)(nl - text.data()) + 1; start[q] = at;
		}
		if (n + 1 >= ((uint64_t)1 << 32)) return fail(err, err_cap, "more than 2^32 records");
		const int rc = fn(n, start);
		if (rc) return rc;
		++n;
	}
	return 0;
}
// the checks of k_fastq_lengths; *sl = the sequence length
uint32_t host_check(const std::vector<uint8_t> &text, const size_t *s, size_t *sl)
{
	const size_t a = s[0], b = s[1], c = s[2], d = s[3], e = s[4];
	uint32_t bad = 0;
	if (b - 1 - a < 1 || text[a] != '@') bad |= MCOM_FASTQ_F_NAME;
	if (d - 1 - c < 1 || text[c] != '+') bad |= MCOM_FASTQ_F_PLUS;
	*sl = c - 1 - b;
	if (e - 1 - d != *sl || *sl < 1 || *sl > 256) return bad | MCOM_FASTQ_F_LENGTH;
	for (size_t j = 0; j < *sl; ++j) {
		if (text[d + j] < 33 || text[d + j] > 126) bad |= MCOM_FASTQ_F_CHAR;
		if (!base_ok(text[b + j])) bad |= MCOM_FASTQ_F_BASE;
	}
	return bad;
}

int host_lengths(const char *path, std::vector<uint8_t> &len, uint64_t *hist, char *err, size_t err_cap)
{
	std::vector<uint8_t> text;
	if (host_text(path, text, err, err_cap)) return -1;
	uint64_t n = 0;
	len.clear(); memset(hist, 0, 256 * 8);
	return host_records(text, [&](uint64_t r, const size_t *s) {
		size_t sl = 0;
		if (host_check(text, s, &sl)) return bad_record(err, err_cap, r + 1);
		len.push_back((uint8_t)(sl - 1)); ++hist[sl - 1];
		return 0;
	}, n, err, err_cap);
}

// line `which` of every record: the even rows back to back, the odd text; the twin of k_fastq_ragged_rows and its piece loop
int host_split(const char *path, int which, int L, const std::vector<uint8_t> &len, std::vector<uint8_t> &rows, std::vector<uint8_t> &odd, uint64_t &n_even, char *err, size_t err_cap)
{
	std::vector<uint8_t> text;
	if (host_text(path, text, err, err_cap)) return -1;
	std::vector<uint64_t> slot;
	uint64_t odd_bytes = 0, n = 0;
	host_index(len, L, slot, n_even, odd_bytes);
	rows.assign((size_t)n_even * (size_t)L, 0); odd.assign((size_t)odd_bytes, 0);
	if (host_records(text, [&](uint64_t r, const size_t *s) {
		if (r >= len.size()) return fail(err, err_cap, "the file holds more records than the length file's %llu", (unsigned long long)len.size());
		const size_t p = s[which], q = s[which + 1], want = (size_t)len[r] + 1;
		if (q - 1 - p != want) return bad_table(err, err_cap, r + 1);
		uint8_t *dst = slot[r] & ODD ? odd.data() + (slot[r] & ~ODD) : rows.data() + slot[r] * (size_t)L;
		for (size_t j = 0; j < want; ++j) {
			const uint8_t v = text[p + j];
			if (which == 1 ? !base_ok(v) : (v < 33 || v > 126)) return bad_record(err, err_cap, r + 1);
			dst[j] = v;
		}
		return 0;
	}, n, err, err_cap)) return -1;
	if (n != len.size()) return fail(err, err_cap, "the file holds %llu records, the length file %llu", (unsigned long long)n, (unsigned long long)len.size());
	return 0;
}

#ifndef MCOM_ENTROPY_HOST_ONLY
// ---- the device route: the piece loop of mcomh_fastq_qualities_to_device (mcom_qual_gpu.cpp) with the pass as a callback ---------------------
const size_t DEFAULT_PIECE = (size_t)32 << 20;
const size_t LEAST_PIECE = 4 * (2 * (size_t)256 + 64);                     // a piece holds a few records at least: the documented minimum (include/mcom_host.h)

struct Job {                                                // what one call holds, released however it ends
	mcom_ctx *ctx = nullptr; hipStream_t copy = nullptr; hipEvent_t ev[2] = {nullptr, nullptr};
	uint8_t *pin[2] = {nullptr, nullptr}, *d_text[2] = {nullptr, nullptr};
	uint64_t *d_start = nullptr; uint32_t *d_flag = nullptr;
	std::vector<void*> dev;                                 // the pass's own tables
	gzFile f = nullptr;
	bool own_ctx = true;                                    // false: the caller's context, which outlives the job
	~Job()
	{
		if (copy) (void)hipStreamSynchronize(copy);
		if (ctx) (void)mcom_sync(ctx);
		if (f) gzclose(f);
		for (int k = 0; k < 2; ++k) { if (pin[k]) (void)hipHostFree(pin[k]); if (d_text[k]) (void)hipFree(d_text[k]); if (ev[k]) (void)hipEventDestroy(ev[k]); }
		if (d_start) (void)hipFree(d_start);
		if (d_flag) (void)hipFree(d_flag);
		for (void *p : dev) if (p) (void)hipFree(p);
		if (copy) (void)hipStreamDestroy(copy);
		if (ctx && own_ctx) mcom_destroy(ctx);
	}
	template <class T> T *alloc(size_t n) { void *p = nullptr; if (hipMalloc(&p, (n ? n : 1) * sizeof(T) + 16) != hipSuccess) return nullptr; dev.push_back(p); return (T*)p; }
	void release(void *p) { for (void *&q : dev) if (q == p) { (void)hipFree(q); q = nullptr; } }
	void disown(void *p) { for (void *&q : dev) if (q == p) q = nullptr; }
};

int open_job(Job &J, const char *path, int device, char *err, size_t err_cap, mcom_ctx *ctx = nullptr)
{
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return fail(err, err_cap, "no GPU %llu (%llu visible)", (unsigned long long)device, (unsigned long long)n_dev);
	if (hipSetDevice(device) != hipSuccess) return fail(err, err_cap, "cannot select the GPU");
	J.f = gzopen(path, "rb");
	if (!J.f) return fail(err, err_cap, "cannot open the file");
	if (ctx) { J.ctx = ctx; J.own_ctx = false; }
	else if (mcom_create(&J.ctx, device, nullptr) != MCOM_OK) { J.ctx = nullptr; return fail(err, err_cap, "cannot create a context on the GPU"); }
	if (hipStreamCreate(&J.copy) != hipSuccess) return fail(err, err_cap, "no stream");
	if (hipMalloc((void**)&J.d_flag, 16) != hipSuccess) return fail(err, err_cap, "no room on the card");
	return 0;
}

// One piece on the card: `records` whole records from record `first` of the file, their text and line index.  0: go on; -1 with *err set: the
// file is refused.  The flag words are cleared in front of the line index; the pass reads them back (flagged(): the index's word counts too).
typedef std::function<int(const uint8_t *d_text, uint64_t bytes, uint64_t records, const uint64_t *d_line_start, uint64_t first)> PieceFn;

// 0: no record of the piece was flagged; 1: *record = the first flagged one; -1: the copy failed
int flagged(Job &J, uint32_t *record, uint32_t *bits = nullptr)
{
	uint32_t fl[4];
	if (hipMemcpy(fl, J.d_flag, 16, hipMemcpyDeviceToHost) != hipSuccess) return -1;
	*record = fl[1];
	if (bits) *bits = fl[0];
	return fl[0] || fl[2] ? 1 : 0;
}
bool clear_flags(Job &J)
{
	const uint32_t init[4] = {0, 0xFFFFFFFFu, 0, 0};
	return hipMemcpy(J.d_flag, init, 16, hipMemcpyHostToDevice) == hipSuccess;
}

// every record of the file through `pass`, *n = their number.  again(): the pass forgets what it has seen (the BGZF route gave the file up
// and zlib's reader starts it again).  lpr: the lines of a record, 4, or 1 for a file of one read per line (which
// always goes through zlib's reader: the BGZF route hands four-line records on)
int for_each_piece(Job &J, const char *path, size_t piece_bytes, const PieceFn &pass, const std::function<bool()> &again, uint64_t *n_out, char *err, size_t err_cap, size_t lpr = 4)
{
	size_t piece = piece_bytes ? piece_bytes : DEFAULT_PIECE;
	if (piece < LEAST_PIECE) piece = LEAST_PIECE;
	uint64_t n = 0;
	const bool on_device = lpr == 4 && mcom_gz_device_route(path, J.ctx, piece, [&](const uint8_t *d_text, uint64_t bytes, uint64_t records, const uint64_t *d_line_start) {
		if (n + records >= ((uint64_t)1 << 32) || !clear_flags(J) || pass(d_text, bytes, records, d_line_start, n)) return false;
		n += records;
		return true;
	});
	if (on_device) { *n_out = n; return 0; }
	n = 0;
	if (!again()) return fail(err, err_cap, "no room on the card");
	for (int k = 0; k < 2; ++k)
		if (hipHostMalloc((void**)&J.pin[k], piece + 1, hipHostMallocDefault) != hipSuccess || hipMalloc((void**)&J.d_text[k], piece + 16) != hipSuccess ||
		    hipEventCreateWithFlags(&J.ev[k], hipEventDisableTiming) != hipSuccess) return fail(err, err_cap, "no room for the pieces");
	// fill: `have` carried bytes are in front already; eof when the file ended (a missing last newline is added)
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
	auto whole_records = [&](const uint8_t *buf, size_t len, size_t &bytes, size_t &records) {
		size_t lines = 0; bytes = 0; records = 0;
		const uint8_t *p = buf, *const e = buf + len;
		while (p < e) { const uint8_t *q = (const uint8_t*)memchr(p, '\n', (size_t)(e - p)); if (!q) break; p = q + 1; if (++lines % lpr == 0) { bytes = (size_t)(p - buf); records = lines / lpr; } }
	};
	size_t len = 0, cap_lines = 0; bool eof = false;
	if (!fill(J.pin[0], 0, len, eof)) return fail(err, err_cap, "cannot read the file (a damaged gzip stream?)");
	for (int k = 0; ; k ^= 1) {
		size_t bytes, records;
		whole_records(J.pin[k], len, bytes, records);
		if (!eof && !records) return fail(err, err_cap, "record %llu is longer than a piece of %llu bytes", (unsigned long long)(n + 1), (unsigned long long)piece);
		if (n + records >= ((uint64_t)1 << 32)) return fail(err, err_cap, "more than 2^32 records");
		if (bytes && (hipMemcpyAsync(J.d_text[k], J.pin[k], bytes, hipMemcpyHostToDevice, J.copy) != hipSuccess || hipEventRecord(J.ev[k], J.copy) != hipSuccess)) return fail(err, err_cap, "upload failed");
		// the next piece is read while this one travels: its front is this piece's unfinished record
		size_t next_len = 0; bool next_eof = true;
		if (!eof) {
			memcpy(J.pin[k ^ 1], J.pin[k] + bytes, len - bytes);
			if (!fill(J.pin[k ^ 1], len - bytes, next_len, next_eof)) return fail(err, err_cap, "cannot read the file (a damaged gzip stream?)");
		}
		if (records) {
			if (hipEventSynchronize(J.ev[k]) != hipSuccess) return fail(err, err_cap, "upload failed");
			if (lpr * records + 1 > cap_lines) {
				if (J.d_start) (void)hipFree(J.d_start);
				J.d_start = nullptr; cap_lines = lpr * records + 1;
				if (hipMalloc((void**)&J.d_start, cap_lines * 8 + 16) != hipSuccess) return fail(err, err_cap, "no room on the card");
			}
			if (!clear_flags(J)) return fail(err, err_cap, "upload failed");
			uint64_t got_lines = 0;
			if (mcom_decode_line_index(J.ctx, J.d_text[k], bytes, J.d_start, lpr * records, &got_lines, J.d_flag + 2) || got_lines != lpr * records) {
				if (err && err_cap) snprintf(err, err_cap, "device call failed: %s", mcom_last_error(J.ctx));
				return -1;
			}
			if (pass(J.d_text[k], bytes, records, J.d_start, n)) return -1;
			n += records;
		}
		if (eof && bytes != len) return fail(err, err_cap, "the file ends inside record %llu", (unsigned long long)(n + 1));   // (behind the records in front of it: one of them may be the first bad one)
		if (eof) break;
		len = next_len; eof = next_eof;
	}
	*n_out = n;
	return 0;
}

int device_lengths(const char *path, int device, size_t piece_bytes, std::vector<uint8_t> &len, uint64_t *hist, char *err, size_t err_cap)
{
	Job J;
	if (open_job(J, path, device, err, err_cap)) return -1;
	uint64_t *d_hist = J.alloc<uint64_t>(256);
	uint8_t *d_len = nullptr;
	size_t cap = 0, held = 0;
	if (!d_hist || hipMemset(d_hist, 0, 256 * 8) != hipSuccess) return fail(err, err_cap, "no room on the card");
	auto room_for = [&](size_t rows) {                                     // the table grows by doubling: the number of records is not known in advance
		if (rows <= cap) return true;
		size_t want = cap ? cap : 65536;
		while (want < rows) want *= 2;
		uint8_t *p = J.alloc<uint8_t>(want);
		if (!p) return false;
		if (held && hipMemcpy(p, d_len, held, hipMemcpyDeviceToDevice) != hipSuccess) return false;
		if (d_len) J.release(d_len);
		d_len = p; cap = want;
		return true;
	};
	uint64_t n = 0;
	if (for_each_piece(J, path, piece_bytes, [&](const uint8_t *d_text, uint64_t bytes, uint64_t records, const uint64_t *d_line_start, uint64_t first) {
		uint32_t rec = 0;
		if (!room_for(first + records)) return fail(err, err_cap, "no room on the card");
		if (mcom_fastq_lengths(J.ctx, d_text, bytes, d_line_start, first, records, d_len, d_hist, J.d_flag)) { if (err && err_cap) snprintf(err, err_cap, "device call failed: %s", mcom_last_error(J.ctx)); return -1; }
		const int f = flagged(J, &rec);
		if (f < 0) return fail(err, err_cap, "cannot read the flag word");
		if (f) return bad_record(err, err_cap, (unsigned long long)rec + 1);
		held = first + records;
		return 0;
	}, [&]() { held = 0; return hipMemset(d_hist, 0, 256 * 8) == hipSuccess; }, &n, err, err_cap)) return -1;
	len.resize(n);
	if (n && hipMemcpy(len.data(), d_len, n, hipMemcpyDeviceToHost) != hipSuccess) return fail(err, err_cap, "download failed");
	if (hipMemcpy(hist, d_hist, 256 * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(err, err_cap, "download failed");
	return 0;
}

// the even rows in HBM (*d_rows_out, released with mcomh_device_free) and the odd text on the host
int device_split(const char *path, int device, int which, int L, const std::vector<uint8_t> &len, size_t piece_bytes, uint8_t **d_rows_out, std::vector<uint8_t> &odd, uint64_t &n_even,
                 char *err, size_t err_cap)
{
	Job J;
	if (open_job(J, path, device, err, err_cap)) return -1;
	const uint64_t n_total = len.size();
	if (n_total >= ((uint64_t)1 << 32)) return fail(err, err_cap, "more than 2^32 records");
	uint8_t *d_len = J.alloc<uint8_t>(n_total);
	uint64_t *d_slot = J.alloc<uint64_t>(n_total);
	if (!d_len || !d_slot || (n_total && hipMemcpy(d_len, len.data(), n_total, hipMemcpyHostToDevice) != hipSuccess)) return fail(err, err_cap, "no room on the card");
	uint64_t n_odd = 0, odd_bytes = 0, n = 0;
	if (mcom_ragged_index(J.ctx, d_len, n_total, (uint32_t)L, d_slot, &n_even, &n_odd, &odd_bytes)) { if (err && err_cap) snprintf(err, err_cap, "device call failed: %s", mcom_last_error(J.ctx)); return -1; }
	uint8_t *d_rows = J.alloc<uint8_t>((size_t)n_even * (size_t)L), *d_odd = J.alloc<uint8_t>((size_t)odd_bytes);
	if (!d_rows || !d_odd) return fail(err, err_cap, "no room on the card for %llu rows", (unsigned long long)n_even);
	if (for_each_piece(J, path, piece_bytes, [&](const uint8_t *d_text, uint64_t bytes, uint64_t records, const uint64_t *d_line_start, uint64_t first) {
		uint32_t rec = 0, bits = 0;
		if (first + records > n_total) return fail(err, err_cap, "the file holds more records than the length file's %llu", (unsigned long long)n_total);
		if (mcom_fastq_ragged_rows(J.ctx, d_text, bytes, d_line_start, first, records, which, (uint32_t)L, d_len, d_slot, n_total, d_rows, (uint64_t)L, n_even, d_odd, odd_bytes, J.d_flag)) {
			if (err && err_cap) snprintf(err, err_cap, "device call failed: %s", mcom_last_error(J.ctx));
			return -1;
		}
		const int f = flagged(J, &rec, &bits);
		if (f < 0) return fail(err, err_cap, "cannot read the flag word");
		if (f) return bits & MCOM_FASTQ_F_LENGTH ? bad_table(err, err_cap, (unsigned long long)rec + 1) : bad_record(err, err_cap, (unsigned long long)rec + 1);
		return 0;
	}, []() { return true; }, &n, err, err_cap)) return -1;
	if (n != n_total) return fail(err, err_cap, "the file holds %llu records, the length file %llu", (unsigned long long)n, (unsigned long long)n_total);
	odd.resize((size_t)odd_bytes);
	if (odd_bytes && hipMemcpy(odd.data(), d_odd, (size_t)odd_bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(err, err_cap, "download failed");
	J.disown(d_rows);
	*d_rows_out = d_rows;
	return 0;
}
#endif  // MCOM_ENTROPY_HOST_ONLY

int load_lengths(const char *len_path, int L, std::vector<uint8_t> &len, char *err, size_t err_cap)
{
	if (L < 1 || L > 256) return fail(err, err_cap, "reads of %llu characters (1 .. 256)", (unsigned long long)L);
	if (!len_path || !slurp_file(len_path, len)) return fail(err, err_cap, "cannot read the length file");
	return 0;
}

}  // namespace

extern "C" int mcomh_fastq_lengths_file(const char *fastq, int device, size_t piece_bytes, const char *out_path, uint64_t *n, int *L, uint64_t *n_odd, char *err, size_t err_cap)
{
	if (!fastq || !out_path || !n || !L || !n_odd) return fail(err, err_cap, "null pointer");
	*n = 0; *L = 0; *n_odd = 0;
	try {
		std::vector<uint8_t> len;
		uint64_t hist[256];
		if (device < 0) { if (host_lengths(fastq, len, hist, err, err_cap)) return -1; }
		else {
#ifndef MCOM_ENTROPY_HOST_ONLY
			if (device_lengths(fastq, device, piece_bytes, len, hist, err, err_cap)) return -1;
#else
			return fail(err, err_cap, "built without the device route");
#endif
		}
		if (len.empty()) return fail(err, err_cap, "the file holds no record");
		*L = modal_length(hist);
		*n = len.size(); *n_odd = len.size() - hist[*L - 1];
		if (!write_file(out_path, len.data(), len.size())) return fail(err, err_cap, "cannot write the length file");
		return 0;
	} catch (...) { return fail(err, err_cap, "out of memory"); }
}

extern "C" int mcomh_fastq_ragged_files(const char *fastq, int which, int L, int device, const char *len_path, size_t piece_bytes, const char *out_rows, const char *out_odd,
                                        uint64_t *n_even, char *err, size_t err_cap)
{
	if (!fastq || !out_rows || !out_odd || !n_even || (which != 1 && which != 3)) return fail(err, err_cap, "null pointer, or a line that is neither 1 (sequence) nor 3 (quality)");
	*n_even = 0;
	try {
		std::vector<uint8_t> len, rows, odd;
		if (load_lengths(len_path, L, len, err, err_cap)) return -1;
		if (device < 0) { if (host_split(fastq, which, L, len, rows, odd, *n_even, err, err_cap)) return -1; }
		else {
#ifndef MCOM_ENTROPY_HOST_ONLY
			struct Rows { uint8_t *d = nullptr; ~Rows() { mcomh_device_free(d); } } R;
			if (device_split(fastq, device, which, L, len, piece_bytes, &R.d, odd, *n_even, err, err_cap)) return -1;
			rows.resize((size_t)*n_even * (size_t)L);
			if (!rows.empty() && hipMemcpy(rows.data(), R.d, rows.size(), hipMemcpyDeviceToHost) != hipSuccess) return fail(err, err_cap, "download failed");
#else
			return fail(err, err_cap, "built without the device route");
#endif
		}
		if (!write_file(out_rows, rows.data(), rows.size())) return fail(err, err_cap, "cannot write the rows");
		if (!write_file(out_odd, odd.data(), odd.size())) { remove(out_rows); return fail(err, err_cap, "cannot write the odd text"); }
		return 0;
	} catch (...) { return fail(err, err_cap, "out of memory"); }
}

#ifndef MCOM_ENTROPY_HOST_ONLY
int mcom_fastq_for_each_piece(const char *path, mcom_ctx *ctx, int device, int lines_per_record, size_t piece_bytes, const McomPiecePass &pass, const std::function<bool()> &again,
                              uint64_t *n, char *err, size_t err_cap)
{
	Job J;
	if (open_job(J, path, device, err, err_cap, ctx)) return -1;
	return for_each_piece(J, path, piece_bytes, [&](const uint8_t *d_text, uint64_t bytes, uint64_t records, const uint64_t *d_line_start, uint64_t first) {
		return pass(d_text, bytes, records, d_line_start, first, J.d_flag);
	}, again, n, err, err_cap, lines_per_record == 1 ? 1 : 4);
}

int mcom_ragged_split_to_device(const char *path, int device, int which, int L, const char *len_path, uint8_t **d_rows, std::vector<uint8_t> &odd, uint64_t *n_even, char *err, size_t err_cap)
{
	std::vector<uint8_t> len;
	*d_rows = nullptr; *n_even = 0;
	if (load_lengths(len_path, L, len, err, err_cap)) return -1;
	return device_split(path, device, which, L, len, 0, d_rows, odd, *n_even, err, err_cap);
}

extern "C" int mcomh_fastq_to_device_ragged(const char *path, int device, int L, const char *len_path, size_t piece_bytes, uint8_t **d_reads, size_t *n_even, const char *odd_seq_path,
                                            char *err, size_t err_cap)
{
	if (!path || !d_reads || !n_even || !odd_seq_path) return fail(err, err_cap, "null pointer");
	*d_reads = nullptr; *n_even = 0;
	try {
		std::vector<uint8_t> len, odd;
		uint64_t ne = 0;
		if (load_lengths(len_path, L, len, err, err_cap)) return -1;
		if (device_split(path, device, 1, L, len, piece_bytes, d_reads, odd, ne, err, err_cap)) return -1;
		if (!write_file(odd_seq_path, odd.data(), odd.size())) { mcomh_device_free(*d_reads); *d_reads = nullptr; return fail(err, err_cap, "cannot write the odd text"); }
		*n_even = (size_t)ne;
		return 0;
	} catch (...) { return fail(err, err_cap, "out of memory"); }
}
#endif

extern "C" int mcomh_fastq_quality_member_ragged(const char *fastq, int L, int device, const char *len_path, const char *out_mcq, const char *out_odd_qual, uint64_t *n_even, char *err,
                                                 size_t err_cap)
{
	if (!fastq || !out_mcq || !out_odd_qual || !n_even) return fail(err, err_cap, "null pointer");
	*n_even = 0;
	try {
		std::vector<uint8_t> len, rows, odd, out;
		uint64_t out_len = 0;
		if (load_lengths(len_path, L, len, err, err_cap)) return -1;
		if (device < 0) {
			if (host_split(fastq, 3, L, len, rows, odd, *n_even, err, err_cap)) return -1;
			out.resize(mcomh_qual_bound(*n_even, (uint32_t)L));
			if (mcomh_qual_encode(rows.data(), *n_even, (uint32_t)L, (uint64_t)L, out.data(), out.size(), &out_len, 0)) return fail(err, err_cap, "the quality coder failed");
		} else {
#ifndef MCOM_ENTROPY_HOST_ONLY
			struct Rows { uint8_t *d = nullptr; ~Rows() { mcomh_device_free(d); } } R;
			if (device_split(fastq, device, 3, L, len, 0, &R.d, odd, *n_even, err, err_cap)) return -1;
			const uint64_t cap = mcomh_qual_bound(*n_even, (uint32_t)L);
			struct Dev { mcom_ctx *ctx = nullptr; uint8_t *d_out = nullptr; ~Dev() { if (ctx) (void)mcom_sync(ctx); if (d_out) (void)hipFree(d_out); if (ctx) mcom_destroy(ctx); } } D;
			if (mcom_create(&D.ctx, device, nullptr) != MCOM_OK) { D.ctx = nullptr; return fail(err, err_cap, "cannot create a context on the GPU"); }
			if (hipMalloc((void**)&D.d_out, cap + 16) != hipSuccess) return fail(err, err_cap, "no room on the card");
			if (mcom_qual_encode(D.ctx, R.d, *n_even, (uint32_t)L, (uint64_t)L, D.d_out, cap, &out_len, 0)) { if (err && err_cap) snprintf(err, err_cap, "%s", mcom_last_error(D.ctx)); return -1; }
			out.resize(out_len);
			if (out_len && hipMemcpy(out.data(), D.d_out, out_len, hipMemcpyDeviceToHost) != hipSuccess) return fail(err, err_cap, "download failed");
#else
			return fail(err, err_cap, "built without the device route");
#endif
		}
		if (!write_file(out_mcq, out.data(), out_len)) return fail(err, err_cap, "cannot write the member");
		if (!write_file(out_odd_qual, odd.data(), odd.size())) { remove(out_mcq); return fail(err, err_cap, "cannot write the odd text"); }
		return 0;
	} catch (...) { return fail(err, err_cap, "out of memory"); }
}

// ---- even rows + odd texts (+ names) -> records: the twin of mcom_fastq_emit_ragged, every pointer in host memory ---------------------------
extern "C" int mcomh_fastq_emit_ragged(const mcomh_ragged_src *src, uint64_t first, uint64_t count, uint8_t *out, uint64_t cap, uint64_t *bytes)
{
	if (!src || !bytes) return -1;
	*bytes = 0;
	mcom_ragged_src S;                                                      // (the same fields under the device call's names)
	S.d_reads = src->reads; S.read_pitch = src->read_pitch; S.d_quals = src->quals; S.qual_pitch = src->qual_pitch; S.n_even = src->n_even;
	S.d_odd_seq = src->odd_seq; S.d_odd_qual = src->odd_qual; S.odd_bytes = src->odd_bytes; S.d_slot = src->slot; S.d_len = src->len; S.n = src->n;
	S.d_names = src->names; S.names_bytes = src->names_bytes; S.d_rec_off = src->rec_off; S.L = src->L;
	if (S.L < 1 || S.L > 256 || S.n >= ((uint64_t)1 << 32) || first > S.n || count > S.n - first || (S.n_even && S.read_pitch < S.L) || (S.d_quals && S.qual_pitch < S.L)) return -1;
	if (!count) return 0;
	if (!S.d_len || !S.d_slot || (S.n_even && !S.d_reads) || (S.odd_bytes && (!S.d_odd_seq || (S.d_quals && !S.d_odd_qual))) || (S.d_names && !S.d_rec_off)) return -1;
	uint64_t total = 0;
	for (int round = 0; round < 2; ++round) {                               // the sizes and every check first, then the bytes
		uint8_t *o = out;
		for (uint64_t i = first; i < first + count; ++i) {
			const uint32_t l = (uint32_t)S.d_len[i] + 1;
			const uint64_t s = S.d_slot[i], at = s & ~ODD;
			const bool is_odd = (s & ODD) != 0;
			if (is_odd == (l == S.L) || (is_odd ? (at > S.odd_bytes || l > S.odd_bytes - at) : at >= S.n_even)) return -1;
			const uint8_t *rd = is_odd ? S.d_odd_seq + at : S.d_reads + at * S.read_pitch;
			if (!S.d_quals) {
				if (round) { memcpy(o, rd, l); o[l] = '\n'; o += l + 1; } else total += (uint64_t)l + 1;
				continue;
			}
			const uint8_t *ql = is_odd ? S.d_odd_qual + at : S.d_quals + at * S.qual_pitch;
			char digits[24];
			const uint8_t *name = (const uint8_t*)digits, *plus = name;
			uint64_t nl, pl = 0;
			if (S.d_names) {
				const uint64_t a = S.d_rec_off[i], e = S.d_rec_off[i + 1];
				if (e < a + 2 || e - a > 2 * (uint64_t)255 + 2 || e > S.names_bytes) return -1;
				const uint8_t *mid = (const uint8_t*)memchr(S.d_names + a, '\n', (size_t)(e - 1 - a));
				if (!mid || S.d_names[e - 1] != '\n') return -1;
				name = S.d_names + a; nl = (uint64_t)(mid - name); plus = mid + 1; pl = e - 1 - a - nl - 1;
			} else nl = (uint64_t)snprintf(digits, sizeof digits, "%llu", (unsigned long long)(i + 1));
			if (!round) { total += 2 * (uint64_t)l + 6 + nl + pl; continue; }
			*o++ = '@'; memcpy(o, name, nl); o += nl; *o++ = '\n';
			memcpy(o, rd, l); o += l; *o++ = '\n';
			*o++ = '+'; memcpy(o, plus, pl); o += pl; *o++ = '\n';
			memcpy(o, ql, l); o += l; *o++ = '\n';
		}
		if (!round) {
			*bytes = total;
			if (!out) return 0;
			if (total > cap) return -2;
		}
	}
	return 0;
}

// ---- what the decoders share -------------------------------------------------------------------------------------------------------------------
bool mcom_ragged_present(const char *folder)
{
	FILE *f = fopen((std::string(folder) + "/len.bin").c_str(), "rb");
	if (!f) return false;
	fclose(f);
	return true;
}

bool mcom_ragged_load(const char *folder, int L, uint64_t n_even, bool want_qual, McomRaggedParts &P, std::string &why, bool rebuild_odd)
{
	const std::string dir(folder);
	if (L < 1 || L > 256) { why = "reads of a length outside 1 .. 256"; return false; }
	if (!slurp_file((dir + "/len.bin").c_str(), P.len)) { why = "cannot read len.bin"; return false; }
	if (P.len.size() >= ((uint64_t)1 << 32)) { why = "len.bin holds 2^32 records or more"; return false; }
	// `minicom -V -A`: odd.aln codes some of the odd reads against the contigs and odd.seq holds the others; the full
	// odd text is rebuilt here, before anything else looks at it
	const bool aligned = mcom_odd_align_present(folder);
	if (aligned && !rebuild_odd) { P.odd_seq.clear(); (void)slurp_file((dir + "/odd.seq").c_str(), P.odd_seq); }
	else if (aligned) { if (!mcom_odd_align_rebuild(folder, L, P, why)) return false; }
	else if (!slurp_file((dir + "/odd.seq").c_str(), P.odd_seq)) { why = "len.bin without odd.seq"; return false; }
	const bool have_qual = slurp_file((dir + "/odd.qual").c_str(), P.odd_qual);
	if (have_qual != want_qual) { why = want_qual ? "qual.mcq without odd.qual" : "odd.qual without qual.mcq"; return false; }
	uint64_t odd_bytes = 0;
	P.n = P.len.size();
	host_index(P.len, L, P.slot, P.n_even, odd_bytes);
	if (P.n_even != n_even) { why = "len.bin counts another number of reads of the modal length than the archive holds"; return false; }
	if (aligned && !rebuild_odd) return true;                               // (the caller sets the sizes against the text it rebuilds)
	if (odd_bytes != P.odd_seq.size()) { why = "the lengths of len.bin do not add up to the size of odd.seq"; return false; }
	if (want_qual && odd_bytes != P.odd_qual.size()) { why = "the lengths of len.bin do not add up to the size of odd.qual"; return false; }
	return true;
}
