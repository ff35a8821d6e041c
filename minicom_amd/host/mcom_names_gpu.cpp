// minicom_amd/host/mcom_names_gpu.cpp -- the drivers of the read-name coder.
// File forms (bin/mcomz e --names, d): a file of name text <-> a `.mcn` member.  device = -1: the host twin (host/mcom_names.cpp);
// otherwise mcom_name_encode / mcom_name_decode on that GPU -- an error, never the host twin, when there is no such GPU.
// mcomh_fastq_names_to_device: the name text of a FASTQ file in HBM.  The text goes up through two page-locked pieces exactly as in
// mcomh_fastq_qualities_to_device (host/mcom_qual_gpu.cpp): the next piece is read while one travels, the unfinished record of a piece
// is carried in front of the next; on the card mcom_decode_line_index finds the lines and mcom_fastq_name_text checks every record and
// gathers its two lines.  This is a pass of its own over the file: `minicom -Q -N` reads the file once for qual.mcq and once for name.mcn.
// A BGZF file goes up compressed and is inflated on the card (mcom_gz_device_route, host/mcom_gzip_gpu.cpp);
// whatever is off there starts the file again through zlib's reader.
// mcomh_fastq_name_member: that and mcom_name_encode; device = -1 a host twin of the record rules and mcomh_name_encode.
// The _mate forms: the same drivers with a second name text, the mate, beside the first -- mcom[h]_name_encode_mate
// and mcom[h]_name_decode_mate stand where the calls without a mate stood.
// mcomh_verify_names_gpu: name.mcn decoded on the device against the file's name text, record against record (mcom_name_compare).
#include "../../include/mcom_host.h"
#include "../../include/mcom.h"
#include "mcom_gzip_gpu.hpp"
#include <hip/hip_runtime.h>
#include <zlib.h>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

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
struct DevBuf { mcom_ctx *ctx = nullptr; uint8_t *a = nullptr, *b = nullptr, *m = nullptr; ~DevBuf() { if (ctx) (void)mcom_sync(ctx); for (uint8_t *p : {a, b, m}) if (p) (void)hipFree(p); if (ctx) mcom_destroy(ctx); } };
// the mate text in a block of exactly its length (the coder reads it up to its last byte and no further)
bool upload_mate(DevBuf &D, const std::vector<uint8_t> &mate)
{
	if (mate.empty()) return true;
	return hipMalloc((void**)&D.m, mate.size()) == hipSuccess && hipMemcpy(D.m, mate.data(), mate.size(), hipMemcpyHostToDevice) == hipSuccess;
}
bool open_device(DevBuf &D, int device, size_t bytes_a, size_t bytes_b)
{
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev || hipSetDevice(device) != hipSuccess) return false;   // no such GPU: an error, never the host twin
	if (mcom_create(&D.ctx, device, nullptr) != MCOM_OK) { D.ctx = nullptr; return false; }
	return hipMalloc((void**)&D.a, bytes_a + 16) == hipSuccess && hipMalloc((void**)&D.b, bytes_b + 16) == hipSuccess;
}

const size_t DEFAULT_PIECE = (size_t)32 << 20;

int fail(char *err, size_t cap, const char *fmt, unsigned long long a = 0, unsigned long long b = 0)
{
	if (err && cap) snprintf(err, cap, fmt, a, b);
	return -1;
}
void record_message(char *err, size_t cap, unsigned long long record1, uint32_t bits)
{
	if (err && cap) snprintf(err, cap, "record %llu cannot keep its name:%s%s%s%s", record1, bits & MCOM_FASTQ_F_NAME ? " no '@' line" : "", bits & MCOM_FASTQ_F_PLUS ? " no '+' line" : "",
	                         bits & MCOM_FASTQ_F_LONG ? " a name or a '+' text above 255 bytes" : "", bits & MCOM_FASTQ_F_LENGTH ? " a damaged line index" : "");
}

struct Job {                                                // what one call holds, released however it ends
	mcom_ctx *ctx = nullptr; hipStream_t copy = nullptr; hipEvent_t ev[2] = {nullptr, nullptr};
	uint8_t *pin[2] = {nullptr, nullptr}, *d_text[2] = {nullptr, nullptr}, *d_names = nullptr;
	uint64_t *d_start = nullptr, *d_off = nullptr, *d_piece_off = nullptr; uint32_t *d_flag = nullptr;
	gzFile f = nullptr;
	~Job()
	{
		if (copy) (void)hipStreamSynchronize(copy);
		if (ctx) (void)mcom_sync(ctx);
		if (f) gzclose(f);
		for (int k = 0; k < 2; ++k) { if (pin[k]) (void)hipHostFree(pin[k]); if (d_text[k]) (void)hipFree(d_text[k]); if (ev[k]) (void)hipEventDestroy(ev[k]); }
		for (void *p : {(void*)d_start, (void*)d_off, (void*)d_piece_off, (void*)d_flag, (void*)d_names}) if (p) (void)hipFree(p);
		if (copy) (void)hipStreamDestroy(copy);
		if (ctx) mcom_destroy(ctx);
	}
};

// *d_names_out: the name text (release with mcomh_device_free), *bytes_out its length, *n_out the records
int names_to_device(const char *path, int device, size_t piece_bytes, uint8_t **d_names_out, uint64_t *bytes_out, size_t *n_out, char *err, size_t err_cap)
{
	if (!path || !d_names_out || !bytes_out || !n_out) return fail(err, err_cap, "null pointer");
	*d_names_out = nullptr; *bytes_out = 0; *n_out = 0;
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return fail(err, err_cap, "no GPU %llu (%llu visible)", (unsigned long long)device, (unsigned long long)n_dev);
	if (hipSetDevice(device) != hipSuccess) return fail(err, err_cap, "cannot select the GPU");
	size_t piece = piece_bytes ? piece_bytes : DEFAULT_PIECE;
	if (piece < 64) piece = 64;
	Job J;
	J.f = gzopen(path, "rb");
	if (!J.f) return fail(err, err_cap, "cannot open the file");
	if (mcom_create(&J.ctx, device, nullptr) != MCOM_OK) { J.ctx = nullptr; return fail(err, err_cap, "cannot create a context on the GPU"); }
	if (hipStreamCreate(&J.copy) != hipSuccess) return fail(err, err_cap, "no stream");
	if (hipMalloc((void**)&J.d_flag, 16) != hipSuccess) return fail(err, err_cap, "no room on the card");
	size_t cap_bytes = 0, n = 0, cap_lines = 0; uint64_t used = 0;
	auto room_for = [&](uint64_t bytes) {                                  // the text grows by doubling: its length is not known in advance
		if (bytes <= cap_bytes) return true;
		size_t want = cap_bytes ? cap_bytes : (size_t)1 << 16;
		while (want < bytes) want *= 2;
		uint8_t *p = nullptr;
		if (hipMalloc((void**)&p, want + 16) != hipSuccess) return false;
		if (used && hipMemcpy(p, J.d_names, used, hipMemcpyDeviceToDevice) != hipSuccess) { (void)hipFree(p); return false; }
		if (J.d_names) (void)hipFree(J.d_names);
		J.d_names = p; cap_bytes = want;
		return true;
	};
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
		while (p < e) { const uint8_t *q = (const uint8_t*)memchr(p, '\n', (size_t)(e - p)); if (!q) break; p = q + 1; if ((++lines & 3) == 0) { bytes = (size_t)(p - buf); records = lines / 4; } }
	};
	// A BGZF file goes up compressed and is inflated on the card (mcom_gzip_gpu.cpp): the same kernels over the same
	// records.  Whatever is off there -- also a record the kernel flags -- sends the file to zlib's reader below, from its beginning.
	size_t cap_off = 0;
	const bool on_device = mcom_gz_device_route(path, J.ctx, piece, [&](const uint8_t *d_text, uint64_t bytes, uint64_t records, const uint64_t *d_line_start) {
		if (n + records >= ((size_t)1 << 32) || !room_for(used + bytes)) return false;
		if (records + 1 > cap_off) {
			if (J.d_piece_off) (void)hipFree(J.d_piece_off);
			J.d_piece_off = nullptr; cap_off = 0;
			if (hipMalloc((void**)&J.d_piece_off, (records + 1) * 8 + 16) != hipSuccess) return false;
			cap_off = records + 1;
		}
		const uint32_t init[4] = {0, 0xFFFFFFFFu, 0, 0};
		uint32_t fl[4]; uint64_t got_bytes = 0;
		if (hipMemcpy(J.d_flag, init, 16, hipMemcpyHostToDevice) != hipSuccess ||
		    mcom_fastq_name_text(J.ctx, d_text, bytes, d_line_start, n, records, J.d_names + used, cap_bytes - used, &got_bytes, J.d_piece_off, J.d_flag) ||
		    hipMemcpy(fl, J.d_flag, 16, hipMemcpyDeviceToHost) != hipSuccess || fl[0] || fl[2]) return false;
		used += got_bytes; n += records;
		return true;
	});
	if (!on_device) {
		n = 0; used = 0;
		if (J.d_piece_off) (void)hipFree(J.d_piece_off);              // (the zlib route sizes it with its line index)
		J.d_piece_off = nullptr;
	}
	auto zlib_route = [&]() -> int {
	for (int k = 0; k < 2; ++k)
		if (hipHostMalloc((void**)&J.pin[k], piece + 1, hipHostMallocDefault) != hipSuccess || hipMalloc((void**)&J.d_text[k], piece + 16) != hipSuccess ||
		    hipEventCreateWithFlags(&J.ev[k], hipEventDisableTiming) != hipSuccess) return fail(err, err_cap, "no room for the pieces");
	size_t len = 0; bool eof = false;
	if (!fill(J.pin[0], 0, len, eof)) return fail(err, err_cap, "cannot read the file (a damaged gzip stream?)");
	for (int k = 0; ; k ^= 1) {
		size_t bytes, records;
		whole_records(J.pin[k], len, bytes, records);
		if (eof && bytes != len) return fail(err, err_cap, "the file ends inside record %llu", (unsigned long long)(n + records + 1));
		if (!eof && !records) return fail(err, err_cap, "record %llu is longer than a piece of %llu bytes", (unsigned long long)(n + 1), (unsigned long long)piece);
		if (n + records >= ((size_t)1 << 32)) return fail(err, err_cap, "more than 2^32 records");
		if (bytes && (hipMemcpyAsync(J.d_text[k], J.pin[k], bytes, hipMemcpyHostToDevice, J.copy) != hipSuccess || hipEventRecord(J.ev[k], J.copy) != hipSuccess)) return fail(err, err_cap, "upload failed");
		size_t next_len = 0; bool next_eof = true;
		if (!eof) {                                                           // the next piece is read while this one travels: its front is this piece's unfinished record
			memcpy(J.pin[k ^ 1], J.pin[k] + bytes, len - bytes);
			if (!fill(J.pin[k ^ 1], len - bytes, next_len, next_eof)) return fail(err, err_cap, "cannot read the file (a damaged gzip stream?)");
		}
		if (records) {
			if (hipEventSynchronize(J.ev[k]) != hipSuccess) return fail(err, err_cap, "upload failed");
			if (4 * records + 1 > cap_lines) {
				if (J.d_start) (void)hipFree(J.d_start);
				if (J.d_piece_off) (void)hipFree(J.d_piece_off);
				J.d_start = J.d_piece_off = nullptr; cap_lines = 4 * records + 1;
				if (hipMalloc((void**)&J.d_start, cap_lines * 8 + 16) != hipSuccess || hipMalloc((void**)&J.d_piece_off, (records + 1) * 8 + 16) != hipSuccess) return fail(err, err_cap, "no room on the card");
			}
			if (!room_for(used + bytes)) return fail(err, err_cap, "no room on the card for the name text");      // (a piece's name text is shorter than the piece)
			const uint32_t init[4] = {0, 0xFFFFFFFFu, 0, 0};
			if (hipMemcpy(J.d_flag, init, 16, hipMemcpyHostToDevice) != hipSuccess) return fail(err, err_cap, "upload failed");
			uint64_t got_lines = 0, got_bytes = 0;
			if (mcom_decode_line_index(J.ctx, J.d_text[k], bytes, J.d_start, 4 * records, &got_lines, J.d_flag + 2) || got_lines != 4 * records ||
			    mcom_fastq_name_text(J.ctx, J.d_text[k], bytes, J.d_start, n, records, J.d_names + used, cap_bytes - used, &got_bytes, J.d_piece_off, J.d_flag)) {
				if (err && err_cap) snprintf(err, err_cap, "device call failed: %s", mcom_last_error(J.ctx));
				return -1;
			}
			uint32_t fl[4];
			if (hipMemcpy(fl, J.d_flag, 16, hipMemcpyDeviceToHost) != hipSuccess) return fail(err, err_cap, "cannot read the flag word");
			if (fl[0] || fl[2]) { record_message(err, err_cap, (unsigned long long)fl[1] + 1, fl[0]); return -1; }
			used += got_bytes; n += records;
		}
		if (eof) break;
		len = next_len; eof = next_eof;
	}
	return 0;
	};
	if (!on_device) { const int rc = zlib_route(); if (rc) return rc; }
	if (!room_for(1)) return fail(err, err_cap, "no room on the card");
	*d_names_out = J.d_names; J.d_names = nullptr;
	*bytes_out = used; *n_out = n;
	return 0;
}

// The host twin of the route above (`minicom -N` without -G): the same records accepted, the same refused, the same first bad record named.
int host_names(const char *path, std::vector<uint8_t> &names, size_t &n, char *err, size_t err_cap)
{
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
	names.clear(); n = 0;
	size_t at = 0, start[5];
	while (at < text.size()) {
		start[0] = at;
		for (int q = 1; q <= 4; ++q) {
			const uint8_t *nl = at < text.size() ? (const uint8_t*)memchr(text.data() + at, '\n', text.size() - at) : nullptr;
			if (!nl) return fail(err, err_cap, "the file ends inside record %llu", (unsigned long long)(n + 1));
			at = (size_t)(nl - text.data()) + 1; start[q] = at;
		}
		if (n + 1 >= ((size_t)1 << 32)) return fail(err, err_cap, "more than 2^32 records");
		const size_t a = start[0], b = start[1], c = start[2], d = start[3];
		uint32_t bad = 0;
		if (b - 1 - a < 1 || text[a] != '@') bad |= MCOM_FASTQ_F_NAME;
		if (d - 1 - c < 1 || text[c] != '+') bad |= MCOM_FASTQ_F_PLUS;
		if (!bad && (b - 2 - a > 255 || d - 2 - c > 255)) bad |= MCOM_FASTQ_F_LONG;
		if (bad) { record_message(err, err_cap, (unsigned long long)n + 1, bad); return -1; }
		names.insert(names.end(), text.begin() + a + 1, text.begin() + b);
		names.insert(names.end(), text.begin() + c + 1, text.begin() + d);
		++n;
	}
	return 0;
}

struct DevText { uint8_t *d = nullptr; ~DevText() { mcomh_device_free(d); } };

// mate_fastq != NULL: `fastq` is the second file of a pair and mate_fastq the first; the member is coded against the first file's names
int fastq_member(const char *fastq, const char *mate_fastq, int device, const char *out_path, uint64_t *n_out, char *err, size_t err_cap)
{
	if (!fastq || !out_path) return fail(err, err_cap, "null pointer");
	std::vector<uint8_t> out;
	uint64_t len = 0, bad = ~(uint64_t)0; size_t n = 0, n_mate = 0;
	if (device < 0) {
		std::vector<uint8_t> names, mate;
		if (host_names(fastq, names, n, err, err_cap)) return -1;
		if (mate_fastq && host_names(mate_fastq, mate, n_mate, err, err_cap)) return -1;
		if (mate_fastq && n_mate != n) return fail(err, err_cap, "%llu records, its mate file has %llu", (unsigned long long)n, (unsigned long long)n_mate);
		out.resize(mcomh_name_bound(names.size()));
		if (mate_fastq ? mcomh_name_encode_mate(names.data(), names.size(), n, mate.data(), mate.size(), out.data(), out.size(), &len, &bad)
		               : mcomh_name_encode(names.data(), names.size(), n, out.data(), out.size(), &len, &bad)) return fail(err, err_cap, "the name coder failed (more than 171798691 records, or 4 GiB of names or more?)");
	} else {
		DevText in, mate; uint64_t bytes = 0, mate_bytes = 0;
		if (names_to_device(fastq, device, 0, &in.d, &bytes, &n, err, err_cap)) return -1;
		if (mate_fastq && names_to_device(mate_fastq, device, 0, &mate.d, &mate_bytes, &n_mate, err, err_cap)) return -1;
		if (mate_fastq && n_mate != n) return fail(err, err_cap, "%llu records, its mate file has %llu", (unsigned long long)n, (unsigned long long)n_mate);
		const uint64_t cap = mcomh_name_bound(bytes);
		struct Dev { mcom_ctx *ctx = nullptr; uint8_t *d_out = nullptr; ~Dev() { if (ctx) (void)mcom_sync(ctx); if (d_out) (void)hipFree(d_out); if (ctx) mcom_destroy(ctx); } } D;
		if (mcom_create(&D.ctx, device, nullptr) != MCOM_OK) { D.ctx = nullptr; return fail(err, err_cap, "cannot create a context on the GPU"); }
		if (hipMalloc((void**)&D.d_out, cap + 16) != hipSuccess) return fail(err, err_cap, "no room on the card");
		if (mate_fastq ? mcom_name_encode_mate(D.ctx, in.d, bytes, n, mate.d, mate_bytes, D.d_out, cap, &len, &bad) : mcom_name_encode(D.ctx, in.d, bytes, n, D.d_out, cap, &len, &bad)) {
			if (err && err_cap) snprintf(err, err_cap, "%s", mcom_last_error(D.ctx));
			return -1;
		}
		out.resize(len);
		if (len && hipMemcpy(out.data(), D.d_out, len, hipMemcpyDeviceToHost) != hipSuccess) return fail(err, err_cap, "download failed");
	}
	if (!write_file(out_path, out.data(), len)) return fail(err, err_cap, "cannot write the member");
	if (n_out) *n_out = n;
	return 0;
}

// member: name.mcn, or name_1.mcn / name_2.mcn of a pair.  mate_member != NULL: the member is decoded against the decoded text of that
// member of the folder (name_2.mcn against name_1.mcn)
int verify_names(const char *folder, const char *member_name, const char *mate_member, const char *fastq, int device, mcomh_verify_report *rep)
{
	std::vector<uint8_t> member, mmember;
	if (!slurp_file((std::string(folder) + "/" + member_name).c_str(), member)) { fprintf(stderr, "minicom verify: %s has no %s\n", folder, member_name); return -1; }
	if (mate_member && !slurp_file((std::string(folder) + "/" + mate_member).c_str(), mmember)) { fprintf(stderr, "minicom verify: %s has no %s, which %s is coded against\n", folder, mate_member, member_name); return -1; }
	uint64_t nn = 0, tl = 0, mn = 0, mtl = 0;
	if (mate_member ? mcom_name_info_mate(member.data(), member.size(), &nn, &tl) : mcom_name_info(member.data(), member.size(), &nn, &tl)) { fprintf(stderr, "minicom verify: %s/%s is not a .mcn member\n", folder, member_name); return -1; }
	if (mate_member && mcom_name_info(mmember.data(), mmember.size(), &mn, &mtl)) { fprintf(stderr, "minicom verify: %s/%s is not a .mcn member\n", folder, mate_member); return -1; }
	DevText in; uint64_t in_bytes = 0; size_t n_in = 0;
	char err[320] = "";
	if (names_to_device(fastq, device, 0, &in.d, &in_bytes, &n_in, err, sizeof err)) { fprintf(stderr, "minicom verify: cannot read the names of %s: %s\n", fastq, err); return -1; }
	struct Dev { mcom_ctx *ctx = nullptr; std::vector<void*> v; ~Dev() { if (ctx) (void)mcom_sync(ctx); for (void *p : v) (void)hipFree(p); if (ctx) mcom_destroy(ctx); }
	             void *get(size_t bytes) { void *p = nullptr; if (hipMalloc(&p, bytes + 16) != hipSuccess) return nullptr; v.push_back(p); return p; } } D;
	if (mcom_create(&D.ctx, device, nullptr) != MCOM_OK) { D.ctx = nullptr; return -1; }
	uint8_t *d_member = (uint8_t*)D.get(member.size()), *d_text = (uint8_t*)D.get(tl);
	uint64_t *d_off = (uint64_t*)D.get((nn + 1) * 8), *d_off_in = (uint64_t*)D.get((n_in + 1) * 8);
	if (!d_member || !d_text || !d_off || !d_off_in) { fprintf(stderr, "minicom verify: the card has no room for the names\n"); return -1; }
	if (hipMemcpy(d_member, member.data(), member.size(), hipMemcpyHostToDevice) != hipSuccess) return -1;
	if (mate_member) {
		uint8_t *d_mm = (uint8_t*)D.get(mmember.size()), *d_mate = (uint8_t*)D.get(mtl);
		if (!d_mm || !d_mate || hipMemcpy(d_mm, mmember.data(), mmember.size(), hipMemcpyHostToDevice) != hipSuccess) return -1;
		if (mcom_name_decode(D.ctx, d_mm, mmember.size(), d_mate, mtl, &mtl, &mn, nullptr)) { fprintf(stderr, "minicom verify: %s/%s refused: %s\n", folder, mate_member, mcom_last_error(D.ctx)); return -1; }
		if (mcom_name_decode_mate(D.ctx, d_member, member.size(), d_mate, mtl, d_text, tl, &tl, &nn) || mcom_name_text_offsets(D.ctx, d_text, tl, nn, d_off)) {
			fprintf(stderr, "minicom verify: %s/%s refused: %s\n", folder, member_name, mcom_last_error(D.ctx)); return -1;
		}
	} else if (mcom_name_decode(D.ctx, d_member, member.size(), d_text, tl, &tl, &nn, d_off)) { fprintf(stderr, "minicom verify: %s/%s refused: %s\n", folder, member_name, mcom_last_error(D.ctx)); return -1; }
	rep->mode = 1; rep->n_input = n_in; rep->n_archive = nn;
	rep->missing = n_in > nn ? n_in - nn : 0; rep->extra = nn > n_in ? nn - n_in : 0;
	const uint64_t common = n_in < nn ? n_in : nn;
	uint64_t differing = 0, first = ~(uint64_t)0;
	if (mcom_name_text_offsets(D.ctx, in.d, in_bytes, n_in, d_off_in) || mcom_name_compare(D.ctx, in.d, d_off_in, in_bytes, d_text, d_off, tl, common, &differing, &first)) {
		fprintf(stderr, "minicom verify: %s\n", mcom_last_error(D.ctx)); return -1;
	}
	rep->differing = differing; rep->first_diff = first;
	rep->identical = n_in == nn && differing == 0;
	return 0;
}

// name_1.mcn against the names of fastq1 and name_2.mcn against those of fastq2 in one context: name_1 is decoded once and serves both
// as what is compared with the first file and as the mate that name_2 is decoded against
int verify_names_pair(const char *folder, const char *fastq1, const char *fastq2, int device, mcomh_verify_report *rep1, mcomh_verify_report *rep2)
{
	std::vector<uint8_t> m[2];
	uint64_t nn[2] = {0, 0}, tl[2] = {0, 0};
	for (int k = 0; k < 2; ++k) {
		const char *name = k ? "name_2.mcn" : "name_1.mcn";
		if (!slurp_file((std::string(folder) + "/" + name).c_str(), m[k])) { fprintf(stderr, "minicom verify: %s has no %s\n", folder, name); return -1; }
		if (k ? mcom_name_info_mate(m[k].data(), m[k].size(), &nn[k], &tl[k]) : mcom_name_info(m[k].data(), m[k].size(), &nn[k], &tl[k])) { fprintf(stderr, "minicom verify: %s/%s is not a .mcn member\n", folder, name); return -1; }
	}
	struct Dev { mcom_ctx *ctx = nullptr; std::vector<void*> v; ~Dev() { if (ctx) (void)mcom_sync(ctx); for (void *p : v) (void)hipFree(p); if (ctx) mcom_destroy(ctx); }
	             void *get(size_t bytes) { void *p = nullptr; if (hipMalloc(&p, bytes + 16) != hipSuccess) return nullptr; v.push_back(p); return p; } } D;
	if (mcom_create(&D.ctx, device, nullptr) != MCOM_OK) { D.ctx = nullptr; return -1; }
	uint8_t *d_text[2] = {nullptr, nullptr}; uint64_t *d_off[2] = {nullptr, nullptr};
	const char *fq[2] = {fastq1, fastq2};
	mcomh_verify_report *rep[2] = {rep1, rep2};
	for (int k = 0; k < 2; ++k) {
		uint8_t *d_member = (uint8_t*)D.get(m[k].size());
		d_text[k] = (uint8_t*)D.get(tl[k]); d_off[k] = (uint64_t*)D.get((nn[k] + 1) * 8);
		if (!d_member || !d_text[k] || !d_off[k] || hipMemcpy(d_member, m[k].data(), m[k].size(), hipMemcpyHostToDevice) != hipSuccess) { fprintf(stderr, "minicom verify: the card has no room for the names\n"); return -1; }
		const int rc = k ? (mcom_name_decode_mate(D.ctx, d_member, m[1].size(), d_text[0], tl[0], d_text[1], tl[1], &tl[1], &nn[1]) || mcom_name_text_offsets(D.ctx, d_text[1], tl[1], nn[1], d_off[1]))
		                 : mcom_name_decode(D.ctx, d_member, m[0].size(), d_text[0], tl[0], &tl[0], &nn[0], d_off[0]);
		if (rc) { fprintf(stderr, "minicom verify: %s/name_%d.mcn refused: %s\n", folder, k + 1, mcom_last_error(D.ctx)); return -1; }
		DevText in; uint64_t in_bytes = 0; size_t n_in = 0;
		char err[320] = "";
		if (names_to_device(fq[k], device, 0, &in.d, &in_bytes, &n_in, err, sizeof err)) { fprintf(stderr, "minicom verify: cannot read the names of %s: %s\n", fq[k], err); return -1; }
		uint64_t *d_off_in = (uint64_t*)D.get((n_in + 1) * 8);
		if (!d_off_in) return -1;
		mcomh_verify_report *r = rep[k];
		r->mode = 1; r->n_input = n_in; r->n_archive = nn[k];
		r->missing = n_in > nn[k] ? n_in - nn[k] : 0; r->extra = nn[k] > n_in ? nn[k] - n_in : 0;
		uint64_t differing = 0, first = ~(uint64_t)0;
		if (mcom_name_text_offsets(D.ctx, in.d, in_bytes, n_in, d_off_in) ||
		    mcom_name_compare(D.ctx, in.d, d_off_in, in_bytes, d_text[k], d_off[k], tl[k], n_in < nn[k] ? n_in : nn[k], &differing, &first)) { fprintf(stderr, "minicom verify: %s\n", mcom_last_error(D.ctx)); return -1; }
		r->differing = differing; r->first_diff = first;
		r->identical = n_in == nn[k] && differing == 0;
	}
	return 0;
}

// mate_path != NULL: a file of name text, the mate the member is coded against or was coded against
int name_file(const char *in_path, const char *mate_path, const char *out_path, int device, bool pack)
{
	if (!in_path || !out_path) return -1;
	std::vector<uint8_t> in, out, mate;
	if (!slurp_file(in_path, in)) return -1;
	if (mate_path && !slurp_file(mate_path, mate)) return -1;
	if (pack) {
		uint64_t lines = 0, len = 0, bad = ~(uint64_t)0;
		for (uint8_t c : in) lines += c == '\n';
		if (lines & 1) { fprintf(stderr, "mcomz: %llu lines are not two lines per record\n", (unsigned long long)lines); return -1; }
		const uint64_t n = lines / 2, cap = mcomh_name_bound(in.size());
		out.resize(cap);
		if (device < 0) {
			if (mate_path ? mcomh_name_encode_mate(in.data(), in.size(), n, mate.data(), mate.size(), out.data(), cap, &len, &bad) : mcomh_name_encode(in.data(), in.size(), n, out.data(), cap, &len, &bad)) {
				if (bad != ~(uint64_t)0) fprintf(stderr, "mcomz: record %llu has a name or a '+' text above 255 bytes\n", (unsigned long long)bad + 1);
				return -1;
			}
		} else {
			DevBuf D;
			if (!open_device(D, device, in.size(), cap)) return -1;
			if (in.size() && hipMemcpy(D.a, in.data(), in.size(), hipMemcpyHostToDevice) != hipSuccess) return -1;
			if (!upload_mate(D, mate)) return -1;
			if (mate_path ? mcom_name_encode_mate(D.ctx, D.a, in.size(), n, D.m, mate.size(), D.b, cap, &len, &bad) : mcom_name_encode(D.ctx, D.a, in.size(), n, D.b, cap, &len, &bad)) { fprintf(stderr, "mcomz: %s\n", mcom_last_error(D.ctx)); return -1; }
			if (hipMemcpy(out.data(), D.b, len, hipMemcpyDeviceToHost) != hipSuccess) return -1;
		}
		return write_file(out_path, out.data(), len) ? 0 : -1;
	}
	uint64_t n = 0, text_len = 0, gn = 0, gt = 0;
	if (mate_path ? mcomh_name_info_mate(in.data(), in.size(), &n, &text_len) : mcomh_name_info(in.data(), in.size(), &n, &text_len)) return -1;
	out.resize(text_len + 1);
	if (device < 0) {
		if (mate_path ? mcomh_name_decode_mate(in.data(), in.size(), mate.data(), mate.size(), out.data(), text_len, &gt, &gn) : mcomh_name_decode(in.data(), in.size(), out.data(), text_len, &gt, &gn)) return -1;
	}
	else {
		DevBuf D;
		if (!open_device(D, device, in.size(), text_len)) return -1;
		if (hipMemcpy(D.a, in.data(), in.size(), hipMemcpyHostToDevice) != hipSuccess) return -1;
		if (!upload_mate(D, mate)) return -1;
		if (mate_path ? mcom_name_decode_mate(D.ctx, D.a, in.size(), D.m, mate.size(), D.b, text_len, &gt, &gn) : mcom_name_decode(D.ctx, D.a, in.size(), D.b, text_len, &gt, &gn, nullptr)) { fprintf(stderr, "mcomz: %s\n", mcom_last_error(D.ctx)); return -1; }
		if (text_len && hipMemcpy(out.data(), D.b, text_len, hipMemcpyDeviceToHost) != hipSuccess) return -1;
	}
	return write_file(out_path, out.data(), text_len) ? 0 : -1;
}

}  // namespace

extern "C" int mcomh_name_pack_file(const char *in_path, const char *out_path, int device) { try { return name_file(in_path, nullptr, out_path, device, true); } catch (...) { return -1; } }
extern "C" int mcomh_name_unpack_file(const char *in_path, const char *out_path, int device) { try { return name_file(in_path, nullptr, out_path, device, false); } catch (...) { return -1; } }
extern "C" int mcomh_name_pack_file_mate(const char *in_path, const char *mate_path, const char *out_path, int device)
{
	if (!mate_path) return -1;
	try { return name_file(in_path, mate_path, out_path, device, true); } catch (...) { return -1; }
}
extern "C" int mcomh_name_unpack_file_mate(const char *in_path, const char *mate_path, const char *out_path, int device)
{
	if (!mate_path) return -1;
	try { return name_file(in_path, mate_path, out_path, device, false); } catch (...) { return -1; }
}

extern "C" int mcomh_fastq_names_to_device(const char *path, int device, size_t piece_bytes, uint8_t **d_names, uint64_t *bytes, size_t *n, char *err, size_t err_cap)
{
	if (err && err_cap) err[0] = 0;
	try { return names_to_device(path, device, piece_bytes, d_names, bytes, n, err, err_cap); } catch (...) { return -1; }
}
extern "C" int mcomh_fastq_name_member(const char *fastq, int device, const char *out_path, uint64_t *n, char *err, size_t err_cap)
{
	if (err && err_cap) err[0] = 0;
	try { return fastq_member(fastq, nullptr, device, out_path, n, err, err_cap); } catch (...) { return -1; }
}
extern "C" int mcomh_fastq_name_member_mate(const char *fastq2, const char *fastq1, int device, const char *out_path, uint64_t *n, char *err, size_t err_cap)
{
	if (err && err_cap) err[0] = 0;
	if (!fastq1) return fail(err, err_cap, "null pointer");
	try { return fastq_member(fastq2, fastq1, device, out_path, n, err, err_cap); } catch (...) { return -1; }
}
extern "C" int mcomh_verify_names_member_gpu(const char *folder, const char *member, const char *mate_member, const char *fastq, int device, mcomh_verify_report *rep)
{
	if (!folder || !member || !fastq || !rep) { fprintf(stderr, "minicom verify: bad arguments (a folder with name.mcn and one FASTQ file)\n"); return -1; }
	memset(rep, 0, sizeof(*rep));
	rep->first_diff = ~(uint64_t)0;
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) { fprintf(stderr, "minicom verify: no GPU %d (%d visible); there is no host route\n", device, n_dev); return -1; }
	try { return verify_names(folder, member, mate_member, fastq, device, rep); } catch (...) { return -1; }
}
extern "C" int mcomh_verify_names_gpu(const char *folder, const char *fastq, int device, mcomh_verify_report *rep) { return mcomh_verify_names_member_gpu(folder, "name.mcn", nullptr, fastq, device, rep); }

// ---- a pair kept in input order: every check the archive's members allow, file by file ----
// part 0 the reads, line against line over both files; 1 / 2 the quality lines of file 1 / 2; 3 / 4 the names and '+' lines of file 1 / 2.
// present[k] says whether check k was made (the archive holds its members).  -1 when a check could not be made, or when the archive
// holds one quality member of two, name_2 without name_1 (or the reverse), or names without quality values.
extern "C" int mcomh_verify_order_pe_parts_gpu(const char *folder, const char *fastq1, const char *fastq2, int device, mcomh_verify_report rep[5], int present[5])
{
	if (!folder || !fastq1 || !fastq2 || !rep || !present) { fprintf(stderr, "minicom verify: bad arguments (a folder and the two FASTQ files)\n"); return -1; }
	auto has = [&](const char *name) { FILE *f = fopen((std::string(folder) + "/" + name).c_str(), "rb"); if (f) fclose(f); return f != nullptr; };
	const bool q1 = has("qual_1.mcq"), q2 = has("qual_2.mcq"), n1 = has("name_1.mcn"), n2 = has("name_2.mcn");
	if (q1 != q2 || n1 != n2 || (n1 && !q1)) { fprintf(stderr, "minicom verify: %s holds one member of a pair of members without the other, or names without quality values\n", folder); return -1; }
	for (int k = 0; k < 5; ++k) { memset(&rep[k], 0, sizeof rep[k]); present[k] = 0; }
	present[0] = 1; present[1] = present[2] = q1; present[3] = present[4] = n1;
	int rc = mcomh_verify_order_pe_reads_gpu(folder, fastq1, fastq2, device, &rep[0]);
	if (q1) rc |= mcomh_verify_quality_member_gpu(folder, "qual_1.mcq", fastq1, device, &rep[1]) | mcomh_verify_quality_member_gpu(folder, "qual_2.mcq", fastq2, device, &rep[2]);
	if (n1) {
		rep[3].first_diff = rep[4].first_diff = ~(uint64_t)0;
		try { rc |= verify_names_pair(folder, fastq1, fastq2, device, &rep[3], &rep[4]); } catch (...) { rc = -1; }
	}
	return rc ? -1 : 0;
}
// the same as one verdict: identical when every check made says so; the counts are the reads', `differing` is summed over the checks
extern "C" int mcomh_verify_order_pe_gpu(const char *folder, const char *fastq1, const char *fastq2, int device, mcomh_verify_report *rep)
{
	if (!rep) return -1;
	mcomh_verify_report part[5]; int present[5];
	if (mcomh_verify_order_pe_parts_gpu(folder, fastq1, fastq2, device, part, present)) return -1;
	*rep = part[0];
	for (int k = 1; k < 5; ++k) if (present[k]) { rep->identical = rep->identical && part[k].identical; rep->differing += part[k].differing; }
	return 0;
}
