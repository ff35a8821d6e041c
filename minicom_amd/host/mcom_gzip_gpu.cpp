// minicom_amd/host/mcom_gzip_gpu.cpp -- BGZF input inflated on the GPU, and the host twin of that.
// mcomh_gzip_inflate / mcomh_gzip_inflate_members are a plain loop over csrc/inflate_model.hpp, which the kernel compiles as well: the
// same bytes and the same status per member as mcom_gzip_inflate.  This half builds alone with -DMCOM_GZIP_HOST_ONLY
// (tests/fuzz_inflate_model.cpp runs it under the sanitizers).
// mcomh_gunzip_file: a BGZF file to its text; device >= 0 uploads runs of whole members, inflates them on that GPU and brings the text
// down.  mcom_gz_device_route (mcom_gzip_gpu.hpp) is the piece loop of the two FASTQ passes (mcom_qual_gpu.cpp, mcom_names_gpu.cpp): the
// members of a piece are read into page-locked memory and uploaded while the piece before is worked on, inflated behind the carried
// bytes of the unfinished record, the lines indexed, the whole records handed to the pass and the rest carried on by a device-to-device
// copy.  Whatever is off sends the file to the passes' zlib route, from its beginning.
#include "../../include/mcom_host.h"
#include "../../include/mcom_test.h"
#include "../csrc/inflate_model.hpp"
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>
#ifndef MCOM_GZIP_HOST_ONLY
#include "../../include/mcom.h"
#include "mcom_gzip_gpu.hpp"
#include <hip/hip_runtime.h>
#endif

using namespace mcom_inflate_model;

namespace {

static_assert(sizeof(mcomh_gzip_member) == sizeof(Member) && offsetof(mcomh_gzip_member, in_bytes) == offsetof(Member, in_bytes) && offsetof(mcomh_gzip_member, out_off) == offsetof(Member, out_off) &&
              offsetof(mcomh_gzip_member, isize) == offsetof(Member, isize) && offsetof(mcomh_gzip_member, crc) == offsetof(Member, crc), "the model's member is the interface's");

struct CrcTable { uint32_t t[256]; CrcTable() { for (uint32_t i = 0; i < 256; ++i) t[i] = mcom_deflate::crc_table_entry(i); } };
const uint32_t *crc_table() { static const CrcTable c; return c.t; }

int inflate_table(const uint8_t *in, uint64_t in_bytes, const Member *tab, uint64_t n, uint8_t *out, uint64_t out_bytes, uint8_t *status, uint64_t *bad, uint64_t *first_bad)
{
	int why = 0;
	if (check_table(tab, n, in_bytes, out_bytes, &why) >= 0) return -1;
	Tables *T = new (std::nothrow) Tables;
	if (!T) return -1;
	uint64_t nb = 0, fb = n;
	for (uint64_t m = 0; m < n; ++m) {
		const int st = inflate_member(in, tab[m], out, *T, crc_table());
		if (status) status[m] = (uint8_t)st;
		if (st) { if (!nb) fb = m; ++nb; }
	}
	delete T;
	if (bad) *bad = nb;
	if (first_bad) *first_bad = fb;
	return 0;
}

const size_t FILE_PIECE = (size_t)32 << 20;                       // text per piece of mcomh_gunzip_file

int host_gunzip_file(const char *in_path, const char *out_path)
{
	FILE *fin = fopen(in_path, "rb");
	if (!fin) return -1;
	std::vector<uint8_t> file;
	{
		uint8_t buf[65536]; size_t got;
		while ((got = fread(buf, 1, sizeof buf, fin)) > 0) file.insert(file.end(), buf, buf + got);
		const bool bad = ferror(fin) != 0;
		fclose(fin);
		if (bad) return -1;
	}
	uint64_t n = 0, text = 0, used = 0;
	if (!walk_members(file.data(), file.size(), nullptr, 0, &n, &text, &used) || used != file.size() || !n) return -1;   // (a file without a member is no BGZF file)
	std::vector<Member> tab((size_t)n);
	walk_members(file.data(), file.size(), tab.data(), n, &n, &text, &used);
	std::vector<uint8_t> out((size_t)text + 1);
	uint64_t bad = 0, first = 0;
	if (inflate_table(file.data(), file.size(), tab.data(), n, out.data(), text, nullptr, &bad, &first) || bad) return -1;
	FILE *fout = fopen(out_path, "wb");
	if (!fout) return -1;
	const bool ok = !text || fwrite(out.data(), 1, (size_t)text, fout) == text;
	if (fclose(fout) != 0 || !ok) { remove(out_path); return -1; }
	return 0;
}

#ifndef MCOM_GZIP_HOST_ONLY
long g_device_members = 0;

// Runs of whole members out of a file, through two page-locked buffers: stage() reads the next run and sends it on its way to the card,
// wait() is called before the run is used.  A run staged while the one before is worked on travels beside that work.
struct Feed {
	FILE *f = nullptr; hipStream_t copy = nullptr; hipEvent_t ev[2] = {nullptr, nullptr};
	uint8_t *pin[2] = {nullptr, nullptr}, *d_comp[2] = {nullptr, nullptr};
	mcom_gzip_member *pin_tab[2] = {nullptr, nullptr}, *d_tab[2] = {nullptr, nullptr};
	size_t cap = 0, max_members = 0, have = 0, consumed = 0;
	uint64_t max_text = 0;
	int cur = 1;
	bool file_eof = false;
	struct Run { int k = 0; uint64_t comp_bytes = 0, n_members = 0, text = 0; };
	~Feed()
	{
		if (copy) (void)hipStreamSynchronize(copy);
		if (f) fclose(f);
		for (int k = 0; k < 2; ++k) {
			if (pin[k]) (void)hipHostFree(pin[k]);
			if (pin_tab[k]) (void)hipHostFree(pin_tab[k]);
			if (d_comp[k]) (void)hipFree(d_comp[k]);
			if (d_tab[k]) (void)hipFree(d_tab[k]);
			if (ev[k]) (void)hipEventDestroy(ev[k]);
		}
		if (copy) (void)hipStreamDestroy(copy);
	}
	// false: cannot open, no room, or the file's first member carries no BC field (nothing is allocated before that is known)
	bool open(const char *path, uint64_t piece_text)
	{
		f = fopen(path, "rb");
		if (!f) return false;
		uint8_t head[512];
		const size_t got = fread(head, 1, sizeof head, f);
		uint64_t n = 0, text = 0, used = 0;
		walk_members(head, got, nullptr, 0, &n, &text, &used);
		if (!n) {                                                      // (a first member above 512 bytes: its header alone is looked at)
			bool bc = false;
			if (got >= 18 && head[0] == 0x1f && head[1] == 0x8b && head[2] == 8 && !(head[3] & 0xE0) && (head[3] & 4)) {
				const size_t xend = 12 + (size_t)le16(head + 10);
				for (size_t q = 12; q + 4 <= xend && q + 4 <= got; ) {
					const size_t sl = le16(head + q + 2);
					if (head[q] == 'B' && head[q + 1] == 'C' && sl == 2) { bc = true; break; }
					q += 4 + sl;
				}
			}
			if (!bc) return false;
		}
		if (fseek(f, 0, SEEK_SET)) return false;
		max_text = piece_text;
		cap = (size_t)piece_text + 2 * 65536;
		max_members = (size_t)(piece_text / 512) + 64;
		if (hipStreamCreate(&copy) != hipSuccess) return false;
		for (int k = 0; k < 2; ++k)
			if (hipHostMalloc((void**)&pin[k], cap, hipHostMallocDefault) != hipSuccess || hipHostMalloc((void**)&pin_tab[k], max_members * sizeof(mcom_gzip_member), hipHostMallocDefault) != hipSuccess ||
			    hipMalloc((void**)&d_comp[k], cap + 16) != hipSuccess || hipMalloc((void**)&d_tab[k], max_members * sizeof(mcom_gzip_member)) != hipSuccess ||
			    hipEventCreateWithFlags(&ev[k], hipEventDisableTiming) != hipSuccess) return false;
		return true;
	}
	// 0: a run is on its way; 1: the file ended behind the run before; -1: what follows is no whole BGZF member
	int stage(Run &r)
	{
		const int nk = cur ^ 1;
		const size_t tail = have - consumed;
		if (tail) memcpy(pin[nk], pin[cur] + consumed, tail);          // (pin[nk]: the run before the last one, long since on the card)
		cur = nk; have = tail; consumed = 0;
		while (have < cap && !file_eof) {
			const size_t got = fread(pin[cur] + have, 1, cap - have, f);
			if (!got) { if (ferror(f)) return -1; file_eof = true; }
			have += got;
		}
		if (!have) return 1;
		uint64_t n = 0, text = 0, used = 0;
		walk_members(pin[cur], have, reinterpret_cast<Member*>(pin_tab[cur]), max_members, &n, &text, &used);
		if (!n) return -1;                                              // (a BGZF member is at most 65536 bytes: one always fits the buffer)
		uint64_t j = 0, t = 0;
		for (; j < n; ++j) {
			const uint64_t sz = pin_tab[cur][j].isize;
			if (sz > 65536) { if (!j) return -1; break; }              // not a BGZF member's text: the run ends in front of it, the next one refuses it
			if (j && t + sz > max_text) break;                         // one member at least, however small the piece
			t += sz;
		}
		r.k = cur; r.n_members = j; r.text = t;
		r.comp_bytes = pin_tab[cur][j - 1].in_off + pin_tab[cur][j - 1].in_bytes + 8;
		consumed = (size_t)r.comp_bytes;
		if (hipMemcpyAsync(d_comp[cur], pin[cur], (size_t)r.comp_bytes, hipMemcpyHostToDevice, copy) != hipSuccess ||
		    hipMemcpyAsync(d_tab[cur], pin_tab[cur], (size_t)j * sizeof(mcom_gzip_member), hipMemcpyHostToDevice, copy) != hipSuccess ||
		    hipEventRecord(ev[cur], copy) != hipSuccess) return -1;
		return 0;
	}
	bool wait(const Run &r) { return hipEventSynchronize(ev[r.k]) == hipSuccess; }
};

struct DevBlocks {                                                    // device and page-locked blocks of one call, freed however it ends
	std::vector<void*> dev, host;
	~DevBlocks() { for (void *p : dev) (void)hipFree(p); for (void *p : host) (void)hipHostFree(p); }
	template <class T> bool get(T **out, size_t bytes) { void *p = nullptr; if (hipMalloc(&p, bytes) != hipSuccess) return false; dev.push_back(p); *out = (T*)p; return true; }
	template <class T> bool get_host(T **out, size_t bytes) { void *p = nullptr; if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return false; host.push_back(p); *out = (T*)p; return true; }
};
struct Ctx { mcom_ctx *ctx = nullptr; ~Ctx() { if (ctx) { (void)mcom_sync(ctx); mcom_destroy(ctx); } } };

int device_gunzip_file(const char *in_path, const char *out_path, int device)
{
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev) return -1;      // no such GPU: an error, never the host twin
	if (hipSetDevice(device) != hipSuccess) return -1;
	Feed F;                                                           // (declared first: destroyed last, behind the context's work)
	DevBlocks B;
	Ctx C;
	if (!F.open(in_path, FILE_PIECE)) return -1;
	if (mcom_create(&C.ctx, device, nullptr) != MCOM_OK) { C.ctx = nullptr; return -1; }
	uint8_t *d_text = nullptr, *d_status = nullptr, *pin_text = nullptr;
	if (!B.get(&d_text, FILE_PIECE + 65536 + 16) || !B.get(&d_status, F.max_members) || !B.get_host(&pin_text, FILE_PIECE + 65536)) return -1;
	FILE *fout = fopen(out_path, "wb");
	if (!fout) return -1;
	bool ok = true;
	Feed::Run run, next;
	int rc = F.stage(run);
	while (rc == 0) {
		const int rc_next = F.stage(next);                            // the next run is read and sent while this one is inflated
		uint64_t bad = 0, first = 0;
		ok = F.wait(run) && mcom_gzip_inflate(C.ctx, F.d_comp[run.k], run.comp_bytes, F.d_tab[run.k], run.n_members, d_text, run.text, d_status, &bad, &first) == MCOM_OK && !bad &&
		     (!run.text || (hipMemcpy(pin_text, d_text, (size_t)run.text, hipMemcpyDeviceToHost) == hipSuccess && fwrite(pin_text, 1, (size_t)run.text, fout) == run.text));
		if (!ok) break;
		run = next; rc = rc_next;
	}
	if (rc < 0) ok = false;
	if (fclose(fout) != 0) ok = false;
	if (!ok) { remove(out_path); return -1; }
	return 0;
}
#endif

}  // namespace

#ifndef MCOM_GZIP_HOST_ONLY
void mcom_gz_note_device_members(long n) { g_device_members = n; }
extern "C" long mcomh_test_gz_device_members(void) { return g_device_members; }

bool mcom_gz_device_route(const char *path, mcom_ctx *ctx, size_t piece_bytes, const mcom_gz_piece_fn &piece)
{
	g_device_members = 0;
	const uint64_t piece_text = piece_bytes < 64 ? 64 : piece_bytes;
	Feed F;
	DevBlocks B;
	if (!F.open(path, piece_text)) return false;
	// the text of a piece lies behind what the piece before left: an unfinished record, below one piece as long as pieces hold records
	const size_t text_cap = 2 * ((size_t)piece_text + 65536) + 16;
	uint8_t *d_text[2] = {nullptr, nullptr}, *d_status = nullptr;
	uint32_t *d_flag = nullptr;
	uint64_t *d_start = nullptr;
	size_t cap_lines = 0;
	if (!B.get(&d_text[0], text_cap + 16) || !B.get(&d_text[1], text_cap + 16) || !B.get(&d_status, F.max_members) || !B.get(&d_flag, 16)) return false;
	if (hipMemset(d_flag, 0, 16) != hipSuccess) return false;
	long members = 0;
	uint64_t carry = 0;
	int t = 0;
	Feed::Run run, next;
	int rc = F.stage(run);
	if (rc) return false;
	for (;;) {
		const int rc_next = F.stage(next);
		if (rc_next < 0) return false;
		const bool eof = rc_next == 1;
		if (carry + run.text + 1 > text_cap) return false;            // records that do not fit the pieces: the zlib route says so
		uint64_t bad = 0, first = 0;
		if (!F.wait(run) || mcom_gzip_inflate(ctx, F.d_comp[run.k], run.comp_bytes, F.d_tab[run.k], run.n_members, d_text[t] + carry, run.text, d_status, &bad, &first) != MCOM_OK || bad) return false;
		members += (long)run.n_members;
		uint64_t total = carry + run.text;
		if (eof && total) {                                            // a missing last newline is added on the card
			uint8_t lastc = 0;
			if (hipMemcpy(&lastc, d_text[t] + total - 1, 1, hipMemcpyDeviceToHost) != hipSuccess) return false;
			if (lastc != '\n') { if (hipMemset(d_text[t] + total, '\n', 1) != hipSuccess) return false; ++total; }
		}
		uint64_t lines = 0;
		if (total && mcom_decode_line_index(ctx, d_text[t], total, nullptr, 0, &lines, d_flag)) return false;
		const uint64_t records = lines / 4;
		if (records) {
			if (lines + 1 > cap_lines) {
				size_t want = cap_lines ? cap_lines : 4096;
				while (want < lines + 1) want *= 2;
				if (!B.get(&d_start, want * 8 + 16)) return false;     // (the smaller one stays with the call's blocks to its end)
				cap_lines = want;
			}
			uint64_t lines2 = 0, bytes = 0; uint32_t flag = 0;
			if (mcom_decode_line_index(ctx, d_text[t], total, d_start, lines, &lines2, d_flag) || lines2 != lines) return false;
			if (hipMemcpy(&bytes, d_start + 4 * records, 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&flag, d_flag, 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
			if (flag || bytes > total || (eof && bytes != total)) return false;
			if (!piece(d_text[t], bytes, records, d_start)) return false;
			carry = total - bytes;
			if (carry && hipMemcpy(d_text[t ^ 1], d_text[t] + bytes, (size_t)carry, hipMemcpyDeviceToDevice) != hipSuccess) return false;
			t ^= 1;
		} else {
			if (eof && total) return false;                            // the file ends inside a record
			carry = total;                                             // no whole record yet: the next piece's text goes behind it
		}
		if (eof) break;
		run = next;
	}
	g_device_members = members;
	return true;
}
#endif

extern "C" int mcomh_gzip_inflate_members(const uint8_t *in, uint64_t in_bytes, const mcomh_gzip_member *members, uint64_t n_members,
                                          uint8_t *out, uint64_t out_bytes, uint8_t *status, uint64_t *bad, uint64_t *first_bad)
{
	if (bad) *bad = 0;
	if (first_bad) *first_bad = n_members;
	if (!n_members) return 0;
	if (!members || (in_bytes && !in) || (out_bytes && !out)) return -1;
	return inflate_table(in, in_bytes, reinterpret_cast<const Member*>(members), n_members, out, out_bytes, status, bad, first_bad);
}

extern "C" int mcomh_gzip_inflate(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len)
{
	if (!out_len || (n && !in)) return -1;
	*out_len = 0;
	uint64_t nm = 0, text = 0, used = 0;
	if (!walk_members(in, n, nullptr, 0, &nm, &text, &used) || used != n) return -1;
	*out_len = text;
	if (text > cap) return -4;
	if (text && !out) return -1;
	try {
		std::vector<Member> tab((size_t)nm);
		std::vector<uint8_t> status((size_t)nm);
		walk_members(in, n, tab.data(), nm, &nm, &text, &used);
		uint64_t bad = 0, first = 0;
		if (inflate_table(in, n, tab.data(), nm, out, text, status.data(), &bad, &first)) return -1;
		return bad ? (int)status[(size_t)first] : 0;
	} catch (const std::bad_alloc &) { return -1; }
}

extern "C" int mcomh_gunzip_file(const char *in_path, const char *out_path, int device)
{
	if (!in_path || !out_path) return -1;
	if (device < 0) {
		try { return host_gunzip_file(in_path, out_path); } catch (const std::bad_alloc &) { return -1; }
	}
#ifndef MCOM_GZIP_HOST_ONLY
	return device_gunzip_file(in_path, out_path, device);
#else
	return -1;
#endif
}
