// minicom_amd/host/mcom_entropy.cpp -- the built-in entropy stage on the host: the twin of csrc/entropy.hip and its specification, and
// the file forms behind bin/mcomz.
//
// mcomh_rans_encode / mcomh_rans_decode are plain C++ on host buffers -- no GPU, no HIP call: the same histograms, the same shared
// normalisation, choice and serialisation (csrc/rans_model.hpp), the same coder step, so the bytes equal the device's and the same
// members are refused.  This half builds alone with -DMCOM_ENTROPY_HOST_ONLY (tests/fuzz_entropy.cpp runs it under the sanitizers).
// (mcomh_bwt_pack_file / _unpack_file are the same file forms around the `.bwt` coder of host/mcom_bwt.cpp and csrc/bwt.hip.)
// mcomh_entropy_pack_file / _unpack_file with device >= 0 run mcom_rans_encode / _decode on that GPU: the file is read into two
// page-locked pieces that alternate between fread and the copy engine, the result comes back the same way, the copy of piece i + 1
// under the write of piece i.  device = -1 is the host twin.  A refused or failed member leaves no output file.
#include "../../include/mcom_host.h"
#include "../csrc/rans_model.hpp"
#include "../csrc/bwt_model.hpp"
#include "mcom_inflate.hpp"
#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>
#ifndef MCOM_ENTROPY_HOST_ONLY
#include "../../include/mcom.h"
#include <hip/hip_runtime.h>
#endif

using namespace mcom_rans;

namespace {

// one coding step, as rn_code of csrc/entropy.hip; bytes are written downwards from *wp
inline void code_symbol(uint32_t &x, uint8_t *&wp, const uint16_t *row, uint32_t sym)
{
	const uint32_t c = row[sym], f = row[sym + 1] - c;
	const uint32_t x_max = f << 19;
	while (x >= x_max) { *--wp = (uint8_t)x; x >>= 8; }
	x = ((x / f) << PROB_BITS) + (x % f) + c;
}

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
double g_times[8];          // ms of the last file call: [0] read (+ upload, overlapped) | [1] the codec call | [2] (download +) write | [3] whole call | [4] raw bytes | [5] coded bytes

}  // namespace

extern "C" uint64_t mcomh_rans_bound(uint64_t n)
{
	const uint64_t n_seg = (n + SEG - 1) >> SEG_LOG2;
	return HEADER_BYTES + (uint64_t)4 * 256 * (2 + 3 * 256) + n_seg * (2 + run_cap(SEG)) + 64;
}

extern "C" int mcomh_rans_estimate(const uint8_t *in, uint64_t n, uint64_t est7[7])
{
	if ((n && !in) || !est7) return -1;
	Hist h; Model m;
	hist_host(in, n, h);
	choose(h, n, 0, m, est7);
	return 0;
}

extern "C" int mcomh_rans_encode(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len, int model_hint)
{
	if (!out_len || !out || (n && !in)) return -1;
	*out_len = 0;
	if (cap < HEADER_BYTES) return -4;
	Hist h; Model m;
	hist_host(in, n, h);
	if (!choose(h, n, model_hint, m, nullptr)) return -1;
	Header hd; hd.raw_len = n; hd.model = (uint8_t)m.model; hd.stride = (uint8_t)m.stride; hd.table_bytes = (uint32_t)m.ser.size();
	hd.crc = n ? mcom_crc32(0, in, n) : 0;
	if (m.model == STORED) {
		if (cap < HEADER_BYTES + n) return -4;
		hd.payload_bytes = n;
		write_header(out, hd);
		if (n) memcpy(out + HEADER_BYTES, in, n);
		*out_len = HEADER_BYTES + n;
		return 0;
	}
	const uint64_t n_seg = (n + SEG - 1) >> SEG_LOG2;
	const size_t head = HEADER_BYTES + m.ser.size();
	if (cap < head + 2 * n_seg) return -4;
	uint8_t *lens = out + head, *runs = lens + 2 * n_seg, *const out_end = out + cap;
	const int nctx = m.n_ctx(), stride = m.stride;
	const bool o1 = m.model == ORDER1;
	std::vector<uint8_t> scratch(run_cap(SEG));
	uint64_t payload = 0;
	for (uint64_t seg = 0; seg < n_seg; ++seg) {
		const uint8_t *s = in + seg * SEG;
		const uint32_t len = n - seg * SEG < SEG ? (uint32_t)(n - seg * SEG) : SEG;
		uint8_t *const top = scratch.data() + scratch.size(), *wp = top;
		uint32_t x = STATE_L;
		for (uint32_t i = len; i-- > 0; ) {
			const uint32_t ctx = o1 && i >= (uint32_t)stride ? s[i - stride] : 0u;
			code_symbol(x, wp, &m.cum[((size_t)(i & (stride - 1)) * nctx + ctx) * ROW], s[i]);
		}
		*--wp = (uint8_t)(x >> 24); *--wp = (uint8_t)(x >> 16); *--wp = (uint8_t)(x >> 8); *--wp = (uint8_t)x;
		const size_t rl = (size_t)(top - wp);
		if ((uint64_t)(out_end - runs) < payload + rl) return -4;
		memcpy(runs + payload, wp, rl);
		put_u16(lens + 2 * seg, (uint32_t)rl);
		payload += rl;
	}
	hd.payload_bytes = payload;
	write_header(out, hd);
	if (!m.ser.empty()) memcpy(out + HEADER_BYTES, m.ser.data(), m.ser.size());
	*out_len = head + 2 * n_seg + payload;
	return 0;
}

// Accepts exactly what mcom_rans_decode accepts: the header describes the member to the byte, the tables are well formed, the run lengths
// add up to the payload, every run holds a state in [2^23, 2^31), every slot belongs to a symbol of its row, no run is read beyond its
// end, every run ends at its last byte with the state the encoder started from, and the CRC-32 of the result is the header's.
extern "C" int mcomh_rans_decode(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t cap, uint64_t *out_len)
{
	if (!out_len || (in_len && !in)) return -1;
	*out_len = 0;
	Header hd;
	if (!read_header(in, in_len, hd)) return -1;
	*out_len = hd.raw_len;
	if (hd.raw_len > cap) return -4;
	if (hd.raw_len && !out) return -1;
	if (hd.model == STORED) {
		if (hd.raw_len) memcpy(out, in + HEADER_BYTES, hd.raw_len);
	} else {
		std::vector<uint16_t> cum;
		if (!parse_tables(in + HEADER_BYTES, hd.table_bytes, hd.model, hd.stride, cum)) { *out_len = 0; return -1; }
		const uint64_t n_seg = hd.n_seg(), seg_bytes = (uint64_t)1 << hd.seg_log2;
		const uint8_t *lens = in + HEADER_BYTES + hd.table_bytes, *runs = lens + 2 * n_seg;
		uint64_t sum = 0;
		for (uint64_t s = 0; s < n_seg; ++s) sum += get_u16(lens + 2 * s);
		if (sum != hd.payload_bytes) { *out_len = 0; return -1; }
		const bool o1 = hd.model == ORDER1;
		const int stride = hd.stride, nctx = o1 ? 256 : 1;
		std::vector<uint8_t> slot_sym;                       // order-0: slot -> symbol per plane (the device keeps the same table in LDS)
		if (!o1) {
			slot_sym.assign((size_t)stride * PROB_M, 0);
			for (int pl = 0; pl < stride; ++pl) for (uint32_t s = 0; s < 256; ++s)
				for (uint32_t q = cum[(size_t)pl * ROW + s]; q < cum[(size_t)pl * ROW + s + 1]; ++q) slot_sym[(size_t)pl * PROB_M + q] = (uint8_t)s;
		}
		uint64_t at_run = 0;
		bool bad = false;
		for (uint64_t seg = 0; seg < n_seg && !bad; ++seg) {
			const uint32_t rl = get_u16(lens + 2 * seg);
			const uint8_t *p = runs + at_run, *const end = p + rl;
			at_run += rl;
			if (rl < 4) { bad = true; break; }
			uint32_t x = get_u32(p); p += 4;
			if (x < STATE_L || x >= (1u << 31)) { bad = true; break; }
			uint8_t *d = out + seg * seg_bytes;
			const uint32_t len = hd.raw_len - seg * seg_bytes < seg_bytes ? (uint32_t)(hd.raw_len - seg * seg_bytes) : (uint32_t)seg_bytes;
			for (uint32_t i = 0; i < len && !bad; ++i) {
				const uint32_t pl = i & (stride - 1), ctx = o1 && i >= (uint32_t)stride ? d[i - stride] : 0u;
				const uint16_t *row = &cum[((size_t)pl * nctx + ctx) * ROW];
				const uint32_t slot = x & (PROB_M - 1);
				uint32_t sym;
				if (o1) { sym = 0; for (int st = 128; st; st >>= 1) if (row[sym + st] <= slot) sym += st; }
				else sym = slot_sym[(size_t)pl * PROB_M + slot];
				const uint32_t c = row[sym], f = row[sym + 1] - c;
				if (slot - c >= f) { bad = true; break; }
				x = f * (x >> PROB_BITS) + slot - c;
				while (x < STATE_L) { if (p >= end) { bad = true; break; } x = (x << 8) | *p++; }
				d[i] = (uint8_t)sym;
			}
			if (!bad && (p != end || x != STATE_L)) bad = true;
		}
		if (bad) { *out_len = 0; return -1; }
	}
	if ((hd.raw_len ? mcom_crc32(0, out, hd.raw_len) : 0u) != hd.crc) { *out_len = 0; return -1; }
	return 0;
}

// ---- files -----------------------------------------------------------------------------------------------------------------------------
namespace {

bool file_size(FILE *f, uint64_t &n)
{
	if (fseeko(f, 0, SEEK_END)) return false;
	const off_t e = ftello(f);
	if (e < 0 || fseeko(f, 0, SEEK_SET)) return false;
	n = (uint64_t)e;
	return true;
}
bool write_all(const char *path, const uint8_t *p, uint64_t n)
{
	FILE *f = fopen(path, "wb");
	if (!f) return false;
	const bool ok = (!n || fwrite(p, 1, n, f) == n);
	if (fclose(f) || !ok) { remove(path); return false; }
	return true;
}

// bwt: the `.bwt` coder (section 3.8) instead of the `.rans` one
int host_file(const char *in_path, const char *out_path, bool pack, bool bwt)
{
	const double t0 = now_ms();
	FILE *f = fopen(in_path, "rb");
	uint64_t n = 0;
	if (!f || !file_size(f, n)) { if (f) fclose(f); return -1; }
	std::vector<uint8_t> in(n);
	const bool got = !n || fread(in.data(), 1, n, f) == n;
	fclose(f);
	if (!got) return -1;
	const double t1 = now_ms();
	std::vector<uint8_t> out;
	uint64_t out_len = 0;
	int rc;
	if (pack && bwt) { out.resize(mcomh_bwt_bound(n)); rc = mcomh_bwt_encode(in.data(), n, out.data(), out.size(), &out_len); }
	else if (pack) { out.resize(mcomh_rans_bound(n)); rc = mcomh_rans_encode(in.data(), n, out.data(), out.size(), &out_len, 0); }
	else if (bwt) {
		mcom_bwt::Header bh;
		if (!mcom_bwt::read_header(in.data(), n, bh)) return -1;
		out.resize(bh.raw_len);
		rc = mcomh_bwt_decode(in.data(), n, out.data(), out.size(), &out_len);
	} else {
		Header hd;
		if (!read_header(in.data(), n, hd) || hd.raw_len > ((uint64_t)1 << 40)) return -1;
		out.resize(hd.raw_len);
		rc = mcomh_rans_decode(in.data(), n, out.data(), out.size(), &out_len);
	}
	const double t2 = now_ms();
	if (rc) return -1;
	if (!write_all(out_path, out.data(), out_len)) return -1;
	const double t3 = now_ms();
	g_times[0] = t1 - t0; g_times[1] = t2 - t1; g_times[2] = t3 - t2; g_times[3] = t3 - t0;
	g_times[4] = (double)(pack ? n : out_len); g_times[5] = (double)(pack ? out_len : n);
	return 0;
}

#ifndef MCOM_ENTROPY_HOST_ONLY
const size_t PIECE_BYTES = (size_t)32 << 20;

struct DeviceJob {                                           // what one file call holds on the card and in page-locked memory
	mcom_ctx *ctx = nullptr; hipStream_t stream = nullptr;
	uint8_t *d_in = nullptr, *d_out = nullptr, *pin[2] = {nullptr, nullptr};
	hipEvent_t ev[2] = {nullptr, nullptr};
	FILE *fin = nullptr, *fout = nullptr;
	~DeviceJob()
	{
		if (stream) (void)hipStreamSynchronize(stream);
		if (fin) fclose(fin);
		if (fout) fclose(fout);
		if (ctx) mcom_destroy(ctx);
		if (d_in) (void)hipFree(d_in);
		if (d_out) (void)hipFree(d_out);
		for (int k = 0; k < 2; ++k) { if (pin[k]) (void)hipHostFree(pin[k]); if (ev[k]) (void)hipEventDestroy(ev[k]); }
		if (stream) (void)hipStreamDestroy(stream);
	}
};

int device_file(const char *in_path, const char *out_path, bool pack, int device, bool bwt)
{
	const double t0 = now_ms();
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev) return -1;      // no such GPU: an error, never the host twin
	if (hipSetDevice(device) != hipSuccess) return -1;
	DeviceJob J;
	uint64_t n = 0;
	J.fin = fopen(in_path, "rb");
	if (!J.fin || !file_size(J.fin, n)) return -1;
	if (hipStreamCreate(&J.stream) != hipSuccess || mcom_create(&J.ctx, device, (void*)J.stream) != MCOM_OK) return -1;
	for (int k = 0; k < 2; ++k)
		if (hipHostMalloc((void**)&J.pin[k], PIECE_BYTES, hipHostMallocDefault) != hipSuccess || hipEventCreateWithFlags(&J.ev[k], hipEventDisableTiming) != hipSuccess) return -1;
	if (hipMalloc((void**)&J.d_in, n + 16) != hipSuccess) return -1;
	// the file up: fread of piece i + 1 beside the copy of piece i
	Header hd;
	mcom_bwt::Header bh;
	bool header_ok = pack;
	for (uint64_t at = 0, i = 0; at < n; at += PIECE_BYTES, ++i) {
		const int k = (int)(i & 1);
		const size_t piece = n - at < PIECE_BYTES ? (size_t)(n - at) : PIECE_BYTES;
		if (i >= 2 && hipEventSynchronize(J.ev[k]) != hipSuccess) return -1;
		if (fread(J.pin[k], 1, piece, J.fin) != piece) return -1;
		if (!pack && at == 0) header_ok = bwt ? mcom_bwt::read_header(J.pin[k], n, bh) : read_header(J.pin[k], n, hd);             // sizes are judged before anything is launched
		if (!header_ok) return -1;
		if (hipMemcpyAsync(J.d_in + at, J.pin[k], piece, hipMemcpyHostToDevice, J.stream) != hipSuccess || hipEventRecord(J.ev[k], J.stream) != hipSuccess) return -1;
	}
	if (!header_ok || hipStreamSynchronize(J.stream) != hipSuccess) return -1;
	const double t1 = now_ms();
	const uint64_t cap = pack ? (bwt ? mcom_bwt::HEADER_BYTES : 0) + HEADER_BYTES + n : bwt ? bh.raw_len : hd.raw_len;                      // (the chosen model never needs more than stored)
	if (!pack && cap > ((uint64_t)1 << 40)) return -1;
	if (hipMalloc((void**)&J.d_out, cap + 16) != hipSuccess) return -1;
	uint64_t out_len = 0;
	const int rc = bwt ? (pack ? mcom_bwt_encode(J.ctx, J.d_in, n, J.d_out, cap, &out_len) : mcom_bwt_decode(J.ctx, J.d_in, n, J.d_out, cap, &out_len))
	                   : (pack ? mcom_rans_encode(J.ctx, J.d_in, n, J.d_out, cap, &out_len, 0) : mcom_rans_decode(J.ctx, J.d_in, n, J.d_out, cap, &out_len));
	if (rc) { fprintf(stderr, "mcom entropy stage: %s\n", mcom_last_error(J.ctx)); return -1; }
	const double t2 = now_ms();
	// the result down: the copy of piece i + 1 under the write of piece i
	J.fout = fopen(out_path, "wb");
	if (!J.fout) return -1;
	bool ok = true;
	const uint64_t pieces = (out_len + PIECE_BYTES - 1) / PIECE_BYTES;
	auto piece_len = [&](uint64_t i) { return (size_t)(out_len - i * PIECE_BYTES < PIECE_BYTES ? out_len - i * PIECE_BYTES : PIECE_BYTES); };
	if (pieces) ok = hipMemcpyAsync(J.pin[0], J.d_out, piece_len(0), hipMemcpyDeviceToHost, J.stream) == hipSuccess && hipEventRecord(J.ev[0], J.stream) == hipSuccess;
	for (uint64_t i = 0; ok && i < pieces; ++i) {
		const int k = (int)(i & 1);
		if (i + 1 < pieces) ok = hipMemcpyAsync(J.pin[k ^ 1], J.d_out + (i + 1) * PIECE_BYTES, piece_len(i + 1), hipMemcpyDeviceToHost, J.stream) == hipSuccess &&
		                         hipEventRecord(J.ev[k ^ 1], J.stream) == hipSuccess;
		ok = ok && hipEventSynchronize(J.ev[k]) == hipSuccess && fwrite(J.pin[k], 1, piece_len(i), J.fout) == piece_len(i);
	}
	const bool closed = fclose(J.fout) == 0;
	J.fout = nullptr;
	if (!ok || !closed) { remove(out_path); return -1; }
	const double t3 = now_ms();
	g_times[0] = t1 - t0; g_times[1] = t2 - t1; g_times[2] = t3 - t2; g_times[3] = t3 - t0;
	g_times[4] = (double)(pack ? n : out_len); g_times[5] = (double)(pack ? out_len : n);
	return 0;
}
#endif

int file_call(const char *in_path, const char *out_path, int device, bool pack, bool bwt = false)
{
	if (!in_path || !out_path) return -1;
	memset(g_times, 0, sizeof g_times);
	if (device < 0) {
		try { return host_file(in_path, out_path, pack, bwt); } catch (const std::bad_alloc &) { return -1; }      // (a header that asks for more than there is)
	}
#ifndef MCOM_ENTROPY_HOST_ONLY
	return device_file(in_path, out_path, pack, device, bwt);
#else
	return -1;
#endif
}

}  // namespace

extern "C" int mcomh_entropy_pack_file(const char *in_path, const char *out_path, int device) { return file_call(in_path, out_path, device, true); }
extern "C" int mcomh_entropy_unpack_file(const char *in_path, const char *out_path, int device) { return file_call(in_path, out_path, device, false); }
extern "C" void mcomh_entropy_times(double *ms8) { memcpy(ms8, g_times, sizeof g_times); }
extern "C" int mcomh_bwt_pack_file(const char *in_path, const char *out_path, int device) { return file_call(in_path, out_path, device, true, true); }
extern "C" int mcomh_bwt_unpack_file(const char *in_path, const char *out_path, int device) { return file_call(in_path, out_path, device, false, true); }
