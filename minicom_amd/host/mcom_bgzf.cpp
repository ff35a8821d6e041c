// minicom_amd/host/mcom_bgzf.cpp -- BGZF output on the host: the twin of csrc/bgzf.hip.
// mcomh_bgzf_encode is a plain loop over csrc/deflate_model.hpp, which the kernels compile as well: the same hash, candidates, matches,
// codes and stored-or-dynamic decision, so the bytes equal the device's.  This half builds alone with -DMCOM_BGZF_HOST_ONLY
// (tests/fuzz_bgzf.cpp runs it under the sanitizers).  mcomh_bgzf_file with device >= 0 runs mcom_bgzf_encode on that GPU in pieces of
// whole blocks through two page-locked buffers each way, the write of piece i beside the copy of piece i + 1; device = -1 is the twin.
// A failed call leaves no output file.
#include "../../include/mcom_host.h"
#include "../csrc/deflate_model.hpp"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>
#ifndef MCOM_BGZF_HOST_ONLY
#include "../../include/mcom.h"
#include <hip/hip_runtime.h>
#endif

using namespace mcom_deflate;

namespace {

struct BitWriter {
	uint8_t *out; uint64_t acc = 0; uint32_t fill = 0; size_t at = 0;
	void operator()(uint32_t v, uint32_t bits) { put((uint64_t)v, bits); }
	void put(uint64_t v, uint32_t bits)
	{
		acc |= v << fill; fill += bits;                           // (bits <= 48 and fill < 8 on entry)
		while (fill >= 8) { out[at++] = (uint8_t)acc; acc >>= 8; fill -= 8; }
	}
	size_t finish() { if (fill) { out[at++] = (uint8_t)acc; acc = 0; fill = 0; } return at; }
};

struct BlockState {                                              // one encoder's scratch, reused from block to block
	std::vector<uint64_t> words = std::vector<uint64_t>(TEXT_WORDS);
	std::vector<uint32_t> table = std::vector<uint32_t>(HASH_SLOTS), tokens = std::vector<uint32_t>(MAX_TOKENS);
	uint32_t crc_table[256];
	Work work; Plan plan;
	BlockState() { for (uint32_t i = 0; i < 256; ++i) crc_table[i] = crc_table_entry(i); }
};

// one member from in[0 .. n), 1 <= n <= BLOCK, into out (room for n + MEMBER_EXTRA); returns its size
size_t encode_block(BlockState &S, const uint8_t *in, uint32_t n, uint8_t *out)
{
	uint64_t *w = S.words.data();
	memset(w, 0, sizeof(uint64_t) * TEXT_WORDS);
	for (uint32_t i = 0; i < n; ++i) w[i >> 3] |= (uint64_t)in[i] << ((i & 7) * 8);          // little-endian words whatever the host is
	std::fill(S.table.begin(), S.table.end(), 0u);
	uint32_t ll[N_LL] = {0}, dd[N_D] = {0};
	uint32_t ntok = 0, p = 0;
	for (uint32_t base = 0; base < n; base += TILE) {
		const uint32_t end = base + TILE < n ? base + TILE : n;
		while (p < end) {                                         // the greedy walk visits the positions that matter; the table is as it stood before the tile
			const Match m = find_match(w, n, p, p + 4 <= n ? S.table[hash4((uint32_t)load64(w, p))] : 0);
			if (m.len) {
				uint32_t s, eb, ev;
				len_symbol(m.len, s, eb, ev); ++ll[s];
				dist_symbol(m.dist, s, eb, ev); ++dd[s];
				S.tokens[ntok++] = match_token(m);
				p += m.len;
			} else {
				const uint32_t b = (uint32_t)(w[p >> 3] >> ((p & 7) * 8)) & 255;
				++ll[b];
				S.tokens[ntok++] = b;
				++p;
			}
		}
		for (uint32_t q = base; q < end && q + 4 <= n; ++q) {
			uint32_t &slot = S.table[hash4((uint32_t)load64(w, q))];
			if (slot < q + 1) slot = q + 1;
		}
	}
	S.tokens[ntok++] = EOB; ++ll[EOB];
	plan_block(ll, dd, n, &S.plan, &S.work);
	// CRC-32 as the device makes it: chunk CRCs joined by the combine step
	uint32_t crc = 0;
	for (uint32_t at = 0; at < n; at += CRC_CHUNK) {
		const uint32_t end = at + CRC_CHUNK < n ? at + CRC_CHUNK : n;
		const uint32_t c = crc_chunk(w, at, end, S.crc_table);
		crc = at ? crc_combine(crc, c, end - at) : c;
	}
	size_t payload;
	uint8_t *pay = out + HEADER_BYTES;
	if (S.plan.stored) {
		pay[0] = 1; pay[1] = (uint8_t)n; pay[2] = (uint8_t)(n >> 8); pay[3] = (uint8_t)~n; pay[4] = (uint8_t)(~n >> 8);
		memcpy(pay + STORED_BYTES, in, n);
		payload = STORED_BYTES + (size_t)n;
	} else {
		BitWriter bw; bw.out = pay;
		write_header(&S.plan, bw);
		for (uint32_t i = 0; i < ntok; ++i) {
			uint64_t bits; uint32_t nb;
			encode_token(&S.plan, S.tokens[i], bits, nb);
			bw.put(bits, nb);
		}
		payload = bw.finish();
	}
	const size_t size = HEADER_BYTES + payload + TRAILER_BYTES;
	for (uint32_t i = 0; i < HEADER_BYTES; ++i) out[i] = header_byte(i, (uint32_t)size);
	uint8_t *t = pay + payload;
	for (int i = 0; i < 4; ++i) { t[i] = (uint8_t)(crc >> (8 * i)); t[4 + i] = (uint8_t)(n >> (8 * i)); }
	return size;
}

int encode_buffer(BlockState &S, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len, int flags)
{
	uint8_t member[BLOCK + MEMBER_EXTRA + 8];
	uint64_t at = 0;
	for (uint64_t off = 0; off < n; off += BLOCK) {
		const uint32_t bn = (uint32_t)(n - off < BLOCK ? n - off : BLOCK);
		const size_t size = encode_block(S, in + off, bn, member);
		if (at + size > cap) return -4;
		memcpy(out + at, member, size);
		at += size;
	}
	if (flags & MCOMH_BGZF_EOF) {
		if (at + EOF_BYTES > cap) return -4;
		for (uint32_t i = 0; i < EOF_BYTES; ++i) out[at + i] = eof_byte(i);
		at += EOF_BYTES;
	}
	*out_len = at;
	return 0;
}

const size_t PIECE_BLOCKS = 1024;                                // 64 MB of text per piece
const size_t PIECE_BYTES = PIECE_BLOCKS * (size_t)BLOCK;

int host_file(const char *in_path, const char *out_path)
{
	FILE *fin = fopen(in_path, "rb");
	if (!fin) return -1;
	FILE *fout = fopen(out_path, "wb");
	if (!fout) { fclose(fin); return -1; }
	bool ok = true;
	{
		BlockState S;
		const size_t piece = 64 * (size_t)BLOCK;
		std::vector<uint8_t> in(piece), out((size_t)bound(piece));
		for (;;) {
			const size_t got = fread(in.data(), 1, piece, fin);
			if (ferror(fin)) { ok = false; break; }
			const bool last = got < piece;
			uint64_t len = 0;
			if (encode_buffer(S, in.data(), got, out.data(), out.size(), &len, last ? MCOMH_BGZF_EOF : 0) || fwrite(out.data(), 1, (size_t)len, fout) != len) { ok = false; break; }
			if (last) break;
		}
	}
	fclose(fin);
	if (fclose(fout) != 0) ok = false;
	if (!ok) { remove(out_path); return -1; }
	return 0;
}

#ifndef MCOM_BGZF_HOST_ONLY
struct DeviceJob {
	mcom_ctx *ctx = nullptr; hipStream_t stream = nullptr;
	uint8_t *d_in = nullptr, *d_out = nullptr, *pin_in[2] = {nullptr, nullptr}, *pin_out[2] = {nullptr, nullptr};
	hipEvent_t up[2] = {nullptr, nullptr}, down[2] = {nullptr, nullptr};
	FILE *fin = nullptr, *fout = nullptr;
	~DeviceJob()
	{
		if (stream) (void)hipStreamSynchronize(stream);
		if (fin) fclose(fin);
		if (fout) fclose(fout);
		if (ctx) mcom_destroy(ctx);
		if (d_in) (void)hipFree(d_in);
		if (d_out) (void)hipFree(d_out);
		for (int k = 0; k < 2; ++k) {
			if (pin_in[k]) (void)hipHostFree(pin_in[k]);
			if (pin_out[k]) (void)hipHostFree(pin_out[k]);
			if (up[k]) (void)hipEventDestroy(up[k]);
			if (down[k]) (void)hipEventDestroy(down[k]);
		}
		if (stream) (void)hipStreamDestroy(stream);
	}
};

int device_file(const char *in_path, const char *out_path, int device)
{
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev) return -1;      // no such GPU: an error, never the host twin
	if (hipSetDevice(device) != hipSuccess) return -1;
	DeviceJob J;
	J.fin = fopen(in_path, "rb");
	if (!J.fin) return -1;
	const size_t out_cap = (size_t)bound(PIECE_BYTES);
	if (hipStreamCreate(&J.stream) != hipSuccess || mcom_create(&J.ctx, device, (void*)J.stream) != MCOM_OK) return -1;
	for (int k = 0; k < 2; ++k)
		if (hipHostMalloc((void**)&J.pin_in[k], PIECE_BYTES, hipHostMallocDefault) != hipSuccess || hipHostMalloc((void**)&J.pin_out[k], out_cap, hipHostMallocDefault) != hipSuccess ||
		    hipEventCreateWithFlags(&J.up[k], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&J.down[k], hipEventDisableTiming) != hipSuccess) return -1;
	if (hipMalloc((void**)&J.d_in, PIECE_BYTES + 16) != hipSuccess || hipMalloc((void**)&J.d_out, 2 * out_cap + 16) != hipSuccess) return -1;
	J.fout = fopen(out_path, "wb");
	if (!J.fout) return -1;
	bool ok = true;
	uint64_t pending[2] = {0, 0};
	bool have[2] = {false, false};
	auto drain = [&](int k) {                                     // piece in pin_out[k]: wait for its copy, write it
		if (!have[k]) return true;
		have[k] = false;
		return hipEventSynchronize(J.down[k]) == hipSuccess && fwrite(J.pin_out[k], 1, (size_t)pending[k], J.fout) == pending[k];
	};
	for (uint64_t i = 0; ok; ++i) {
		const int k = (int)(i & 1);
		const size_t got = fread(J.pin_in[k], 1, PIECE_BYTES, J.fin);        // (pin_in[k] was last read by the copy of piece i - 2, which the encode of that piece waited for)
		if (ferror(J.fin)) { ok = false; break; }
		const bool last = got < PIECE_BYTES;
		uint64_t len = 0;
		ok = (!got || hipMemcpyAsync(J.d_in, J.pin_in[k], got, hipMemcpyHostToDevice, J.stream) == hipSuccess) && drain(k);
		if (!ok) break;
		uint8_t *d_o = J.d_out + (size_t)k * out_cap;
		if (mcom_bgzf_encode(J.ctx, J.d_in, got, d_o, out_cap, &len, last ? MCOM_BGZF_EOF : 0) != MCOM_OK) { fprintf(stderr, "mcom bgzf: %s\n", mcom_last_error(J.ctx)); ok = false; break; }
		if (len) ok = hipMemcpyAsync(J.pin_out[k], d_o, (size_t)len, hipMemcpyDeviceToHost, J.stream) == hipSuccess && hipEventRecord(J.down[k], J.stream) == hipSuccess;
		pending[k] = len; have[k] = ok && len;
		ok = ok && drain(k ^ 1);                                   // the write of piece i - 1 beside the copy of piece i
		if (last) break;
	}
	ok = ok && drain(0) && drain(1);
	if (hipStreamSynchronize(J.stream) != hipSuccess) ok = false;
	const bool closed = fclose(J.fout) == 0;
	J.fout = nullptr;
	if (!ok || !closed) { remove(out_path); return -1; }
	return 0;
}
#endif

}  // namespace

extern "C" uint64_t mcomh_bgzf_bound(uint64_t n) { return bound(n); }

extern "C" int mcomh_bgzf_encode(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len, int flags)
{
	if (!out || !out_len || (n && !in)) return -1;
	*out_len = 0;
	try {
		BlockState S;
		return encode_buffer(S, in, n, out, cap, out_len, flags);
	} catch (const std::bad_alloc &) { return -1; }
}

extern "C" int mcomh_bgzf_file(const char *in_path, const char *out_path, int device)
{
	if (!in_path || !out_path) return -1;
	if (device < 0) {
		try { return host_file(in_path, out_path); } catch (const std::bad_alloc &) { remove(out_path); return -1; }
	}
#ifndef MCOM_BGZF_HOST_ONLY
	return device_file(in_path, out_path, device);
#else
	return -1;
#endif
}
