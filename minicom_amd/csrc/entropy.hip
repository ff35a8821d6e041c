// minicom_amd/csrc/entropy.hip -- the built-in entropy stage: a static rANS coder with order-0 / order-1 models per byte plane
// (format, normalisation, model choice: rans_model.hpp; specification and cross-check: host/mcom_entropy.cpp).
//
//   k_rans_hist     one pass over the member, 16 bytes per thread and step: the order-0 counts of the four byte positions i mod 4 in LDS
//                   (4 KB, flushed once per workgroup), the order-1 counts of stride 1, 2 and 4 -- seven planes of 256 x 256 -- by 64-bit
//                   atomics on one 3.5 MB table in global memory.  A plane of u32 alone would be 256 KB against 160 KB of LDS; slicing the
//                   contexts would read the member four times or more, the table stays in L2 (4 MB) beside a streaming read, so: atomics.
//   k_rans_crc      CRC-32 per segment (one lane per segment, table in LDS); the host joins them (CrcShift)
//   k_rans_encode   one lane per segment, walking it backwards 16 bytes at a time; coded bytes go, last byte first, into the lane's own
//                   scratch run, four at a time; the run's length into lens[]
//   (mcom_scan64)   run offsets
//   k_rans_compact  a wave copies 16 runs to their final places and writes their u16 lengths
//   k_rans_lens     decode: the u16 lengths (at any byte offset) -> u64 for the scan
//   k_rans_decode   one lane per segment.  Order-0: slot -> symbol and the cumulative rows in LDS; order-1: the cumulative row of the
//                   context is bisected in global memory (4 planes x 256 rows x 514 bytes = 526 KB, L2; a direct slot table per context
//                   would be 4 MB per member and push the coded bytes out of L2).  64 decoded bytes per lane are staged in LDS, then
//                   every group of four lanes stores one segment's 64 bytes as four aligned 16-byte pieces.
// Untrusted input (the rule of section 3.5): sizes are checked on the host before a kernel runs (read_header, parse_tables, the sum of
// the run lengths); inside the kernels a run is never read beyond its end, a slot that no symbol of the row owns, a state outside
// [2^23, 2^31) and a run that does not end where and how it must raise the flag word and skip the access.
#include "mcom_dev.hpp"
#include "rans_model.hpp"

using namespace mcom_rans;

#define RN_THREADS 256
#define RN_STAGE_PITCH 80                      // bytes of LDS per lane in the decoder's staging area: 64 + 16, so that b128 accesses of neighbouring lanes spread over the banks
enum { RN_F_RUN = 1, RN_F_SLOT = 2, RN_F_STATE = 4, RN_F_END = 8, RN_F_FREQ = 16, RN_F_ROOM = 32 };

__device__ __forceinline__ uint32_t rn_byte(const uint32_t (&w)[4], int k) { return (w[k >> 2] >> ((k & 3) * 8)) & 0xFFu; }

// 16 bytes (valid < 16: the first `valid`, the rest 0); vec: p is 16-byte aligned
__device__ __forceinline__ void rn_ld16(const uint8_t *p, uint32_t valid, bool vec, uint32_t (&w)[4])
{
	if (vec && valid == 16) { const uint4 q = *(const uint4*)p; w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w; return; }
	w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
	for (int k = 0; k < 16; ++k) if ((uint32_t)k < valid) w[k >> 2] |= (uint32_t)p[k] << ((k & 3) * 8);
}

__global__ __launch_bounds__(RN_THREADS) void k_rans_hist(const uint8_t *__restrict__ in, uint64_t n, unsigned long long *__restrict__ o0,
                                                          unsigned long long *__restrict__ o1, int vec)
{
	__shared__ uint32_t s0[4 * 256];
	for (int t = threadIdx.x; t < 4 * 256; t += RN_THREADS) s0[t] = 0;
	__syncthreads();
	const uint64_t chunks = (n + 15) / 16;
	for (uint64_t c = (uint64_t)blockIdx.x * RN_THREADS + threadIdx.x; c < chunks; c += (uint64_t)gridDim.x * RN_THREADS) {
		const uint64_t base = c * 16;
		const uint32_t valid = n - base < 16 ? (uint32_t)(n - base) : 16u;
		uint32_t w[4], before = 0;
		rn_ld16(in + base, valid, vec != 0, w);
		if (base & (SEG - 1)) { const uint8_t *q = in + base - 4; before = q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24; }   // (0 at a segment's start: context 0)
#pragma unroll
		for (int k = 0; k < 16; ++k) {
			if ((uint32_t)k >= valid) continue;
			const uint32_t b = rn_byte(w, k);
			const uint32_t c1 = k >= 1 ? rn_byte(w, k >= 1 ? k - 1 : 0) : before >> 24;
			const uint32_t c2 = k >= 2 ? rn_byte(w, k >= 2 ? k - 2 : 0) : (before >> (16 + 8 * k)) & 0xFFu;
			const uint32_t c4 = k >= 4 ? rn_byte(w, k >= 4 ? k - 4 : 0) : (before >> (8 * k)) & 0xFFu;
			atomicAdd(&s0[(k & 3) * 256 + b], 1u);
			atomicAdd(&o1[(size_t)c1 * 256 + b], 1ull);
			atomicAdd(&o1[(size_t)(1 + (k & 1)) * 65536 + c2 * 256 + b], 1ull);
			atomicAdd(&o1[(size_t)(3 + (k & 3)) * 65536 + c4 * 256 + b], 1ull);
		}
	}
	__syncthreads();
	for (int t = threadIdx.x; t < 4 * 256; t += RN_THREADS) if (s0[t]) atomicAdd(&o0[t], (unsigned long long)s0[t]);
}

__global__ __launch_bounds__(RN_THREADS) void k_rans_crc(const uint8_t *__restrict__ in, uint64_t n, uint64_t n_seg, uint32_t seg_log2, uint32_t *__restrict__ crc_out, int vec)
{
	__shared__ uint32_t tab[256];
	{ uint32_t c = threadIdx.x; for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u))); tab[threadIdx.x] = c; }
	__syncthreads();
	const uint64_t seg = (uint64_t)blockIdx.x * RN_THREADS + threadIdx.x;
	if (seg >= n_seg) return;
	const uint64_t at = seg << seg_log2;
	const uint32_t len = n - at < ((uint64_t)1 << seg_log2) ? (uint32_t)(n - at) : 1u << seg_log2;
	uint32_t crc = 0xFFFFFFFFu;
	for (uint32_t i = 0; i < len; i += 16) {
		uint32_t w[4];
		const uint32_t valid = len - i < 16 ? len - i : 16u;
		rn_ld16(in + at + i, valid, vec != 0, w);
#pragma unroll
		for (int k = 0; k < 16; ++k) if ((uint32_t)k < valid) crc = tab[(crc ^ rn_byte(w, k)) & 0xFFu] ^ (crc >> 8);
	}
	crc_out[seg] = ~crc;
}

// the coded bytes of one lane: written from the top of its scratch run downwards, the byte emitted first at the highest address
struct RnEmit {
	uint8_t *wp, *bottom; uint32_t acc = 0, nacc = 0; bool full = false;
	__device__ __forceinline__ void put(uint32_t b)
	{
		acc = (acc << 8) | (b & 0xFFu);
		if (++nacc == 4) {
			if (wp - 4 < bottom) full = true; else { wp -= 4; *(uint32_t*)wp = acc; }
			nacc = 0;
		}
	}
	__device__ __forceinline__ void finish()
	{
		for (uint32_t j = 0; j < nacc; ++j) { if (wp - 1 < bottom) { full = true; break; } *--wp = (uint8_t)(acc >> ((nacc - 1 - j) * 8)); }
		nacc = 0;
	}
};

__device__ __forceinline__ void rn_code(uint32_t &x, RnEmit &e, const uint16_t *row, uint32_t sym, bool &bad)
{
	const uint32_t c = row[sym], f = row[sym + 1] - c;
	if (f == 0 || f > PROB_M) { bad = true; return; }                      // (a symbol the tables do not hold: they were made from other data)
	const uint32_t x_max = f << 19;                                        // ((STATE_L >> PROB_BITS) << 8) * f
	while (x >= x_max) { e.put(x); x >>= 8; }
	x = ((x / f) << PROB_BITS) + (x % f) + c;
}

template <int O1, int STRIDE>
__global__ __launch_bounds__(RN_THREADS) void k_rans_encode(const uint8_t *__restrict__ in, uint64_t n, uint64_t n_seg, const uint16_t *__restrict__ cum,
                                                            uint8_t *__restrict__ scratch, uint64_t *__restrict__ lens, uint32_t *__restrict__ flag, int vec)
{
	constexpr int NCTX = O1 ? 256 : 1;
	__shared__ uint16_t s_cum[O1 ? 2 : STRIDE * ROW];
	if (!O1) { for (int t = threadIdx.x; t < STRIDE * (int)ROW; t += RN_THREADS) s_cum[t] = cum[t]; __syncthreads(); }
	const uint16_t *tab = O1 ? cum : (const uint16_t*)s_cum;
	const uint64_t seg = (uint64_t)blockIdx.x * RN_THREADS + threadIdx.x;
	if (seg >= n_seg) return;
	const uint8_t *s = in + seg * SEG;
	const uint32_t len = n - seg * SEG < SEG ? (uint32_t)(n - seg * SEG) : SEG;
	const size_t cap = run_cap(SEG);
	RnEmit e; e.bottom = scratch + seg * cap; e.wp = e.bottom + cap;
	uint8_t *const top = e.wp;
	uint32_t x = STATE_L;
	bool bad = false;
	const uint32_t len16 = len & ~15u;
	for (uint32_t i = len; i-- > len16; ) {                                 // the bytes behind the last whole 16 (the member's last segment only)
		const uint32_t ctx = O1 && i >= (uint32_t)STRIDE ? s[i - STRIDE] : 0u;
		rn_code(x, e, tab + ((size_t)(i & (STRIDE - 1)) * NCTX + ctx) * ROW, s[i], bad);
	}
	uint32_t cur[4] = {0, 0, 0, 0}, prev[4];
	if (len16) rn_ld16(s + len16 - 16, 16, vec != 0, cur);
	for (uint32_t j = len16 / 16; j-- > 0; ) {
		prev[0] = prev[1] = prev[2] = prev[3] = 0;
		if (j) rn_ld16(s + 16 * (j - 1), 16, vec != 0, prev);
#pragma unroll
		for (int k = 15; k >= 0; --k) {
			const uint32_t ctx = !O1 ? 0u : k >= STRIDE ? rn_byte(cur, k >= STRIDE ? k - STRIDE : 0) : rn_byte(prev, k < STRIDE ? 16 + k - STRIDE : 0);
			rn_code(x, e, tab + ((size_t)(k & (STRIDE - 1)) * NCTX + ctx) * ROW, rn_byte(cur, k), bad);
		}
		cur[0] = prev[0]; cur[1] = prev[1]; cur[2] = prev[2]; cur[3] = prev[3];
	}
	e.put(x >> 24); e.put(x >> 16); e.put(x >> 8); e.put(x);
	e.finish();
	if (bad) atomicOr(flag, (uint32_t)RN_F_FREQ);
	if (e.full) atomicOr(flag, (uint32_t)RN_F_ROOM);
	lens[seg] = (uint64_t)(top - e.wp);
}

__global__ __launch_bounds__(RN_THREADS) void k_rans_compact(const uint8_t *__restrict__ scratch, const uint64_t *__restrict__ lens, const uint64_t *__restrict__ off,
                                                             uint64_t n_seg, uint8_t *__restrict__ out_lens, uint8_t *__restrict__ out_runs)
{
	const uint64_t wave = ((uint64_t)blockIdx.x * RN_THREADS + threadIdx.x) >> 6;
	const uint32_t lane = threadIdx.x & 63;
	const size_t cap = run_cap(SEG);
	for (uint64_t seg = wave * 16; seg < wave * 16 + 16 && seg < n_seg; ++seg) {
		const uint64_t len = lens[seg];
		if (len > cap) continue;                                            // (cannot be: the encoder never leaves its run)
		const uint8_t *src = scratch + (seg + 1) * cap - len;
		uint8_t *dst = out_runs + off[seg];
		for (uint64_t j = lane; j < len; j += 64) dst[j] = src[j];
		if (lane == 0) { out_lens[2 * seg] = (uint8_t)len; out_lens[2 * seg + 1] = (uint8_t)(len >> 8); }
	}
}

// lens64[seg] = the u16 at lens16 + 2 seg; lens64[n_seg] = 0, so that the exclusive scan ends with the total
__global__ __launch_bounds__(RN_THREADS) void k_rans_lens(const uint8_t *__restrict__ lens16, uint64_t n_seg, uint64_t *__restrict__ lens64)
{
	const uint64_t seg = (uint64_t)blockIdx.x * RN_THREADS + threadIdx.x;
	if (seg > n_seg) return;
	lens64[seg] = seg < n_seg ? (uint64_t)(lens16[2 * seg] | (uint32_t)lens16[2 * seg + 1] << 8) : 0ull;
}

template <int O1, int STRIDE>
__global__ __launch_bounds__(RN_THREADS) void k_rans_decode(const uint8_t *__restrict__ runs, const uint64_t *__restrict__ off, uint64_t payload_bytes,
                                                            const uint16_t *__restrict__ cum, uint8_t *__restrict__ out, uint64_t raw_len, uint64_t n_seg,
                                                            uint32_t seg_log2, uint32_t *__restrict__ flag, int vec)
{
	__shared__ __attribute__((aligned(16))) uint8_t stage[RN_THREADS * RN_STAGE_PITCH];
	__shared__ uint16_t s_cum[O1 ? 2 : STRIDE * ROW];
	__shared__ uint8_t s_sym[O1 ? 4 : STRIDE * PROB_M];
	if (!O1) {
		for (int t = threadIdx.x; t < STRIDE * (int)ROW; t += RN_THREADS) s_cum[t] = cum[t];
		__syncthreads();
		for (int t = threadIdx.x; t < STRIDE * (int)PROB_M; t += RN_THREADS) {
			const uint16_t *row = s_cum + (t >> PROB_BITS) * ROW; const uint32_t slot = t & (PROB_M - 1);
			uint32_t lo = 0;
#pragma unroll
			for (int st = 128; st; st >>= 1) if (row[lo + st] <= slot) lo += st;
			s_sym[t] = (uint8_t)lo;
		}
		__syncthreads();
	}
	const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const uint64_t seg = (uint64_t)blockIdx.x * RN_THREADS + threadIdx.x, wave_seg0 = seg - lane;
	const uint64_t seg_bytes = (uint64_t)1 << seg_log2;
	uint32_t len = 0, x = 0, bad = 0;
	const uint8_t *p = runs, *end = runs;
	if (seg < n_seg) {
		const uint64_t a = off[seg], b = off[seg + 1];
		const uint64_t at = seg << seg_log2;
		len = raw_len - at < seg_bytes ? (uint32_t)(raw_len - at) : (uint32_t)seg_bytes;
		if (b < a || b > payload_bytes || b - a < 4) bad = RN_F_RUN;
		else {
			p = runs + a; end = runs + b;
			x = p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; p += 4;
			if (x < STATE_L || x >= (1u << 31)) bad = RN_F_STATE;
		}
	}
	if (bad) len = 0;
	uint8_t *const my_stage = stage + (size_t)threadIdx.x * RN_STAGE_PITCH;
	const uint8_t *const wave_stage = stage + (size_t)wv * 64 * RN_STAGE_PITCH;
	uint32_t last = 0, done = 0;                                            // last: the four bytes decoded before this chunk
	const uint32_t rounds = 1u << (seg_log2 - 6);
	for (uint32_t r = 0; r < rounds; ++r) {
#pragma unroll 1
		for (int q = 0; q < 4; ++q) {
			uint32_t w[4] = {0, 0, 0, 0};
			const uint32_t valid = bad ? 0u : len - done < 16 ? len - done : 16u;
#pragma unroll
			for (int k = 0; k < 16; ++k) {
				if ((uint32_t)k < valid && !bad) {
					const uint32_t ctx = !O1 ? 0u : k >= STRIDE ? rn_byte(w, k >= STRIDE ? k - STRIDE : 0) : (last >> (8 * (k < STRIDE ? 4 + k - STRIDE : 0))) & 0xFFu;
					const uint32_t slot = x & (PROB_M - 1);
					uint32_t sym, c, f;
					if (O1) {
						const uint16_t *row = cum + ((size_t)(k & (STRIDE - 1)) * 256 + ctx) * ROW;
						uint32_t lo = 0;
#pragma unroll
						for (int st = 128; st; st >>= 1) if (row[lo + st] <= slot) lo += st;
						sym = lo; c = row[lo]; f = row[lo + 1] - c;
					} else {
						const uint32_t pl = k & (STRIDE - 1);
						sym = s_sym[pl * PROB_M + slot]; c = s_cum[pl * ROW + sym]; f = s_cum[pl * ROW + sym + 1] - c;
					}
					if (slot - c >= f) bad = RN_F_SLOT;                     // no symbol of this row owns the slot (an empty row: f = 0)
					else {
						x = f * (x >> PROB_BITS) + slot - c;
						while (x < STATE_L && !bad) {
							if (p >= end) bad = RN_F_RUN;                   // the run is used up: nothing is read
							else x = (x << 8) | *p++;
						}
						w[k >> 2] |= sym << ((k & 3) * 8);
					}
				}
			}
			done += valid;
			last = w[3];
			*(uint4*)(my_stage + q * 16) = make_uint4(w[0], w[1], w[2], w[3]);
		}
		__syncthreads();
		// 64 bytes of 64 segments: four lanes store one segment's, 16 segments per step
#pragma unroll
		for (int it = 0; it < 4; ++it) {
			const uint32_t sseg = it * 16 + (lane >> 2), piece = lane & 3;
			const uint64_t gseg = wave_seg0 + sseg;
			if (gseg >= n_seg) continue;
			const uint64_t goff = (gseg << seg_log2) + (uint64_t)r * 64 + piece * 16;
			if (goff >= raw_len) continue;
			const uint4 v = *(const uint4*)(wave_stage + (size_t)sseg * RN_STAGE_PITCH + piece * 16);
			if (vec && goff + 16 <= raw_len) *(uint4*)(out + goff) = v;
			else {
				const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
				for (int k = 0; k < 16; ++k) if (goff + k < raw_len) out[goff + k] = (uint8_t)rn_byte(vv, k);
			}
		}
		__syncthreads();
	}
	if (seg < n_seg && !bad && (p != end || x != STATE_L)) bad = RN_F_END;
	if (bad) atomicOr(flag, bad);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
extern "C" uint64_t mcom_rans_bound(uint64_t n)
{
	const uint64_t n_seg = (n + SEG - 1) >> SEG_LOG2;
	return HEADER_BYTES + (uint64_t)4 * 256 * (2 + 3 * 256) + n_seg * (2 + run_cap(SEG)) + 64;
}

namespace {
struct Blocks {                                             // pooled device blocks of one call, back to the pool once the stream has passed them
	mcom_ctx *ctx; std::vector<void*> v;
	explicit Blocks(mcom_ctx *c) : ctx(c) {}
	~Blocks() { for (void *p : v) mcom_dfree_later(ctx, p); }
	template <class T> hipError_t get(T **out, size_t bytes) { hipError_t e = mcom_dmalloc((void**)out, bytes ? bytes : 16); if (e == hipSuccess) v.push_back(*out); return e; }
};
unsigned blocks_for(uint64_t items) { return (unsigned)((items + RN_THREADS - 1) / RN_THREADS); }

// The two launches whose results stay inside the library, each in ONE place: the codec calls below and the hooks of include/mcom_test.h
// go through these, so a hook cannot test a launch (grid, `vec`, cleared table) that the product does not make.
// d_hist: 4 * 256 + 7 * 65536 u64, cleared here; n > 0
int launch_hist(mcom_ctx *ctx, const uint8_t *d_in, uint64_t n, unsigned long long *d_hist)
{
	const size_t hist_words = 4 * 256 + (size_t)N_PLANES_ALL * 65536;
	const int vec = ((uintptr_t)d_in & 15) == 0;
	MCOM_HIP(ctx, hipMemsetAsync(d_hist, 0, hist_words * 8, ctx->stream));
	uint64_t g = (n + 16 * RN_THREADS - 1) / (16 * RN_THREADS), gmax = (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 64) * 8;
	if (g > gmax) g = gmax;
	MCOM_LAUNCH(k_rans_hist, dim3((unsigned)g), dim3(RN_THREADS), 0, ctx->stream, d_in, n, d_hist, d_hist + 4 * 256, vec);
	MCOM_LAUNCH_CHECK(ctx);
	return MCOM_OK;
}
// d_crc: one u32 per segment of 2^seg_log2 bytes; n > 0
int launch_seg_crc(mcom_ctx *ctx, const uint8_t *d, uint64_t n, uint32_t seg_log2, uint32_t *d_crc)
{
	const uint64_t n_seg = (n + ((uint64_t)1 << seg_log2) - 1) >> seg_log2;
	const int vec = ((uintptr_t)d & 15) == 0;
	MCOM_LAUNCH(k_rans_crc, dim3(blocks_for(n_seg)), dim3(RN_THREADS), 0, ctx->stream, d, n, n_seg, seg_log2, d_crc, vec);
	MCOM_LAUNCH_CHECK(ctx);
	return MCOM_OK;
}

int device_crc(mcom_ctx *ctx, Blocks &B, const uint8_t *d, uint64_t n, uint32_t seg_log2, uint32_t *crc_out)
{
	*crc_out = 0;
	if (!n) return MCOM_OK;
	const uint64_t seg_bytes = (uint64_t)1 << seg_log2, n_seg = (n + seg_bytes - 1) >> seg_log2;
	uint32_t *d_crc = nullptr;
	MCOM_HIP(ctx, B.get(&d_crc, n_seg * 4));
	int rc = launch_seg_crc(ctx, d, n, seg_log2, d_crc);
	if (rc) return rc;
	std::vector<uint32_t> h(n_seg);
	MCOM_HIP(ctx, hipMemcpyAsync(h.data(), d_crc, n_seg * 4, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	const CrcShift whole(seg_bytes);
	uint32_t crc = 0;
	for (uint64_t s = 0; s + 1 < n_seg; ++s) crc = whole.join(crc, h[s]);
	*crc_out = CrcShift(n - (n_seg - 1) * seg_bytes).join(crc, h[n_seg - 1]);
	return MCOM_OK;
}
}  // namespace

// the CRC-32 of n bytes on the device, for the other coders of the library (bwt.hip): segment CRCs joined on the host, as the codec's own
int mcom_device_crc32(mcom_ctx *ctx, const uint8_t *d, uint64_t n, uint32_t *crc_out)
{
	Blocks B(ctx);
	return device_crc(ctx, B, d, n, SEG_LOG2, crc_out);
}

template <int O1, int STRIDE>
static void launch_encode(mcom_ctx *ctx, const uint8_t *d_in, uint64_t n, uint64_t n_seg, const uint16_t *d_cum, uint8_t *scratch, uint64_t *lens, uint32_t *flag, int vec)
{
	MCOM_LAUNCH((k_rans_encode<O1, STRIDE>), dim3(blocks_for(n_seg)), dim3(RN_THREADS), 0, ctx->stream, d_in, n, n_seg, d_cum, scratch, lens, flag, vec);
}
template <int O1, int STRIDE>
static void launch_decode(mcom_ctx *ctx, const uint8_t *runs, const uint64_t *off, uint64_t payload, const uint16_t *d_cum, uint8_t *out, uint64_t raw_len, uint64_t n_seg,
                          uint32_t seg_log2, uint32_t *flag, int vec)
{
	MCOM_LAUNCH((k_rans_decode<O1, STRIDE>), dim3(blocks_for(n_seg)), dim3(RN_THREADS), 0, ctx->stream, runs, off, payload, d_cum, out, raw_len, n_seg, seg_log2, flag, vec);
}

extern "C" int mcom_rans_encode(mcom_ctx *ctx, const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t cap, uint64_t *out_len, int model_hint)
{
	if (!ctx) return MCOM_E_ARG;
	if (!out_len || !d_out || (n && !d_in)) return mcom_fail(ctx, MCOM_E_ARG, "rans_encode: null pointer");
	if (n > ((uint64_t)1 << 34)) return mcom_fail(ctx, MCOM_E_ARG, "rans_encode: %llu bytes (members of up to 16 GB)", (unsigned long long)n);
	*out_len = 0;
	if (cap < HEADER_BYTES) return mcom_fail(ctx, MCOM_E_OVERFLOW, "rans_encode: room for %llu bytes", (unsigned long long)cap);
	Blocks B(ctx);
	const int vec = ((uintptr_t)d_in & 15) == 0;
	const uint64_t n_seg = (n + SEG - 1) >> SEG_LOG2;
	// histograms down, the model chosen and its tables made by the shared host code
	Hist hist;
	Header hd; hd.raw_len = n;
	if (n) {
		unsigned long long *d_hist = nullptr;
		const size_t hist_words = 4 * 256 + (size_t)N_PLANES_ALL * 65536;
		MCOM_HIP(ctx, B.get(&d_hist, hist_words * 8));
		int rc = launch_hist(ctx, d_in, n, d_hist);
		if (rc) return rc;
		MCOM_HIP(ctx, hipMemcpyAsync(hist.o0.data(), d_hist, 4 * 256 * 8, hipMemcpyDeviceToHost, ctx->stream));
		MCOM_HIP(ctx, hipMemcpyAsync(hist.o1.data(), d_hist + 4 * 256, (size_t)N_PLANES_ALL * 65536 * 8, hipMemcpyDeviceToHost, ctx->stream));
		rc = device_crc(ctx, B, d_in, n, SEG_LOG2, &hd.crc);             // (synchronises: the histograms are down as well)
		if (rc) return rc;
	}
	Model m;
	if (!choose(hist, n, model_hint, m, nullptr)) return mcom_fail(ctx, MCOM_E_ARG, "rans_encode: model hint 0x%x", model_hint);
	hd.model = (uint8_t)m.model; hd.stride = (uint8_t)m.stride; hd.table_bytes = (uint32_t)m.ser.size();
	std::vector<uint8_t> head(HEADER_BYTES + m.ser.size());
	if (m.model == STORED) {
		hd.payload_bytes = n;
		if (cap < HEADER_BYTES + n) return mcom_fail(ctx, MCOM_E_OVERFLOW, "rans_encode: %llu bytes, room for %llu", (unsigned long long)(HEADER_BYTES + n), (unsigned long long)cap);
		write_header(head.data(), hd);
		MCOM_HIP(ctx, hipMemcpyAsync(d_out, head.data(), HEADER_BYTES, hipMemcpyHostToDevice, ctx->stream));
		if (n) MCOM_HIP(ctx, hipMemcpyAsync(d_out + HEADER_BYTES, d_in, n, hipMemcpyDeviceToDevice, ctx->stream));
		MCOM_HIP(ctx, mcom_stream_sync(ctx));
		*out_len = HEADER_BYTES + n;
		return MCOM_OK;
	}
	uint16_t *d_cum = nullptr; uint8_t *scratch = nullptr; uint64_t *lens = nullptr, *off = nullptr; uint32_t *d_flag = nullptr;
	uint64_t payload = 0;
	if (n_seg) {
		MCOM_HIP(ctx, B.get(&d_cum, m.cum.size() * 2));
		MCOM_HIP(ctx, B.get(&scratch, n_seg * run_cap(SEG)));
		MCOM_HIP(ctx, B.get(&lens, 2 * (n_seg + 1) * 8 + 16));
		off = lens + n_seg + 1; d_flag = (uint32_t*)(off + n_seg + 1);
		MCOM_HIP(ctx, hipMemcpyAsync(d_cum, m.cum.data(), m.cum.size() * 2, hipMemcpyHostToDevice, ctx->stream));
		MCOM_HIP(ctx, hipMemsetAsync(d_flag, 0, 4, ctx->stream));
		MCOM_HIP(ctx, hipMemsetAsync(lens + n_seg, 0, 8, ctx->stream));
		const int o1 = m.model == ORDER1;
		switch (o1 * 8 + m.stride) {
		case 1: launch_encode<0, 1>(ctx, d_in, n, n_seg, d_cum, scratch, lens, d_flag, vec); break;
		case 2: launch_encode<0, 2>(ctx, d_in, n, n_seg, d_cum, scratch, lens, d_flag, vec); break;
		case 4: launch_encode<0, 4>(ctx, d_in, n, n_seg, d_cum, scratch, lens, d_flag, vec); break;
		case 9: launch_encode<1, 1>(ctx, d_in, n, n_seg, d_cum, scratch, lens, d_flag, vec); break;
		case 10: launch_encode<1, 2>(ctx, d_in, n, n_seg, d_cum, scratch, lens, d_flag, vec); break;
		default: launch_encode<1, 4>(ctx, d_in, n, n_seg, d_cum, scratch, lens, d_flag, vec); break;
		}
		MCOM_LAUNCH_CHECK(ctx);
		int rc = mcom_scan64(ctx, lens, off, n_seg + 1, nullptr);
		if (rc) return rc;
		uint32_t flag = 0;
		MCOM_HIP(ctx, hipMemcpyAsync(&payload, off + n_seg, 8, hipMemcpyDeviceToHost, ctx->stream));
		MCOM_HIP(ctx, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
		MCOM_HIP(ctx, mcom_stream_sync(ctx));
		if (flag) return mcom_fail(ctx, MCOM_E_HIP, "rans_encode: the encoder raised flag 0x%x", flag);
	}
	hd.payload_bytes = payload;
	const uint64_t total = HEADER_BYTES + m.ser.size() + 2 * n_seg + payload;
	if (total > cap) return mcom_fail(ctx, MCOM_E_OVERFLOW, "rans_encode: %llu bytes, room for %llu", (unsigned long long)total, (unsigned long long)cap);
	write_header(head.data(), hd);
	if (!m.ser.empty()) memcpy(head.data() + HEADER_BYTES, m.ser.data(), m.ser.size());
	MCOM_HIP(ctx, hipMemcpyAsync(d_out, head.data(), head.size(), hipMemcpyHostToDevice, ctx->stream));
	uint8_t *out_lens = d_out + head.size();
	if (n_seg) MCOM_LAUNCH(k_rans_compact, dim3(blocks_for(((n_seg + 15) / 16) * 64)), dim3(RN_THREADS), 0, ctx->stream, (const uint8_t*)scratch, (const uint64_t*)lens, (const uint64_t*)off, n_seg,
	            out_lens, out_lens + 2 * n_seg);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	*out_len = total;
	return MCOM_OK;
}

extern "C" int mcom_rans_decode(mcom_ctx *ctx, const uint8_t *d_in, uint64_t in_len, uint8_t *d_out, uint64_t cap, uint64_t *out_len)
{
	if (!ctx) return MCOM_E_ARG;
	if (!out_len || (in_len && !d_in)) return mcom_fail(ctx, MCOM_E_ARG, "rans_decode: null pointer");
	*out_len = 0;
	Blocks B(ctx);
	uint8_t hb[HEADER_BYTES];
	if (in_len < HEADER_BYTES) return mcom_fail(ctx, MCOM_E_ARG, "rans_decode: not a .rans member (%llu bytes)", (unsigned long long)in_len);
	MCOM_HIP(ctx, hipMemcpyAsync(hb, d_in, HEADER_BYTES, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	Header hd;
	if (!read_header(hb, in_len, hd)) return mcom_fail(ctx, MCOM_E_ARG, "rans_decode: the header does not describe this member");
	*out_len = hd.raw_len;
	if (hd.raw_len > cap) return mcom_fail(ctx, MCOM_E_OVERFLOW, "rans_decode: %llu bytes, room for %llu", (unsigned long long)hd.raw_len, (unsigned long long)cap);
	if (hd.raw_len && !d_out) return mcom_fail(ctx, MCOM_E_ARG, "rans_decode: null pointer");
	const int vec = ((uintptr_t)d_out & 15) == 0;
	const uint64_t n_seg = hd.n_seg();
	if (hd.model == STORED) {
		if (hd.raw_len) MCOM_HIP(ctx, hipMemcpyAsync(d_out, d_in + HEADER_BYTES, hd.raw_len, hipMemcpyDeviceToDevice, ctx->stream));
	} else if (hd.raw_len == 0) {
		std::vector<uint8_t> ser(hd.table_bytes); std::vector<uint16_t> cum;
		if (hd.table_bytes) { MCOM_HIP(ctx, hipMemcpyAsync(ser.data(), d_in + HEADER_BYTES, hd.table_bytes, hipMemcpyDeviceToHost, ctx->stream)); MCOM_HIP(ctx, mcom_stream_sync(ctx)); }
		if (!parse_tables(ser.data(), ser.size(), hd.model, hd.stride, cum)) { *out_len = 0; return mcom_fail(ctx, MCOM_E_ARG, "rans_decode: malformed tables"); }
	} else {
		std::vector<uint8_t> ser(hd.table_bytes); std::vector<uint16_t> cum;
		if (hd.table_bytes) { MCOM_HIP(ctx, hipMemcpyAsync(ser.data(), d_in + HEADER_BYTES, hd.table_bytes, hipMemcpyDeviceToHost, ctx->stream)); MCOM_HIP(ctx, mcom_stream_sync(ctx)); }
		if (!parse_tables(ser.data(), ser.size(), hd.model, hd.stride, cum)) { *out_len = 0; return mcom_fail(ctx, MCOM_E_ARG, "rans_decode: malformed tables"); }
		uint16_t *d_cum = nullptr; uint64_t *lens = nullptr, *off = nullptr; uint32_t *d_flag = nullptr;
		MCOM_HIP(ctx, B.get(&d_cum, cum.size() * 2));
		MCOM_HIP(ctx, B.get(&lens, 2 * (n_seg + 1) * 8 + 16));
		off = lens + n_seg + 1; d_flag = (uint32_t*)(off + n_seg + 1);
		MCOM_HIP(ctx, hipMemcpyAsync(d_cum, cum.data(), cum.size() * 2, hipMemcpyHostToDevice, ctx->stream));
		MCOM_HIP(ctx, hipMemsetAsync(d_flag, 0, 4, ctx->stream));
		const uint8_t *lens16 = d_in + HEADER_BYTES + hd.table_bytes, *runs = lens16 + 2 * n_seg;
		MCOM_LAUNCH(k_rans_lens, dim3(blocks_for(n_seg + 1)), dim3(RN_THREADS), 0, ctx->stream, lens16, n_seg, lens);
		MCOM_LAUNCH_CHECK(ctx);
		int rc = mcom_scan64(ctx, lens, off, n_seg + 1, nullptr);
		if (rc) return rc;
		uint64_t payload = 0;
		MCOM_HIP(ctx, hipMemcpyAsync(&payload, off + n_seg, 8, hipMemcpyDeviceToHost, ctx->stream));
		MCOM_HIP(ctx, mcom_stream_sync(ctx));
		if (payload != hd.payload_bytes) { *out_len = 0; return mcom_fail(ctx, MCOM_E_ARG, "rans_decode: the run lengths do not add up to the payload"); }
		const int o1 = hd.model == ORDER1;
		switch (o1 * 8 + hd.stride) {
		case 1: launch_decode<0, 1>(ctx, runs, off, payload, d_cum, d_out, hd.raw_len, n_seg, hd.seg_log2, d_flag, vec); break;
		case 2: launch_decode<0, 2>(ctx, runs, off, payload, d_cum, d_out, hd.raw_len, n_seg, hd.seg_log2, d_flag, vec); break;
		case 4: launch_decode<0, 4>(ctx, runs, off, payload, d_cum, d_out, hd.raw_len, n_seg, hd.seg_log2, d_flag, vec); break;
		case 9: launch_decode<1, 1>(ctx, runs, off, payload, d_cum, d_out, hd.raw_len, n_seg, hd.seg_log2, d_flag, vec); break;
		case 10: launch_decode<1, 2>(ctx, runs, off, payload, d_cum, d_out, hd.raw_len, n_seg, hd.seg_log2, d_flag, vec); break;
		default: launch_decode<1, 4>(ctx, runs, off, payload, d_cum, d_out, hd.raw_len, n_seg, hd.seg_log2, d_flag, vec); break;
		}
		MCOM_LAUNCH_CHECK(ctx);
		uint32_t flag = 0;
		MCOM_HIP(ctx, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
		MCOM_HIP(ctx, mcom_stream_sync(ctx));
		if (flag) { *out_len = 0; return mcom_fail(ctx, MCOM_E_ARG, "rans_decode: corrupt member (flag 0x%x)", flag); }
	}
	uint32_t crc = 0;
	int rc = device_crc(ctx, B, d_out, hd.raw_len, hd.seg_log2, &crc);
	if (rc) return rc;
	if (crc != hd.crc) { *out_len = 0; return mcom_fail(ctx, MCOM_E_ARG, "rans_decode: CRC mismatch"); }
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}

// ---- test hooks (include/mcom_test.h) ----------------------------------------------------------------------------------------------
extern "C" int mcom_test_rans_hist(mcom_ctx *ctx, const uint8_t *d_in, uint64_t n, uint64_t *d_counts)
{
	if (!ctx) return MCOM_E_ARG;
	if (!d_counts || !d_in || !n) return mcom_fail(ctx, MCOM_E_ARG, "test_rans_hist: null pointer or no bytes");
	if (n > ((uint64_t)1 << 34)) return mcom_fail(ctx, MCOM_E_ARG, "test_rans_hist: %llu bytes (members of up to 16 GB)", (unsigned long long)n);
	int rc = launch_hist(ctx, d_in, n, (unsigned long long*)d_counts);
	if (rc) return rc;
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}

extern "C" int mcom_test_rans_seg_crc(mcom_ctx *ctx, const uint8_t *d_in, uint64_t n, uint32_t seg_log2, uint32_t *d_crc)
{
	if (!ctx) return MCOM_E_ARG;
	if (!d_crc || !d_in || !n) return mcom_fail(ctx, MCOM_E_ARG, "test_rans_seg_crc: null pointer or no bytes");
	if (seg_log2 < SEG_LOG2_MIN || seg_log2 > SEG_LOG2_MAX) return mcom_fail(ctx, MCOM_E_ARG, "test_rans_seg_crc: segments of 2^%u bytes", seg_log2);
	int rc = launch_seg_crc(ctx, d_in, n, seg_log2, d_crc);
	if (rc) return rc;
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}
