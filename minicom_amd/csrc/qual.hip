// minicom_amd/csrc/qual.hip -- quality values as `.mcq` members: a static context-model rANS coder over a matrix of n_rows x L bytes
// (format, alphabet, context rule, normalisation, model choice: qual_model.hpp; specification and cross-check: host/mcom_qual.cpp;
// DESIGN.md section 3.9).
//
//   k_qual_alpha    which byte values occur: flags in LDS, one atomic OR per value and workgroup into the 256-bit map
//   k_qual_hist     the counts of model 4, [s[j-1]][bin of max(s[j-2], s[j-3])][floor(8 j / L)][symbol] over dense symbols, one thread per
//                   16 columns of a row.  Alphabets of at most 8 values (binned instruments): 8 * 8 * 8 * 8 counters of 32 bits in LDS,
//                   flushed once per workgroup; otherwise 64-bit atomics on one table in global memory (94 * 64 * 94 counters = 4.5 MB
//                   for the whole printable range: L2 holds the part that is hit).  The other models' counts are sums of these (host).
//   k_qual_encode   one lane per segment (rows_per_seg rows), last row first, last column first; coded bytes go top-down into the lane's
//                   own scratch run, four at a time; the run's length into lens[]
//   (mcom_scan64)   run offsets
//   k_qual_compact  a wave copies 16 runs to their final places and writes their u16 lengths
//   k_qual_lens     decode: the u16 lengths (at any byte offset) -> u64 for the scan
//   k_qual_decode   one lane per segment.  The cumulative rows of all contexts sit in LDS when they take at most 40 KB, otherwise the
//                   context's row is bisected in global memory; either way the bisection takes at most 8 steps over the A + 1 entries
//                   of a row.  64 decoded bytes per lane are staged in LDS, then every group of four lanes stores one segment's 64 bytes
//                   as 16-byte pieces (vector stores where the address is aligned and the piece lies inside the segment).
//   k_qual_gather   rows through an order: sixteen lanes per OUTPUT row j copy source row order[j], as the aligned 16-byte pieces of the
//                   output they cover (vector stores; ragged byte pieces at both ends; the source is read unaligned).  The kernel is the
//                   order's validity check as well: an index >= n_src raises a flag and is skipped, a source row named twice raises
//                   another (one bit per source row, atomicOr).  DESIGN.md section 3.11.
// The decoder always writes a flat image (row after row); rows that are `pitch` != L apart are spread by a 2-D copy afterwards.
// The CRC-32 goes through the `.rans` coder's path (mcom_device_crc32).
// Untrusted input (the rule of section 3.5): sizes, tables and run lengths are judged on the host before a kernel runs; every loop of
// the decoder is bounded by the header's counts; a run read beyond its end, a state outside [2^23, 2^31), a slot that no symbol owns,
// a run that is not used up exactly and a symbol >= A raise the flag word and skip the access.
#include "mcom_dev.hpp"
#include "qual_model.hpp"

using namespace mcom_qual;

#define QV_THREADS 256
#define QV_STAGE_PITCH 80
#define QV_LDS_TABLE_BYTES (40 * 1024)
enum { QV_F_RUN = 1, QV_F_SLOT = 2, QV_F_STATE = 4, QV_F_END = 8, QV_F_FREQ = 16, QV_F_ROOM = 32, QV_F_SYM = 64 };

__global__ __launch_bounds__(QV_THREADS) void k_qual_alpha(const uint8_t *__restrict__ rows, uint64_t n_rows, uint32_t L, uint64_t pitch, uint32_t *__restrict__ map)
{
	__shared__ uint32_t seen[256];
	seen[threadIdx.x] = 0;
	__syncthreads();
	const uint32_t cpr = (L + 15) / 16;
	const uint64_t chunks = n_rows * cpr;
	for (uint64_t c = (uint64_t)blockIdx.x * QV_THREADS + threadIdx.x; c < chunks; c += (uint64_t)gridDim.x * QV_THREADS) {
		const uint64_t r = c / cpr; const uint32_t j0 = (uint32_t)(c % cpr) * 16;
		const uint8_t *p = rows + r * pitch + j0;
		const uint32_t valid = L - j0 < 16 ? L - j0 : 16u;
		for (uint32_t k = 0; k < valid; ++k) seen[p[k]] = 1;                // (every writer stores the same value)
	}
	__syncthreads();
	if (seen[threadIdx.x]) atomicOr(&map[threadIdx.x >> 5], 1u << (threadIdx.x & 31));
}

// tabs: rank[256] | mbin[256] | value[256]
template <int IN_LDS>
__global__ __launch_bounds__(QV_THREADS) void k_qual_hist(const uint8_t *__restrict__ rows, uint64_t n_rows, uint32_t L, uint64_t pitch, const uint8_t *__restrict__ tabs,
                                                          uint32_t A, uint32_t Q, unsigned long long *__restrict__ counts)
{
	__shared__ uint8_t s_rank[256], s_mbin[256];
	__shared__ uint32_t s_cnt[IN_LDS ? 4096 : 1];
	s_rank[threadIdx.x] = tabs[threadIdx.x]; s_mbin[threadIdx.x] = tabs[256 + threadIdx.x];
	if (IN_LDS) for (int t = threadIdx.x; t < 4096; t += QV_THREADS) s_cnt[t] = 0;
	__syncthreads();
	const uint32_t cpr = (L + 15) / 16;
	const uint64_t chunks = n_rows * cpr;
	for (uint64_t c = (uint64_t)blockIdx.x * QV_THREADS + threadIdx.x; c < chunks; c += (uint64_t)gridDim.x * QV_THREADS) {
		const uint64_t r = c / cpr; const int j0 = (int)(c % cpr) * 16;
		const uint8_t *p = rows + r * pitch;
		uint32_t sy[19];
#pragma unroll
		for (int k = 0; k < 19; ++k) { const int j = j0 - 3 + k; sy[k] = j >= 0 && j < (int)L ? (uint32_t)s_rank[p[j]] : 0u; }
#pragma unroll
		for (int k = 0; k < 16; ++k) {
			const uint32_t j = (uint32_t)(j0 + k);
			if (j >= L) continue;
			const uint32_t s = sy[k + 3], p1 = sy[k + 2], p2 = sy[k + 1], p3 = sy[k], pos = 8 * j / L;
			const uint32_t idx = ((p1 * Q + s_mbin[p2 > p3 ? p2 : p3]) * 8 + pos) * A + s;
			if (IN_LDS) atomicAdd(&s_cnt[idx & 4095], 1u); else atomicAdd(&counts[idx], 1ull);
		}
	}
	if (IN_LDS) {
		__syncthreads();
		const uint32_t words = A * Q * 8 * A;                               // <= 4096: A <= 8
		for (uint32_t t = threadIdx.x; t < words && t < 4096; t += QV_THREADS) if (s_cnt[t]) atomicAdd(&counts[t], (unsigned long long)s_cnt[t]);
	}
}

// the coded bytes of one lane: written from the top of its scratch run downwards, the byte emitted first at the highest address
struct QvEmit {
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

__device__ __forceinline__ uint32_t qv_ctx(int id, uint32_t Q, const uint8_t *mbin, uint32_t p1, uint32_t p2, uint32_t p3, uint32_t pos)
{
	return id == Q_P ? p1 : id == Q_PP ? p1 * 8 + pos : id == Q_PMP ? (p1 * Q + mbin[p2 > p3 ? p2 : p3]) * 8 + pos : 0u;
}

// scratch: n_seg runs of `cap` bytes (a multiple of 4), 4-byte aligned
__global__ __launch_bounds__(QV_THREADS) void k_qual_encode(const uint8_t *__restrict__ rows, uint64_t n_rows, uint32_t L, uint64_t pitch, uint32_t rps,
                                                            const uint8_t *__restrict__ tabs, const uint16_t *__restrict__ cum, int id, uint32_t A, uint32_t Q,
                                                            uint8_t *__restrict__ scratch, uint32_t cap, uint64_t *__restrict__ lens, uint32_t *__restrict__ flag, uint64_t n_seg)
{
	__shared__ uint8_t s_rank[256], s_mbin[256];
	s_rank[threadIdx.x] = tabs[threadIdx.x]; s_mbin[threadIdx.x] = tabs[256 + threadIdx.x];
	__syncthreads();
	const uint64_t seg = (uint64_t)blockIdx.x * QV_THREADS + threadIdx.x;
	if (seg >= n_seg) return;
	const uint64_t r0 = seg * rps, r1 = r0 + rps < n_rows ? r0 + rps : n_rows;
	QvEmit e; e.bottom = scratch + seg * cap; e.wp = e.bottom + cap;
	uint8_t *const top = e.wp;
	uint32_t x = STATE_L;
	bool bad = false;
	const uint32_t pos_last = 8 * (L - 1) / L; const int acc_last = (int)(8 * (L - 1) % L);
	for (uint64_t r = r1; r-- > r0; ) {
		const uint8_t *s = rows + r * pitch;
		uint32_t s0 = s_rank[s[L - 1]], s1 = L >= 2 ? (uint32_t)s_rank[s[L - 2]] : 0u, s2 = L >= 3 ? (uint32_t)s_rank[s[L - 3]] : 0u, s3 = L >= 4 ? (uint32_t)s_rank[s[L - 4]] : 0u;
		uint32_t pos = pos_last; int acc = acc_last;                        // floor(8 j / L) and 8 j mod L of the column in hand
		for (uint32_t j = L; j-- > 0; ) {
			const uint16_t *row = cum + (size_t)qv_ctx(id, Q, s_mbin, s1, s2, s3, pos) * (A + 1);
			const uint32_t c = row[s0], f = row[s0 + 1] - c;
			if (f == 0 || f > PROB_M) bad = true;                           // (a symbol the tables do not hold: they were made from other data)
			else {
				const uint32_t x_max = f << 19;
				while (x >= x_max) { e.put(x); x >>= 8; }
				x = ((x / f) << PROB_BITS) + (x % f) + c;
			}
			s0 = s1; s1 = s2; s2 = s3; s3 = j >= 4 ? (uint32_t)s_rank[s[j - 4]] : 0u;
			if (j) { acc -= 8; while (acc < 0) { acc += (int)L; --pos; } }
		}
	}
	e.put(x >> 24); e.put(x >> 16); e.put(x >> 8); e.put(x);
	e.finish();
	if (bad) atomicOr(flag, (uint32_t)QV_F_FREQ);
	if (e.full) atomicOr(flag, (uint32_t)QV_F_ROOM);
	lens[seg] = (uint64_t)(top - e.wp);
}

__global__ __launch_bounds__(QV_THREADS) void k_qual_compact(const uint8_t *__restrict__ scratch, uint32_t cap, const uint64_t *__restrict__ lens, const uint64_t *__restrict__ off,
                                                             uint64_t n_seg, uint8_t *__restrict__ out_lens, uint8_t *__restrict__ out_runs)
{
	const uint64_t wave = ((uint64_t)blockIdx.x * QV_THREADS + threadIdx.x) >> 6;
	const uint32_t lane = threadIdx.x & 63;
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
__global__ __launch_bounds__(QV_THREADS) void k_qual_lens(const uint8_t *__restrict__ lens16, uint64_t n_seg, uint64_t *__restrict__ lens64)
{
	const uint64_t seg = (uint64_t)blockIdx.x * QV_THREADS + threadIdx.x;
	if (seg > n_seg) return;
	lens64[seg] = seg < n_seg ? (uint64_t)(lens16[2 * seg] | (uint32_t)lens16[2 * seg + 1] << 8) : 0ull;
}

// Segments seg_base .. n_seg - 1 are decoded (n_seg: at most the member's).  out: the flat image of these segments, which begins with
// segment seg_base: (n_seg - seg_base) * rps * L bytes, fewer where the member's last segment is short (seg_base = 0 and all segments:
// the n_rows * L bytes of the whole member).  top: the largest power of two below A (0 for A = 1): the first step of the bisection.
template <int LDS_TAB>
__global__ __launch_bounds__(QV_THREADS) void k_qual_decode(const uint8_t *__restrict__ runs, const uint64_t *__restrict__ off, uint64_t payload_bytes,
                                                            const uint16_t *__restrict__ cum, uint32_t cum_words, const uint8_t *__restrict__ tabs, int id, uint32_t A, uint32_t Q,
                                                            uint32_t top, uint8_t *__restrict__ out, uint64_t n_rows, uint32_t L, uint32_t rps, uint64_t seg_base,
                                                            uint64_t n_seg, uint32_t *__restrict__ flag)
{
	__shared__ __attribute__((aligned(16))) uint8_t stage[QV_THREADS * QV_STAGE_PITCH];
	__shared__ uint8_t s_val[256], s_mbin[256];
	extern __shared__ uint16_t s_cum[];
	s_mbin[threadIdx.x] = tabs[256 + threadIdx.x]; s_val[threadIdx.x] = tabs[512 + threadIdx.x];
	if (LDS_TAB) for (uint32_t t = threadIdx.x; t < cum_words; t += QV_THREADS) s_cum[t] = cum[t];
	__syncthreads();
	const uint16_t *const tab = LDS_TAB ? (const uint16_t*)s_cum : cum;
	const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const uint64_t seg = seg_base + (uint64_t)blockIdx.x * QV_THREADS + threadIdx.x, wave_seg0 = seg - lane;
	const uint64_t seg_bytes = (uint64_t)rps * L, raw_len = n_rows * L, out_at = seg_base * seg_bytes;   // out[0] is byte out_at of the member's image
	uint32_t len = 0, x = 0, bad = 0;
	const uint8_t *p = runs, *end = runs;
	if (seg < n_seg) {
		const uint64_t a = off[seg], b = off[seg + 1];
		const uint64_t at = seg * seg_bytes;
		len = raw_len - at < seg_bytes ? (uint32_t)(raw_len - at) : (uint32_t)seg_bytes;
		if (b < a || b > payload_bytes || b - a < 4) bad = QV_F_RUN;
		else {
			p = runs + a; end = runs + b;
			x = p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; p += 4;
			if (x < STATE_L || x >= (1u << 31)) bad = QV_F_STATE;
		}
	}
	if (bad) len = 0;
	uint8_t *const my_stage = stage + (size_t)threadIdx.x * QV_STAGE_PITCH;
	const uint8_t *const wave_stage = stage + (size_t)wv * 64 * QV_STAGE_PITCH;
	uint32_t done = 0, j = 0, pos = 0, acc = 0, s1 = 0, s2 = 0, s3 = 0;     // the column in hand, floor(8 j / L), 8 j mod L, the three symbols before it
	const uint32_t rounds = (uint32_t)((seg_bytes + 63) / 64);
	for (uint32_t r = 0; r < rounds; ++r) {
#pragma unroll 1
		for (int q = 0; q < 4; ++q) {
			uint32_t w[4] = {0, 0, 0, 0};
			const uint32_t valid = bad ? 0u : len - done < 16 ? len - done : 16u;
#pragma unroll
			for (int k = 0; k < 16; ++k) {
				if ((uint32_t)k < valid && !bad) {
					const uint16_t *row = tab + (size_t)qv_ctx(id, Q, s_mbin, s1, s2, s3, pos) * (A + 1);
					const uint32_t slot = x & (PROB_M - 1);
					uint32_t lo = 0;
					for (uint32_t st = top; st; st >>= 1) if (lo + st < A && row[lo + st] <= slot) lo += st;
					const uint32_t c = row[lo], f = row[lo + 1] - c;
					if (slot - c >= f) bad = QV_F_SLOT;                     // no symbol of this row owns the slot (an empty row: f = 0)
					else if (lo >= A) bad = QV_F_SYM;
					else {
						x = f * (x >> PROB_BITS) + slot - c;
						while (x < STATE_L && !bad) {
							if (p >= end) bad = QV_F_RUN;                   // the run is used up: nothing is read
							else x = (x << 8) | *p++;
						}
						w[k >> 2] |= (uint32_t)s_val[lo] << ((k & 3) * 8);
						s3 = s2; s2 = s1; s1 = lo;
						acc += 8; while (acc >= L) { acc -= L; ++pos; }
						if (++j == L) { j = 0; pos = 0; acc = 0; s1 = s2 = s3 = 0; }
					}
				}
			}
			done += valid;
			*(uint4*)(my_stage + q * 16) = make_uint4(w[0], w[1], w[2], w[3]);
		}
		__syncthreads();
		// 64 bytes of 64 segments: four lanes store one segment's, 16 segments per step; nothing beyond the segment's own bytes
#pragma unroll
		for (int it = 0; it < 4; ++it) {
			const uint32_t sseg = it * 16 + (lane >> 2), piece = lane & 3;
			const uint64_t gseg = wave_seg0 + sseg;
			if (gseg >= n_seg) continue;
			const uint64_t seg_at = gseg * seg_bytes, seg_end = raw_len - seg_at < seg_bytes ? raw_len : seg_at + seg_bytes;
			const uint64_t goff = seg_at + (uint64_t)r * 64 + piece * 16;
			if (goff >= seg_end) continue;
			const uint4 v = *(const uint4*)(wave_stage + (size_t)sseg * QV_STAGE_PITCH + piece * 16);
			uint8_t *const dst = out + (goff - out_at);                         // (gseg >= seg_base: goff >= out_at)
			if (goff + 16 <= seg_end && ((uintptr_t)dst & 15) == 0) *(uint4*)dst = v;
			else {
				const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
				for (int k = 0; k < 16; ++k) if (goff + k < seg_end) dst[k] = (uint8_t)(vv[k >> 2] >> ((k & 3) * 8));
			}
		}
		__syncthreads();
	}
	if (seg < n_seg && !bad && (p != end || x != STATE_L)) bad = QV_F_END;
	if (bad) atomicOr(flag, bad);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
extern "C" uint64_t mcom_qual_bound(uint64_t n_rows, uint32_t L) { return bound(n_rows, L); }

extern "C" int mcom_qual_info(const uint8_t *h_member_prefix, uint64_t len, uint64_t *n_rows, uint32_t *L)
{
	QHeader hd;
	if (!h_member_prefix || !n_rows || !L || !read_qfields(h_member_prefix, len, hd)) return -1;
	*n_rows = hd.n_rows; *L = hd.L;
	return 0;
}

namespace {
struct Blocks {                                             // pooled device blocks of one call, back to the pool once the stream has passed them
	mcom_ctx *ctx; std::vector<void*> v;
	explicit Blocks(mcom_ctx *c) : ctx(c) {}
	~Blocks() { for (void *p : v) mcom_dfree_later(ctx, p); }
	template <class T> hipError_t get(T **out, size_t bytes) { hipError_t e = mcom_dmalloc((void**)out, bytes ? bytes : 16); if (e == hipSuccess) v.push_back(*out); return e; }
};
unsigned blocks_for(uint64_t items) { return (unsigned)((items + QV_THREADS - 1) / QV_THREADS); }
unsigned grid_for_chunks(mcom_ctx *ctx, uint64_t n_rows, uint32_t L)
{
	uint64_t g = (n_rows * ((L + 15) / 16) + QV_THREADS - 1) / QV_THREADS, gmax = (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 64) * 8;
	return (unsigned)(g > gmax ? gmax : g ? g : 1);
}

// The two launches whose results stay inside the library, each in ONE place: mcom_qual_encode and the hook of include/mcom_test.h go
// through these.  n_rows > 0.
int launch_alphabet(mcom_ctx *ctx, Blocks &B, const uint8_t *d_rows, uint64_t n_rows, uint32_t L, uint64_t pitch, uint8_t map[32])
{
	uint32_t *d_map = nullptr;
	MCOM_HIP(ctx, B.get(&d_map, 32));
	MCOM_HIP(ctx, hipMemsetAsync(d_map, 0, 32, ctx->stream));
	MCOM_LAUNCH(k_qual_alpha, dim3(grid_for_chunks(ctx, n_rows, L)), dim3(QV_THREADS), 0, ctx->stream, d_rows, n_rows, L, pitch, d_map);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, hipMemcpyAsync(map, d_map, 32, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}
// d_tabs: rank | mbin | value of g, on the device; d_counts: g.hist_words() u64, cleared here
int launch_hist(mcom_ctx *ctx, const uint8_t *d_rows, uint64_t n_rows, uint32_t L, uint64_t pitch, const Geometry &g, const uint8_t *d_tabs, unsigned long long *d_counts)
{
	MCOM_HIP(ctx, hipMemsetAsync(d_counts, 0, g.hist_words() * 8, ctx->stream));
	const dim3 grid(grid_for_chunks(ctx, n_rows, L));
	if (g.A <= 8) MCOM_LAUNCH(k_qual_hist<1>, grid, dim3(QV_THREADS), 0, ctx->stream, d_rows, n_rows, L, pitch, d_tabs, g.A, g.Q, d_counts);
	else MCOM_LAUNCH(k_qual_hist<0>, grid, dim3(QV_THREADS), 0, ctx->stream, d_rows, n_rows, L, pitch, d_tabs, g.A, g.Q, d_counts);
	MCOM_LAUNCH_CHECK(ctx);
	return MCOM_OK;
}
int upload_tabs(mcom_ctx *ctx, Blocks &B, const Geometry &g, uint8_t **d_tabs)
{
	uint8_t h[768];
	memcpy(h, g.rank, 256); memcpy(h + 256, g.mbin, 256); memcpy(h + 512, g.value, 256);
	MCOM_HIP(ctx, B.get(d_tabs, 768));
	MCOM_HIP(ctx, hipMemcpyAsync(*d_tabs, h, 768, hipMemcpyHostToDevice, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));                                  // (h lives on this frame)
	return MCOM_OK;
}
bool args_ok(uint64_t n_rows, uint32_t L, uint64_t pitch) { return L >= 1 && L <= L_MAX && pitch >= L && n_rows < ((uint64_t)1 << 32) && n_rows * L <= RAW_MAX; }
}  // namespace

extern "C" int mcom_qual_encode(mcom_ctx *ctx, const uint8_t *d_rows, uint64_t n_rows, uint32_t L, uint64_t pitch, uint8_t *d_out, uint64_t cap, uint64_t *out_len, int model_hint)
{
	if (!ctx) return MCOM_E_ARG;
	if (!out_len || !d_out || (n_rows && !d_rows)) return mcom_fail(ctx, MCOM_E_ARG, "qual_encode: null pointer");
	*out_len = 0;
	if (!args_ok(n_rows, L, pitch)) return mcom_fail(ctx, MCOM_E_ARG, "qual_encode: %llu rows of %u bytes, pitch %llu (L 1 .. 256, below 2^32 rows, at most 16 GB)",
	                                                 (unsigned long long)n_rows, L, (unsigned long long)pitch);
	if (cap < QHEADER_BYTES) return mcom_fail(ctx, MCOM_E_OVERFLOW, "qual_encode: room for %llu bytes", (unsigned long long)cap);
	Blocks B(ctx);
	const uint64_t raw = n_rows * L;
	QHeader hd; hd.n_rows = n_rows; hd.L = L; hd.rps = default_rps(L);
	const uint64_t n_seg = hd.n_seg();
	const uint32_t run_room = (uint32_t)qrun_cap(hd.rps * L);
	int rc;
	// the flat image: what the CRC and the `.rans` candidate are made of
	const uint8_t *d_flat = d_rows;
	if (raw && pitch != L) {
		uint8_t *f = nullptr;
		MCOM_HIP(ctx, B.get(&f, raw));
		MCOM_HIP(ctx, hipMemcpy2DAsync(f, L, d_rows, pitch, L, n_rows, hipMemcpyDeviceToDevice, ctx->stream));
		d_flat = f;
	}
	if ((rc = mcom_device_crc32(ctx, d_flat, raw, &hd.crc))) return rc;
	uint8_t *d_rans = nullptr; uint64_t rans_len = 0;
	if (model_hint == 0 || model_hint == HINT_RANS) {
		MCOM_HIP(ctx, B.get(&d_rans, mcom_rans::HEADER_BYTES + raw));
		if ((rc = mcom_rans_encode(ctx, d_flat, raw, d_rans, mcom_rans::HEADER_BYTES + raw, &rans_len, 0))) return rc;
	}
	QModel m; Geometry g;
	uint64_t total = 0, payload = 0;
	uint8_t *scratch = nullptr; uint64_t *lens = nullptr, *off = nullptr;
	if (model_hint != HINT_RANS) {
		std::vector<uint64_t> h4;
		uint8_t *d_tabs = nullptr;
		if (n_rows) {
			if ((rc = launch_alphabet(ctx, B, d_rows, n_rows, L, pitch, hd.map))) return rc;
			g.set(hd.map, L);
			if ((rc = upload_tabs(ctx, B, g, &d_tabs))) return rc;
			unsigned long long *d_counts = nullptr;
			MCOM_HIP(ctx, B.get(&d_counts, g.hist_words() * 8));
			if ((rc = launch_hist(ctx, d_rows, n_rows, L, pitch, g, d_tabs, d_counts))) return rc;
			h4.resize(g.hist_words());
			MCOM_HIP(ctx, hipMemcpyAsync(h4.data(), d_counts, h4.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
			MCOM_HIP(ctx, mcom_stream_sync(ctx));
		} else g.set(hd.map, L);
		if (!choose(g, h4, n_rows, n_seg, model_hint, m, nullptr)) return mcom_fail(ctx, MCOM_E_ARG, "qual_encode: model hint 0x%x", model_hint);
		hd.model = (uint8_t)m.id;
		if (m.id == Q_STORED) total = QHEADER_BYTES + raw;
		else {
			uint16_t *d_cum = nullptr; uint32_t *d_flag = nullptr;
			MCOM_HIP(ctx, B.get(&d_cum, m.cum.size() * 2));
			MCOM_HIP(ctx, B.get(&scratch, n_seg * run_room));
			MCOM_HIP(ctx, B.get(&lens, 2 * (n_seg + 1) * 8 + 16));
			off = lens + n_seg + 1; d_flag = (uint32_t*)(off + n_seg + 1);
			MCOM_HIP(ctx, hipMemcpyAsync(d_cum, m.cum.data(), m.cum.size() * 2, hipMemcpyHostToDevice, ctx->stream));
			MCOM_HIP(ctx, hipMemsetAsync(d_flag, 0, 4, ctx->stream));
			MCOM_HIP(ctx, hipMemsetAsync(lens + n_seg, 0, 8, ctx->stream));
			MCOM_LAUNCH(k_qual_encode, dim3(blocks_for(n_seg)), dim3(QV_THREADS), 0, ctx->stream, d_rows, n_rows, L, pitch, hd.rps, (const uint8_t*)d_tabs, (const uint16_t*)d_cum,
			            m.id, g.A, g.Q, scratch, run_room, lens, d_flag, n_seg);
			MCOM_LAUNCH_CHECK(ctx);
			if ((rc = mcom_scan64(ctx, lens, off, n_seg + 1, nullptr))) return rc;
			uint32_t flag = 0;
			MCOM_HIP(ctx, hipMemcpyAsync(&payload, off + n_seg, 8, hipMemcpyDeviceToHost, ctx->stream));
			MCOM_HIP(ctx, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
			MCOM_HIP(ctx, mcom_stream_sync(ctx));
			if (flag) return mcom_fail(ctx, MCOM_E_HIP, "qual_encode: the encoder raised flag 0x%x", flag);
			hd.table_bytes = (uint32_t)m.ser.size(); hd.payload_bytes = payload;
			total = QHEADER_BYTES + m.ser.size() + 2 * n_seg + payload;
		}
	}
	uint8_t head[QHEADER_BYTES];
	if (model_hint == HINT_RANS || (model_hint == 0 && QHEADER_BYTES + rans_len < total)) {
		QHeader rh; rh.kind = KIND_RANS; rh.n_rows = n_rows; rh.L = L; rh.rps = hd.rps; rh.crc = hd.crc; rh.payload_bytes = rans_len;
		total = QHEADER_BYTES + rans_len;
		if (total > cap) return mcom_fail(ctx, MCOM_E_OVERFLOW, "qual_encode: %llu bytes, room for %llu", (unsigned long long)total, (unsigned long long)cap);
		write_qheader(head, rh);
		MCOM_HIP(ctx, hipMemcpyAsync(d_out, head, QHEADER_BYTES, hipMemcpyHostToDevice, ctx->stream));
		MCOM_HIP(ctx, hipMemcpyAsync(d_out + QHEADER_BYTES, d_rans, rans_len, hipMemcpyDeviceToDevice, ctx->stream));
		MCOM_HIP(ctx, mcom_stream_sync(ctx));
		*out_len = total;
		return MCOM_OK;
	}
	if (total > cap) return mcom_fail(ctx, MCOM_E_OVERFLOW, "qual_encode: %llu bytes, room for %llu", (unsigned long long)total, (unsigned long long)cap);
	std::vector<uint8_t> front;                                            // header | tables of the coded form: alive until the stream has been synchronised
	if (m.id == Q_STORED) {
		hd.payload_bytes = raw;
		write_qheader(head, hd);
		MCOM_HIP(ctx, hipMemcpyAsync(d_out, head, QHEADER_BYTES, hipMemcpyHostToDevice, ctx->stream));
		if (raw) MCOM_HIP(ctx, hipMemcpyAsync(d_out + QHEADER_BYTES, d_flat, raw, hipMemcpyDeviceToDevice, ctx->stream));
	} else {
		front.resize(QHEADER_BYTES + m.ser.size());
		write_qheader(front.data(), hd);
		memcpy(front.data() + QHEADER_BYTES, m.ser.data(), m.ser.size());
		MCOM_HIP(ctx, hipMemcpyAsync(d_out, front.data(), front.size(), hipMemcpyHostToDevice, ctx->stream));
		uint8_t *out_lens = d_out + front.size();
		MCOM_LAUNCH(k_qual_compact, dim3(blocks_for(((n_seg + 15) / 16) * 64)), dim3(QV_THREADS), 0, ctx->stream, (const uint8_t*)scratch, run_room, (const uint64_t*)lens,
		            (const uint64_t*)off, n_seg, out_lens, out_lens + 2 * n_seg);
		MCOM_LAUNCH_CHECK(ctx);
	}
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	*out_len = total;
	return MCOM_OK;
}

namespace {
// The coded form (kind 0, models 1 to 4) of a member whose header read_qheader has accepted: the tables parsed and uploaded, ALL run
// lengths scanned and their sum set against the payload, then segments seg0 .. seg1 - 1 (seg1 <= n_seg) decoded into d_img, the flat image
// that begins with segment seg0.  Synchronous.  MCOM_E_ARG with a message under `who` for what section 3.9 refuses.
int decode_segments(mcom_ctx *ctx, Blocks &B, const QHeader &hd, const uint8_t *d_in, uint64_t seg0, uint64_t seg1, uint8_t *d_img, const char *who)
{
	const uint32_t L = hd.L;
	const uint64_t n_seg = hd.n_seg();
	int rc;
	Geometry g; g.set(hd.map, L);
	std::vector<uint8_t> ser(hd.table_bytes); std::vector<uint16_t> cum;
	if (hd.table_bytes) { MCOM_HIP(ctx, hipMemcpyAsync(ser.data(), d_in + QHEADER_BYTES, hd.table_bytes, hipMemcpyDeviceToHost, ctx->stream)); MCOM_HIP(ctx, mcom_stream_sync(ctx)); }
	if (!parse_tables(ser.data(), ser.size(), g, hd.model, cum)) return mcom_fail(ctx, MCOM_E_ARG, "%s: malformed tables", who);
	uint8_t *d_tabs = nullptr; uint16_t *d_cum = nullptr; uint64_t *lens = nullptr, *off = nullptr; uint32_t *d_flag = nullptr;
	if ((rc = upload_tabs(ctx, B, g, &d_tabs))) return rc;
	MCOM_HIP(ctx, B.get(&d_cum, cum.size() * 2));
	MCOM_HIP(ctx, B.get(&lens, 2 * (n_seg + 1) * 8 + 16));
	off = lens + n_seg + 1; d_flag = (uint32_t*)(off + n_seg + 1);
	MCOM_HIP(ctx, hipMemcpyAsync(d_cum, cum.data(), cum.size() * 2, hipMemcpyHostToDevice, ctx->stream));
	MCOM_HIP(ctx, hipMemsetAsync(d_flag, 0, 4, ctx->stream));
	const uint8_t *lens16 = d_in + QHEADER_BYTES + hd.table_bytes, *runs = lens16 + 2 * n_seg;
	MCOM_LAUNCH(k_qual_lens, dim3(blocks_for(n_seg + 1)), dim3(QV_THREADS), 0, ctx->stream, lens16, n_seg, lens);
	MCOM_LAUNCH_CHECK(ctx);
	if ((rc = mcom_scan64(ctx, lens, off, n_seg + 1, nullptr))) return rc;
	uint64_t payload = 0;
	MCOM_HIP(ctx, hipMemcpyAsync(&payload, off + n_seg, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	if (payload != hd.payload_bytes) return mcom_fail(ctx, MCOM_E_ARG, "%s: the run lengths do not add up to the payload", who);
	if (seg1 <= seg0) return MCOM_OK;
	uint32_t top = 0;
	if (g.A > 1) { top = 1; while (top * 2 < g.A) top *= 2; }
	const size_t cum_bytes = cum.size() * 2;
	const uint32_t cum_words = (uint32_t)cum.size();
	if (cum_bytes <= QV_LDS_TABLE_BYTES)
		MCOM_LAUNCH(k_qual_decode<1>, dim3(blocks_for(seg1 - seg0)), dim3(QV_THREADS), cum_bytes, ctx->stream, runs, (const uint64_t*)off, payload, (const uint16_t*)d_cum, cum_words,
		            (const uint8_t*)d_tabs, (int)hd.model, g.A, g.Q, top, d_img, hd.n_rows, L, hd.rps, seg0, seg1, d_flag);
	else
		MCOM_LAUNCH(k_qual_decode<0>, dim3(blocks_for(seg1 - seg0)), dim3(QV_THREADS), 0, ctx->stream, runs, (const uint64_t*)off, payload, (const uint16_t*)d_cum, cum_words,
		            (const uint8_t*)d_tabs, (int)hd.model, g.A, g.Q, top, d_img, hd.n_rows, L, hd.rps, seg0, seg1, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	uint32_t flag = 0;
	MCOM_HIP(ctx, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	if (flag) return mcom_fail(ctx, MCOM_E_ARG, "%s: corrupt member (flag 0x%x)", who, flag);
	return MCOM_OK;
}
}  // namespace

extern "C" int mcom_qual_decode(mcom_ctx *ctx, const uint8_t *d_in, uint64_t in_len, uint8_t *d_rows, uint64_t pitch, uint64_t cap_rows, uint64_t *n_rows, uint32_t *L_out)
{
	if (!ctx) return MCOM_E_ARG;
	if (!n_rows || !L_out || (in_len && !d_in)) return mcom_fail(ctx, MCOM_E_ARG, "qual_decode: null pointer");
	*n_rows = 0; *L_out = 0;
	if (in_len < QHEADER_BYTES) return mcom_fail(ctx, MCOM_E_ARG, "qual_decode: not a .mcq member (%llu bytes)", (unsigned long long)in_len);
	Blocks B(ctx);
	uint8_t hb[QHEADER_BYTES + mcom_rans::HEADER_BYTES] = {0};
	const size_t head_bytes = in_len < sizeof hb ? (size_t)in_len : sizeof hb;
	MCOM_HIP(ctx, hipMemcpyAsync(hb, d_in, head_bytes, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	QHeader hd;
	if (!read_qheader(hb, in_len, hd)) return mcom_fail(ctx, MCOM_E_ARG, "qual_decode: the header does not describe this member");
	*n_rows = hd.n_rows; *L_out = hd.L;
	if (hd.n_rows > cap_rows) return mcom_fail(ctx, MCOM_E_OVERFLOW, "qual_decode: %llu rows, room for %llu", (unsigned long long)hd.n_rows, (unsigned long long)cap_rows);
	auto refuse = [&](const char *why) { *n_rows = 0; *L_out = 0; return mcom_fail(ctx, MCOM_E_ARG, "qual_decode: %s", why); };
	if (pitch < hd.L || (hd.n_rows && !d_rows)) return refuse("null pointer or a pitch below L");
	const uint32_t L = hd.L;
	const uint64_t raw = hd.raw_len(), n_seg = hd.n_seg();
	uint8_t *d_flat = d_rows;
	if (raw && pitch != L) MCOM_HIP(ctx, B.get(&d_flat, raw));
	int rc;
	uint32_t crc = 0;
	if (hd.kind == KIND_RANS) {
		uint64_t got = 0;
		if ((rc = mcom_rans_decode(ctx, d_in + QHEADER_BYTES, in_len - QHEADER_BYTES, d_flat, raw, &got)) || got != raw) { *n_rows = 0; *L_out = 0; return rc ? rc : mcom_fail(ctx, MCOM_E_ARG, "qual_decode: embedded length"); }
		crc = hd.crc;                                                       // (the embedded member's CRC is the header's and was checked)
	} else if (hd.model == Q_STORED) {
		if ((rc = mcom_device_crc32(ctx, d_in + QHEADER_BYTES, raw, &crc))) return rc;
		if (crc != hd.crc) return refuse("CRC mismatch");
		if (raw) MCOM_HIP(ctx, hipMemcpyAsync(d_flat, d_in + QHEADER_BYTES, raw, hipMemcpyDeviceToDevice, ctx->stream));
	} else {
		if ((rc = decode_segments(ctx, B, hd, d_in, 0, n_seg, d_flat, "qual_decode"))) { if (rc == MCOM_E_ARG) { *n_rows = 0; *L_out = 0; } return rc; }
		if ((rc = mcom_device_crc32(ctx, d_flat, raw, &crc))) return rc;
		if (crc != hd.crc) return refuse("CRC mismatch");
	}
	if (raw && pitch != L) MCOM_HIP(ctx, hipMemcpy2DAsync(d_rows, pitch, d_flat, L, L, hd.n_rows, hipMemcpyDeviceToDevice, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}

// Rows first_row .. first_row + count - 1 alone.  Only the segments that hold them are decoded; the member's
// CRC-32 covers all raw bytes and is not checked here -- a range that is the whole member takes mcom_qual_decode's path, CRC included.
// Kind 1 (an embedded `.rans` member) has no segments of rows: it is decoded whole into a temporary of n_rows * L bytes and sliced.
extern "C" int mcom_qual_decode_rows(mcom_ctx *ctx, const uint8_t *d_in, uint64_t in_len, uint64_t first_row, uint64_t count, uint8_t *d_rows, uint64_t pitch,
                                     uint64_t *n_rows, uint32_t *L_out)
{
	if (!ctx) return MCOM_E_ARG;
	if (!n_rows || !L_out || (in_len && !d_in)) return mcom_fail(ctx, MCOM_E_ARG, "qual_decode_rows: null pointer");
	*n_rows = 0; *L_out = 0;
	if (in_len < QHEADER_BYTES) return mcom_fail(ctx, MCOM_E_ARG, "qual_decode_rows: not a .mcq member (%llu bytes)", (unsigned long long)in_len);
	uint8_t hb[QHEADER_BYTES + mcom_rans::HEADER_BYTES] = {0};
	const size_t head_bytes = in_len < sizeof hb ? (size_t)in_len : sizeof hb;
	MCOM_HIP(ctx, hipMemcpyAsync(hb, d_in, head_bytes, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	QHeader hd;
	if (!read_qheader(hb, in_len, hd)) return mcom_fail(ctx, MCOM_E_ARG, "qual_decode_rows: the header does not describe this member");
	if (first_row > hd.n_rows) return mcom_fail(ctx, MCOM_E_ARG, "qual_decode_rows: row %llu of %llu", (unsigned long long)first_row, (unsigned long long)hd.n_rows);
	if (count > hd.n_rows - first_row) count = hd.n_rows - first_row;
	if (first_row == 0 && count == hd.n_rows) return mcom_qual_decode(ctx, d_in, in_len, d_rows, pitch, hd.n_rows, n_rows, L_out);
	*n_rows = hd.n_rows; *L_out = hd.L;
	auto refuse = [&](const char *why) { *n_rows = 0; *L_out = 0; return mcom_fail(ctx, MCOM_E_ARG, "qual_decode_rows: %s", why); };
	if (pitch < hd.L || (count && !d_rows)) return refuse("null pointer or a pitch below L");
	Blocks B(ctx);
	const uint32_t L = hd.L;
	const uint64_t raw = hd.raw_len();
	int rc;
	const uint8_t *src = nullptr;                                          // row first_row of a flat image
	if (hd.kind == KIND_RANS) {
		uint8_t *d_flat = nullptr; uint64_t got = 0;
		MCOM_HIP(ctx, B.get(&d_flat, raw));
		if ((rc = mcom_rans_decode(ctx, d_in + QHEADER_BYTES, in_len - QHEADER_BYTES, d_flat, raw, &got)) || got != raw) { *n_rows = 0; *L_out = 0; return rc ? rc : mcom_fail(ctx, MCOM_E_ARG, "qual_decode_rows: embedded length"); }
		src = d_flat + first_row * L;
	} else if (hd.model == Q_STORED) src = d_in + QHEADER_BYTES + first_row * L;
	else {
		// every table and run length is judged as ever; a kernel runs over the touched segments only
		const uint64_t seg0 = count ? first_row / hd.rps : 0, seg1 = count ? (first_row + count - 1) / hd.rps + 1 : 0;
		uint64_t img_bytes = (seg1 - seg0) * (uint64_t)hd.rps * L;
		if (seg1 && raw - seg0 * (uint64_t)hd.rps * L < img_bytes) img_bytes = raw - seg0 * (uint64_t)hd.rps * L;
		uint8_t *d_img = nullptr;
		MCOM_HIP(ctx, B.get(&d_img, img_bytes));
		if ((rc = decode_segments(ctx, B, hd, d_in, seg0, seg1, d_img, "qual_decode_rows"))) { if (rc == MCOM_E_ARG) { *n_rows = 0; *L_out = 0; } return rc; }
		src = d_img + (first_row - seg0 * hd.rps) * L;
	}
	if (count) MCOM_HIP(ctx, hipMemcpy2DAsync(d_rows, pitch, src, L, L, count, hipMemcpyDeviceToDevice, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}

// ---- test hook (include/mcom_test.h) ------------------------------------------------------------------------------------------------
extern "C" int mcom_test_qual_hist(mcom_ctx *ctx, const uint8_t *d_rows, uint64_t n_rows, uint32_t L, uint64_t pitch, uint8_t *h_map, uint32_t *h_A, uint64_t *d_counts)
{
	if (!ctx) return MCOM_E_ARG;
	if (!d_rows || !n_rows || !h_map || !h_A || !args_ok(n_rows, L, pitch)) return mcom_fail(ctx, MCOM_E_ARG, "test_qual_hist: null pointer, no rows or a shape outside the coder's");
	Blocks B(ctx);
	int rc = launch_alphabet(ctx, B, d_rows, n_rows, L, pitch, h_map);
	if (rc) return rc;
	Geometry g; g.set(h_map, L);
	*h_A = g.A;
	if (!d_counts) return MCOM_OK;
	uint8_t *d_tabs = nullptr;
	if ((rc = upload_tabs(ctx, B, g, &d_tabs))) return rc;
	if ((rc = launch_hist(ctx, d_rows, n_rows, L, pitch, g, d_tabs, (unsigned long long*)d_counts))) return rc;
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}

// ---- FASTQ text <-> rows (the two ends of `minicom -Q`) --------------------------------------------------------------------------------
//   k_fastq_quality_rows  sixteen lanes per record: lines 4r .. 4r + 3 of a line index; the record is checked ('@', '+', both lengths,
//                         every quality byte in 33 .. 126) and line 4r + 3 copied to row first_record + r
//   k_fastq_emit          sixteen lanes per record: `@<i+1>\n<read>\n+\n<qual>\n` at the record's offset, which has a closed form in
//                         the digit counts of the names (no scan)
// the digits of the names 1 .. m together
__host__ __device__ static inline uint64_t qv_digit_sum(uint64_t m)
{
	if (!m) return 0;
	uint64_t s = 0, p = 1, d = 1;
	while (p * 10 <= m) { s += 9 * p * d; p *= 10; ++d; }
	return s + (m - p + 1) * d;
}

__global__ __launch_bounds__(QV_THREADS) void k_fastq_quality_rows(const uint8_t *__restrict__ text, uint64_t n_bytes, const uint64_t *__restrict__ start, uint64_t first_record,
                                                                   uint64_t n_records, uint32_t L, uint8_t *__restrict__ rows, uint64_t pitch, uint32_t *__restrict__ flag)
{
	const uint64_t r = ((uint64_t)blockIdx.x * QV_THREADS + threadIdx.x) >> 4;
	const uint32_t lane = threadIdx.x & 15;
	if (r >= n_records) return;
	const uint64_t a = start[4 * r], b = start[4 * r + 1], c = start[4 * r + 2], d = start[4 * r + 3], e = start[4 * r + 4];
	uint32_t bad = 0;
	if (!(a < b && b < c && c < d && d < e && e <= n_bytes)) bad = MCOM_FASTQ_F_LENGTH;     // (cannot be: the index is made of this text)
	else {
		if (b - 1 - a < 1 || text[a] != '@') bad |= MCOM_FASTQ_F_NAME;
		if (d - 1 - c < 1 || text[c] != '+') bad |= MCOM_FASTQ_F_PLUS;
		if (c - 1 - b != L || e - 1 - d != L) bad |= MCOM_FASTQ_F_LENGTH;
	}
	if (!bad) {
		uint8_t *row = rows + (first_record + r) * pitch;
		for (uint32_t j = lane; j < L; j += 16) {
			const uint8_t v = text[d + j];
			if (v < 33 || v > 126) bad |= MCOM_FASTQ_F_CHAR; else row[j] = v;
		}
	}
	if (bad) { atomicOr(&flag[0], bad); atomicMin(&flag[1], (uint32_t)(first_record + r)); }
}

__global__ __launch_bounds__(QV_THREADS) void k_fastq_emit(const uint8_t *__restrict__ reads, uint64_t read_pitch, const uint8_t *__restrict__ quals, uint64_t qual_pitch,
                                                           uint64_t first, uint64_t count, uint32_t L, uint64_t digits_before, uint8_t *__restrict__ out)
{
	const uint64_t r = ((uint64_t)blockIdx.x * QV_THREADS + threadIdx.x) >> 4;
	const uint32_t lane = threadIdx.x & 15;
	if (r >= count) return;
	const uint64_t name = first + r + 1;
	uint32_t nd = 1;
	for (uint64_t v = name; v >= 10; v /= 10) ++nd;
	uint8_t *o = out + r * (2 * (uint64_t)L + 6) + (qv_digit_sum(first + r) - digits_before);
	if (lane == 0) {
		o[0] = '@';
		uint64_t v = name;
		for (uint32_t k = nd; k > 0; --k) { o[k] = (uint8_t)('0' + v % 10); v /= 10; }
		o[1 + nd] = '\n';
	}
	o += 2 + nd;
	const uint8_t *rd = reads + r * read_pitch, *ql = quals + r * qual_pitch;
	for (uint32_t j = lane; j < L; j += 16) { o[j] = rd[j]; o[L + 3 + j] = ql[j]; }
	if (lane == 0) { o[L] = '\n'; o[L + 1] = '+'; o[L + 2] = '\n'; o[2 * L + 3] = '\n'; }
}

extern "C" int mcom_fastq_quality_rows(mcom_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_line_start, uint64_t first_record, uint64_t n_records, uint32_t L,
                                       uint8_t *d_rows, uint64_t pitch, uint32_t *d_flag)
{
	if (!ctx) return MCOM_E_ARG;
	if (!d_flag || (n_records && (!d_text || !d_line_start || !d_rows))) return mcom_fail(ctx, MCOM_E_ARG, "fastq_quality_rows: null pointer");
	if (L < 1 || L > L_MAX || pitch < L || first_record + n_records >= ((uint64_t)1 << 32)) return mcom_fail(ctx, MCOM_E_ARG, "fastq_quality_rows: L %u, pitch %llu, %llu records from %llu",
	                                                                                                    L, (unsigned long long)pitch, (unsigned long long)n_records, (unsigned long long)first_record);
	if (!n_records) return MCOM_OK;
	MCOM_LAUNCH(k_fastq_quality_rows, dim3(blocks_for(n_records * 16)), dim3(QV_THREADS), 0, ctx->stream, d_text, n_bytes, d_line_start, first_record, n_records, L, d_rows, pitch, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}

extern "C" int mcom_fastq_emit(mcom_ctx *ctx, const uint8_t *d_reads, uint64_t read_pitch, const uint8_t *d_quals, uint64_t qual_pitch, uint64_t first, uint64_t count, uint32_t L,
                               uint8_t *d_out, uint64_t *bytes)
{
	if (!ctx) return MCOM_E_ARG;
	if (!bytes) return mcom_fail(ctx, MCOM_E_ARG, "fastq_emit: null pointer");
	*bytes = 0;
	if (L < 1 || L > L_MAX || read_pitch < L || qual_pitch < L || first + count >= ((uint64_t)1 << 32)) return mcom_fail(ctx, MCOM_E_ARG, "fastq_emit: L %u, %llu records from %llu",
	                                                                                                    L, (unsigned long long)count, (unsigned long long)first);
	const uint64_t before = qv_digit_sum(first);
	*bytes = count * (2 * (uint64_t)L + 6) + qv_digit_sum(first + count) - before;
	if (!d_out || !count) return MCOM_OK;
	if (!d_reads || !d_quals) { *bytes = 0; return mcom_fail(ctx, MCOM_E_ARG, "fastq_emit: null pointer"); }
	MCOM_LAUNCH(k_fastq_emit, dim3(blocks_for(count * 16)), dim3(QV_THREADS), 0, ctx->stream, d_reads, read_pitch, d_quals, qual_pitch, first, count, L, before, d_out);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}

// ---- rows through an order ------------------------------------------------------------------------------------
// seen: one bit per source row, cleared by the caller.  A row named twice is still copied (it lies inside the table); an index outside
// the table is not followed.
__global__ __launch_bounds__(QV_THREADS) void k_qual_gather(const uint8_t *__restrict__ rows, uint64_t n_src, uint32_t L, uint64_t pitch_in, const uint32_t *__restrict__ order,
                                                            uint64_t n_rows, uint8_t *__restrict__ out, uint64_t pitch_out, uint32_t *__restrict__ seen, uint32_t *__restrict__ flag)
{
	const uint64_t j = ((uint64_t)blockIdx.x * QV_THREADS + threadIdx.x) >> 4;
	const int lane = threadIdx.x & 15;
	if (j >= n_rows) return;                                                // (all sixteen lanes of a row together)
	const uint64_t s = order[j];
	if (s >= n_src) { if (lane == 0) atomicOr(flag, (uint32_t)MCOM_GATHER_F_BOUNDS); return; }
	if (lane == 0) {
		const uint32_t bit = 1u << (s & 31);
		if (atomicOr(seen + (s >> 5), bit) & bit) atomicOr(flag, (uint32_t)MCOM_GATHER_F_DUP);
	}
	const uint8_t *src = rows + s * pitch_in;
	uint8_t *dst = out + j * pitch_out;
	const int lead = (int)(((uintptr_t)dst) & 15), iL = (int)L;
	const int n_pieces = (lead + iL + 15) >> 4;                             // at most 17: L <= 256
	for (int k = lane; k < n_pieces; k += 16) {
		const int at = k * 16 - lead;
		if (at >= 0 && at + 16 <= iL) {
			uint4 v;
			__builtin_memcpy(&v, src + at, 16);                             // (any address: the bytes [at, at + 16) of the source row, nothing else)
			*(uint4*)(dst + at) = v;
		} else {
			const int b = at < 0 ? 0 : at, e = at + 16 < iL ? at + 16 : iL;
			for (int i = b; i < e; ++i) dst[i] = src[i];
		}
	}
}

extern "C" int mcom_qual_gather_rows(mcom_ctx *ctx, const uint8_t *d_rows, uint64_t n_src, uint32_t L, uint64_t pitch_in, const uint32_t *d_order, uint64_t n_rows,
                                     uint8_t *d_out, uint64_t pitch_out, uint32_t *d_flag)
{
	if (!ctx) return MCOM_E_ARG;
	if (!d_flag || (n_rows && (!d_order || !d_out)) || (n_src && !d_rows)) return mcom_fail(ctx, MCOM_E_ARG, "qual_gather_rows: null pointer");
	if (L < 1 || L > L_MAX || pitch_in < L || pitch_out < L || n_src >= ((uint64_t)1 << 32) || n_rows >= ((uint64_t)1 << 32))
		return mcom_fail(ctx, MCOM_E_ARG, "qual_gather_rows: L %u, pitches %llu and %llu, %llu rows out of %llu (L 1 .. 256, pitches >= L, below 2^32 rows)", L,
		                 (unsigned long long)pitch_in, (unsigned long long)pitch_out, (unsigned long long)n_rows, (unsigned long long)n_src);
	if (!n_rows) return MCOM_OK;
	Blocks B(ctx);
	uint32_t *d_seen = nullptr;
	const size_t seen_bytes = (size_t)((n_src + 31) / 32) * 4;
	MCOM_HIP(ctx, B.get(&d_seen, seen_bytes));
	if (seen_bytes) MCOM_HIP(ctx, hipMemsetAsync(d_seen, 0, seen_bytes, ctx->stream));
	MCOM_LAUNCH(k_qual_gather, dim3(blocks_for(n_rows * 16)), dim3(QV_THREADS), 0, ctx->stream, d_rows, n_src, L, pitch_in, d_order, n_rows, d_out, pitch_out, d_seen, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}
