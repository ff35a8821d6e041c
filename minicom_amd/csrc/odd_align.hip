// minicom_amd/csrc/odd_align.hip -- the odd reads of a -V archive coded against the contigs (`minicom -p -V -A`).
//
// The rule and the member are stated in odd_align_model.hpp, which the plain C++ twins (host/mcom_odd_align.cpp) share: the same hits, the
// same member bytes, the same refusals.
//
//   k_oa_text_append   `bases` bases of a ref.bin image behind base `at` of the packed text T: one thread per 64-bit word of T
//   k_oa_grid          the seed grid: (key of T[q, q + K), q) for every q = 8 g, then the project's radix sort by key
//   k_oa_align         the search.  One wave per read: both orientations staged 2 bits per base in LDS beside their N masks; the lanes take
//                      the (strand, offset) pairs, look the 48-bit seed up by binary search over the sorted grid, verify every candidate
//                      on packed words (XOR, fold, OR the N mask, popcount; T's window by a funnel shift) and keep their smallest hit
//                      word; the wave's smallest by shuffles.  No atomics on global memory.
//   k_oa_enc_marks     per odd record: the hit word checked against the text and T; 1 / d / the length for the three scans
//   k_oa_enc_write     per odd record (sixteen lanes): p, d, strand and mismatches to their places, or the read to the residual
//   k_oa_bits          eight marks to one byte of a bit array
//   k_oa_dec_marks     per odd record of an untrusted member: its aligned bit and what it takes of the residual; per aligned record: d
//   k_oa_dec_write     per odd record (sixteen lanes): the window with its mismatches, or the read out of the residual
// Untrusted members never take a kernel outside its buffers: flag and skip.
#include "mcom_dev.hpp"
#include "odd_align_model.hpp"
#include <cstring>

#define OA_THREADS 256
#define OA_WAVES (OA_THREADS / 64)
#define OA_LANES 16                                         // lanes per record of the writing passes
#define OA_RWORDS (OA_MAX_LEN / 32 + 1)                      // words of a staged read: 256 bases and a word of zeros for the funnel shift

struct mcom_odd_index { mcom_mm128 *d_grid; uint64_t n; };

namespace {
struct Blocks {                                             // pooled device blocks of one call, back to the pool once the stream has passed them
	mcom_ctx *ctx; std::vector<void*> v;
	explicit Blocks(mcom_ctx *c) : ctx(c) {}
	~Blocks() { for (void *p : v) mcom_dfree_later(ctx, p); }
	template <class T> hipError_t get(T **out, size_t bytes) { hipError_t e = mcom_dmalloc((void**)out, bytes ? bytes : 16); if (e == hipSuccess) v.push_back(*out); return e; }
};
unsigned blocks_for(uint64_t items) { return (unsigned)((items + OA_THREADS - 1) / OA_THREADS); }
const uint64_t OA_MAX_RECORDS = (uint64_t)1 << 32;
}  // namespace

// ---- T -------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OA_THREADS) void k_oa_text_append(unsigned long long *__restrict__ t, uint64_t at, const uint8_t *__restrict__ ref, uint64_t bases)
{
	const uint64_t w = (at >> 5) + (uint64_t)blockIdx.x * OA_THREADS + threadIdx.x;     // the word of T this thread fills its share of
	if (w > ((at + bases - 1) >> 5)) return;
	const uint64_t b0 = w * 32 > at ? w * 32 : at, b1 = (w + 1) * 32 < at + bases ? (w + 1) * 32 : at + bases;
	uint64_t v = 0;
	for (uint64_t b = b0; b < b1; ++b) { const uint64_t i = b - at; v |= (uint64_t)((ref[i >> 2] >> (2 * (i & 3))) & 3u) << (2 * (b & 31)); }
	// the first and the last word of a set may be shared with its neighbours (another call): everything else is this thread's alone
	if (b0 == w * 32 && b1 == (w + 1) * 32) t[w] = v; else atomicOr(&t[w], (unsigned long long)v);
}

extern "C" int mcom_odd_text_append(mcom_ctx *ctx, uint64_t *d_t, uint64_t t_words, uint64_t at, const uint8_t *d_ref, uint64_t ref_bytes, uint64_t bases)
{
	if (!ctx) return MCOM_E_ARG;
	if (!bases) return MCOM_OK;
	if (!d_t || !d_ref || bases > 4 * ref_bytes || at + bases >= OA_MAX_T || oa_words(at + bases) > t_words)
		return mcom_fail(ctx, MCOM_E_ARG, "odd_text_append: %llu bases at %llu of a text of %llu words, from %llu bytes", (unsigned long long)bases, (unsigned long long)at,
		                 (unsigned long long)t_words, (unsigned long long)ref_bytes);
	MCOM_LAUNCH(k_oa_text_append, dim3(blocks_for(((at + bases - 1) >> 5) - (at >> 5) + 1)), dim3(OA_THREADS), 0, ctx->stream, (unsigned long long*)d_t, at, d_ref, bases);
	MCOM_LAUNCH_CHECK(ctx);
	return MCOM_OK;
}

// ---- the grid ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OA_THREADS) void k_oa_grid(const uint64_t *__restrict__ t, uint64_t n, mcom_mm128 *__restrict__ grid)
{
	const uint64_t g = (uint64_t)blockIdx.x * OA_THREADS + threadIdx.x;
	if (g >= n) return;
	mcom_mm128 e; e.x = oa_key(t, g * OA_G); e.y = g * OA_G;
	grid[g] = e;
}

extern "C" int mcom_odd_index_build(mcom_ctx *ctx, const uint64_t *d_t, uint64_t t_bases, mcom_odd_index **idx)
{
	if (!ctx) return MCOM_E_ARG;
	if (!idx || (t_bases && !d_t)) return mcom_fail(ctx, MCOM_E_ARG, "odd_index_build: null pointer");
	*idx = nullptr;
	if (t_bases >= OA_MAX_T) return mcom_fail(ctx, MCOM_E_ARG, "odd_index_build: a text of %llu bases (below 2^40)", (unsigned long long)t_bases);
	const uint64_t n = oa_grid_size(t_bases);
	if (n >= OA_MAX_RECORDS) return mcom_fail(ctx, MCOM_E_OVERFLOW, "odd_index_build: %llu grid entries, the sort takes fewer than 2^32", (unsigned long long)n);
	size_t fr = 0, tot = 0;
	MCOM_HIP(ctx, hipMemGetInfo(&fr, &tot));
	if (n * 16 + mcom_sort_ws_bytes(n) + ((size_t)16 << 20) > fr)
		return mcom_fail(ctx, MCOM_E_OVERFLOW, "odd_index_build: %llu grid entries of 16 bytes and their sort do not fit the card (%zu bytes free)", (unsigned long long)n, fr);
	mcom_odd_index *X = new mcom_odd_index{nullptr, n};
	if (n) {
		if (hipMalloc((void**)&X->d_grid, n * 16) != hipSuccess) { delete X; return mcom_fail(ctx, MCOM_E_OVERFLOW, "odd_index_build: no room for %llu grid entries", (unsigned long long)n); }
		MCOM_LAUNCH(k_oa_grid, dim3(blocks_for(n)), dim3(OA_THREADS), 0, ctx->stream, d_t, n, X->d_grid);
		int rc = hipGetLastError() == hipSuccess ? mcom_radix_sort_128x(ctx, X->d_grid, n) : mcom_fail(ctx, MCOM_E_HIP, "odd_index_build: launch failed");
		if (!rc && mcom_stream_sync(ctx) != hipSuccess) rc = mcom_fail(ctx, MCOM_E_HIP, "odd_index_build: the sort failed");
		if (rc) { (void)hipFree(X->d_grid); delete X; return rc; }
	}
	*idx = X;
	return MCOM_OK;
}
extern "C" void mcom_odd_index_free(mcom_ctx *ctx, mcom_odd_index *idx)
{
	if (!idx) return;
	if (ctx) (void)mcom_stream_sync(ctx);
	if (idx->d_grid) (void)hipFree(idx->d_grid);
	delete idx;
}
extern "C" uint64_t mcom_odd_index_size(const mcom_odd_index *idx) { return idx ? idx->n : 0; }
extern "C" int mcom_odd_index_copy(mcom_ctx *ctx, const mcom_odd_index *idx, mcom_mm128 *d_out)
{
	if (!ctx) return MCOM_E_ARG;
	if (!idx || (idx->n && !d_out)) return mcom_fail(ctx, MCOM_E_ARG, "odd_index_copy: null pointer");
	if (idx->n) MCOM_HIP(ctx, hipMemcpyAsync(d_out, idx->d_grid, idx->n * sizeof(mcom_mm128), hipMemcpyDeviceToDevice, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}

// ---- the search ----------------------------------------------------------------------------------------------------------------------------
// the 32 bases from base `at` of a staged read (LDS): OA_RWORDS words, the last one zero
__device__ __forceinline__ uint64_t oa_lds_window(const uint64_t *w, uint32_t at)
{
	const uint32_t i = at >> 5, sh = 2u * (at & 31);
	return sh ? (w[i] >> sh) | (w[i + 1] << (64 - sh)) : w[i];
}

__global__ __launch_bounds__(OA_THREADS) void k_oa_align(const mcom_mm128 *__restrict__ grid, uint64_t n_grid, const uint64_t *__restrict__ t, uint64_t t_bases,
                                                         const uint8_t *__restrict__ odd, const uint64_t *__restrict__ off, uint64_t n_odd, uint64_t *__restrict__ hits)
{
	__shared__ uint64_t s_read[OA_WAVES][2][OA_RWORDS], s_nmask[OA_WAVES][2][OA_RWORDS];
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const uint64_t r = (uint64_t)blockIdx.x * OA_WAVES + wave;
	// (every thread of the block reaches both barriers: a wave without a read has l = 0)
	uint64_t at = 0; uint32_t l = 0;
	if (r < n_odd) {
		at = off[r];
		const uint64_t e = off[r + 1];
		l = e >= at && e - at <= OA_MAX_LEN ? (uint32_t)(e - at) : 0;
	}
	if (l < OA_MIN_LEN || l > t_bases) l = 0;                                  // never aligned: costs a store
	if (lane < 2 * OA_RWORDS) { (&s_read[wave][0][0])[lane] = 0; (&s_nmask[wave][0][0])[lane] = 0; }
	__syncthreads();
	for (uint32_t j = lane; j < l; j += 64) {
		const uint32_t c = oa_code(odd[at + j]), k = l - 1 - j;               // base j of the read is base k of its reverse complement
		if (c < 4) {
			atomicOr((unsigned long long*)&s_read[wave][0][j >> 5], (unsigned long long)c << (2 * (j & 31)));
			atomicOr((unsigned long long*)&s_read[wave][1][k >> 5], (unsigned long long)(3u - c) << (2 * (k & 31)));
		} else {                                                               // N (or a byte the caller should not have sent): differs from every base
			atomicOr((unsigned long long*)&s_nmask[wave][0][j >> 5], 1ull << (2 * (j & 31)));
			atomicOr((unsigned long long*)&s_nmask[wave][1][k >> 5], 1ull << (2 * (k & 31)));
		}
	}
	__syncthreads();
	uint64_t best = OA_NONE;
	if (l) {
		const uint32_t n_off = l - OA_K + 1, E = oa_budget(l), n_words = (l + 31) / 32;
		for (uint32_t it = lane; it < 2 * n_off; it += 64) {
			const uint32_t s = it >= n_off, o = s ? it - n_off : it;
			const uint64_t *rd = s_read[wave][s], *nm = s_nmask[wave][s];
			if (oa_lds_window(nm, o) & OA_KEY_MASK) continue;                  // an N inside the seed
			const uint64_t key = oa_lds_window(rd, o) & OA_KEY_MASK;
			uint64_t lo = 0, hi = n_grid;                                      // the first entry whose key is not below
			while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (grid[mid].x < key) lo = mid + 1; else hi = mid; }
			uint32_t run = 0;
			while (run <= OA_M && lo + run < n_grid && grid[lo + run].x == key) ++run;
			if (run > OA_M) continue;                                          // a repeat: ignored entirely
			for (uint32_t c = 0; c < run; ++c) {
				const uint64_t q = grid[lo + c].y;
				if (q < o) continue;
				const uint64_t p = q - o;
				if (p + l > t_bases) continue;
				uint32_t d = 0;
				for (uint32_t w = 0; w < n_words && d <= E; ++w) {
					uint64_t x = oa_diff32(rd[w], oa_window(t, p + 32 * w)) | nm[w];
					const uint32_t left = l - 32 * w;
					if (left < 32) x &= (1ull << (2 * left)) - 1;
					d += (uint32_t)__popcll(x);
				}
				if (d > E) continue;
				const uint64_t h = oa_hit(d, s, p);
				best = h < best ? h : best;
			}
		}
	}
#pragma unroll
	for (int o = 32; o; o >>= 1) { const uint64_t other = __shfl_xor(best, o, 64); best = other < best ? other : best; }
	if (lane == 0 && r < n_odd) hits[r] = best;
}

extern "C" int mcom_odd_align(mcom_ctx *ctx, const mcom_odd_index *idx, const uint64_t *d_t, uint64_t t_bases, const uint8_t *d_odd, const uint64_t *d_off, uint64_t n_odd, uint64_t *d_hits)
{
	if (!ctx) return MCOM_E_ARG;
	if (!idx || !d_off || (n_odd && !d_hits) || (t_bases && !d_t)) return mcom_fail(ctx, MCOM_E_ARG, "odd_align: null pointer");
	if (t_bases >= OA_MAX_T || n_odd >= OA_MAX_RECORDS || idx->n != oa_grid_size(t_bases))
		return mcom_fail(ctx, MCOM_E_ARG, "odd_align: %llu records, a text of %llu bases, an index of %llu entries", (unsigned long long)n_odd, (unsigned long long)t_bases, (unsigned long long)idx->n);
	if (!n_odd) return MCOM_OK;
	MCOM_LAUNCH(k_oa_align, dim3((unsigned)((n_odd + OA_WAVES - 1) / OA_WAVES)), dim3(OA_THREADS), 0, ctx->stream, (const mcom_mm128*)idx->d_grid, idx->n, d_t, t_bases, d_odd, d_off, n_odd, d_hits);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}

// ---- bit arrays ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OA_THREADS) void k_oa_bits(const uint8_t *__restrict__ mark, uint64_t n, uint8_t *__restrict__ bits)
{
	const uint64_t b = (uint64_t)blockIdx.x * OA_THREADS + threadIdx.x;
	if (b >= (n + 7) / 8) return;
	uint32_t v = 0;
	for (uint32_t k = 0; k < 8 && 8 * b + k < n; ++k) v |= (uint32_t)(mark[8 * b + k] != 0) << k;
	bits[b] = (uint8_t)v;
}

// ---- the encoder ---------------------------------------------------------------------------------------------------------------------------
struct OaRead { uint64_t at; uint32_t l; bool ok; };
__device__ __forceinline__ OaRead oa_read_of(const uint64_t *off, uint64_t r)
{
	OaRead R; R.at = off[r];
	const uint64_t e = off[r + 1];
	R.ok = e >= R.at && e - R.at <= OA_MAX_LEN; R.l = R.ok ? (uint32_t)(e - R.at) : 0;
	return R;
}

// entry n_odd of the three arrays is zero: the exclusive scans leave the totals there
__global__ __launch_bounds__(OA_THREADS) void k_oa_enc_marks(const uint64_t *__restrict__ hits, const uint8_t *__restrict__ odd, const uint64_t *__restrict__ off, uint64_t n_odd,
                                                             const uint64_t *__restrict__ t, uint64_t t_bases, uint64_t *__restrict__ a, uint64_t *__restrict__ m, uint64_t *__restrict__ res,
                                                             uint8_t *__restrict__ mark, uint32_t *__restrict__ flag)
{
	const uint64_t r = (uint64_t)blockIdx.x * OA_THREADS + threadIdx.x;
	if (r > n_odd) return;
	uint64_t va = 0, vm = 0, vr = 0;
	if (r < n_odd) {
		const OaRead R = oa_read_of(off, r);
		const uint64_t h = hits[r];
		bool bad = !R.ok;
		for (uint32_t j = 0; j < R.l; ++j) bad |= oa_code(odd[R.at + j]) > 4;
		if (!bad && h != OA_NONE) {
			const uint64_t p = oa_hit_p(h);
			const uint32_t d = oa_hit_d(h), s = oa_hit_s(h);
			if (h != oa_hit(d, s, p) || R.l < OA_MIN_LEN || p > t_bases || R.l > t_bases - p || d > oa_budget(R.l) || oa_encode_read(t, odd + R.at, R.l, s, p, nullptr, nullptr) != d) bad = true;
			else { va = 1; vm = d; }
		} else vr = R.l;
		if (bad) { atomicOr(flag, 1u); va = vm = vr = 0; }
		mark[r] = (uint8_t)va;
	}
	a[r] = va; m[r] = vm; res[r] = vr;
}

__global__ __launch_bounds__(OA_THREADS) void k_oa_enc_write(const uint64_t *__restrict__ hits, const uint8_t *__restrict__ odd, const uint64_t *__restrict__ off, uint64_t n_odd,
                                                             const uint64_t *__restrict__ t, const uint64_t *__restrict__ a, const uint64_t *__restrict__ m, const uint64_t *__restrict__ res,
                                                             OaLayout Y, uint64_t res_bytes, uint8_t *__restrict__ member, uint8_t *__restrict__ strand, uint8_t *__restrict__ residual)
{
	const uint64_t r = ((uint64_t)blockIdx.x * OA_THREADS + threadIdx.x) / OA_LANES;
	const uint32_t lane = threadIdx.x % OA_LANES;
	if (r >= n_odd) return;
	const OaRead R = oa_read_of(off, r);
	const uint64_t h = hits[r];
	if (h == OA_NONE) {
		const uint64_t to = res[r];
		if (to > res_bytes || R.l > res_bytes - to) return;                    // (cannot be: the sizes are the scans of these lengths)
		for (uint32_t j = lane; j < R.l; j += OA_LANES) residual[to + j] = odd[R.at + j];
		return;
	}
	if (lane) return;                                                          // the mismatch list is a serial walk
	const uint64_t k = a[r], mm = m[r], p = oa_hit_p(h);
	const uint32_t d = oa_hit_d(h), s = oa_hit_s(h);
	if (k >= Y.n_aligned || mm > Y.n_mm || d > Y.n_mm - mm) return;
	strand[k] = (uint8_t)s;
	for (int b = 0; b < 5; ++b) member[Y.p + (uint64_t)b * Y.n_aligned + k] = (uint8_t)(p >> (8 * b));
	member[Y.d + k] = (uint8_t)d;
	oa_encode_read(t, odd + R.at, R.l, s, p, member + Y.mm_off + mm, member + Y.mm_base + mm);
}

extern "C" int mcom_odd_align_encode(mcom_ctx *ctx, const uint64_t *d_hits, const uint8_t *d_odd, const uint64_t *d_off, uint64_t n_odd, const uint64_t *d_t, uint64_t t_bases,
                                     uint8_t *d_member, uint64_t member_cap, uint64_t *member_len, uint8_t *d_residual, uint64_t res_cap, uint64_t *res_len)
{
	if (!ctx) return MCOM_E_ARG;
	if (!d_off || !member_len || !res_len || (n_odd && !d_hits) || (t_bases && !d_t)) return mcom_fail(ctx, MCOM_E_ARG, "odd_align_encode: null pointer");
	*member_len = *res_len = 0;
	if (t_bases >= OA_MAX_T || n_odd >= OA_MAX_RECORDS) return mcom_fail(ctx, MCOM_E_ARG, "odd_align_encode: %llu records, a text of %llu bases", (unsigned long long)n_odd, (unsigned long long)t_bases);
	Blocks B(ctx);
	uint64_t *d_a = nullptr, *d_m = nullptr, *d_r = nullptr, odd_bytes = 0, tot[3] = {0, 0, 0};
	uint8_t *d_mark = nullptr, *d_strand = nullptr;
	uint32_t *d_flag = nullptr, flag = 0;
	MCOM_HIP(ctx, B.get(&d_a, (n_odd + 1) * 8));
	MCOM_HIP(ctx, B.get(&d_m, (n_odd + 1) * 8));
	MCOM_HIP(ctx, B.get(&d_r, (n_odd + 1) * 8));
	MCOM_HIP(ctx, B.get(&d_mark, n_odd));
	MCOM_HIP(ctx, B.get(&d_flag, 4));
	MCOM_HIP(ctx, hipMemsetAsync(d_flag, 0, 4, ctx->stream));
	MCOM_LAUNCH(k_oa_enc_marks, dim3(blocks_for(n_odd + 1)), dim3(OA_THREADS), 0, ctx->stream, d_hits, d_odd, d_off, n_odd, d_t, t_bases, d_a, d_m, d_r, d_mark, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	int rc;
	if ((rc = mcom_scan_u64(ctx, d_a, d_a, n_odd + 1)) || (rc = mcom_scan_u64(ctx, d_m, d_m, n_odd + 1)) || (rc = mcom_scan_u64(ctx, d_r, d_r, n_odd + 1))) return rc;
	MCOM_HIP(ctx, hipMemcpyAsync(&tot[0], d_a + n_odd, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(&tot[1], d_m + n_odd, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(&tot[2], d_r + n_odd, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(&odd_bytes, d_off + n_odd, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	if (flag) return mcom_fail(ctx, MCOM_E_ARG, "odd_align_encode: a hit word that its read and the text do not bear out, or a text outside ACGTN");
	if (!tot[0]) {                                                             // no member: the residual is the text
		*res_len = odd_bytes;
		if (!d_residual) return MCOM_OK;
		if (odd_bytes > res_cap) return mcom_fail(ctx, MCOM_E_OVERFLOW, "odd_align_encode: a residual of %llu bytes, room for %llu", (unsigned long long)odd_bytes, (unsigned long long)res_cap);
		if (odd_bytes) MCOM_HIP(ctx, hipMemcpyAsync(d_residual, d_odd, odd_bytes, hipMemcpyDeviceToDevice, ctx->stream));
		MCOM_HIP(ctx, mcom_stream_sync(ctx));
		return MCOM_OK;
	}
	const OaLayout Y = oa_layout(n_odd, tot[0], tot[1]);
	*member_len = Y.total; *res_len = tot[2];
	if (!d_member) return MCOM_OK;
	if (Y.total > member_cap || tot[2] > res_cap || (tot[2] && !d_residual))
		return mcom_fail(ctx, MCOM_E_OVERFLOW, "odd_align_encode: a member of %llu and a residual of %llu bytes, room for %llu and %llu", (unsigned long long)Y.total, (unsigned long long)tot[2],
		                 (unsigned long long)member_cap, (unsigned long long)res_cap);
	OaHeader H;
	H.K = OA_K; H.G = OA_G; H.M = OA_M; H.n_odd = n_odd; H.n_aligned = tot[0]; H.t_bases = t_bases; H.n_mm = tot[1]; H.residual = tot[2];
	if ((rc = mcom_device_crc32(ctx, d_odd, odd_bytes, &H.crc))) return rc;
	uint8_t head[OA_HEADER];
	oa_header_put(head, H);
	MCOM_HIP(ctx, B.get(&d_strand, Y.n_aligned));
	MCOM_HIP(ctx, hipMemcpyAsync(d_member, head, OA_HEADER, hipMemcpyHostToDevice, ctx->stream));
	MCOM_LAUNCH(k_oa_enc_write, dim3(blocks_for(n_odd * OA_LANES)), dim3(OA_THREADS), 0, ctx->stream, d_hits, d_odd, d_off, n_odd, d_t, (const uint64_t*)d_a, (const uint64_t*)d_m,
	            (const uint64_t*)d_r, Y, tot[2], d_member, d_strand, d_residual);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_LAUNCH(k_oa_bits, dim3(blocks_for((n_odd + 7) / 8)), dim3(OA_THREADS), 0, ctx->stream, (const uint8_t*)d_mark, n_odd, d_member + Y.aligned);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_LAUNCH(k_oa_bits, dim3(blocks_for((Y.n_aligned + 7) / 8)), dim3(OA_THREADS), 0, ctx->stream, (const uint8_t*)d_strand, Y.n_aligned, d_member + Y.strand);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, mcom_stream_sync(ctx));                                       // (head lives on this frame)
	return MCOM_OK;
}

// ---- the decoder: the member is untrusted ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t oa_bit(const uint8_t *bits, uint64_t i) { return (bits[i >> 3] >> (i & 7)) & 1u; }

// per odd record: 1 / what it takes of the residual; per aligned record: d.  Entries n_odd and n_aligned are zero.  The unused high bits of
// the two bit arrays must be zero.
__global__ __launch_bounds__(OA_THREADS) void k_oa_dec_marks(const uint8_t *__restrict__ member, OaLayout Y, const uint64_t *__restrict__ off, uint64_t *__restrict__ a,
                                                             uint64_t *__restrict__ res, uint64_t *__restrict__ m, uint32_t *__restrict__ flag)
{
	const uint64_t r = (uint64_t)blockIdx.x * OA_THREADS + threadIdx.x;
	if (r <= Y.n_odd) {
		uint64_t va = 0, vr = 0;
		if (r < Y.n_odd) {
			const OaRead R = oa_read_of(off, r);
			if (!R.ok) atomicOr(flag, 0x80000000u);                            // the caller's offsets, not the member
			if (oa_bit(member + Y.aligned, r)) va = 1; else vr = R.l;
		} else {
			if ((Y.n_odd & 7) && (member[Y.aligned + (Y.n_odd >> 3)] >> (Y.n_odd & 7))) atomicOr(flag, (uint32_t)OA_F_COUNT);
			if ((Y.n_aligned & 7) && (member[Y.strand + (Y.n_aligned >> 3)] >> (Y.n_aligned & 7))) atomicOr(flag, (uint32_t)OA_F_COUNT);
		}
		a[r] = va; res[r] = vr;
	}
	if (r <= Y.n_aligned) m[r] = r < Y.n_aligned ? member[Y.d + r] : 0;
}

__global__ __launch_bounds__(OA_THREADS) void k_oa_dec_write(const uint8_t *__restrict__ member, OaLayout Y, const uint64_t *__restrict__ t, uint64_t t_bases,
                                                             const uint8_t *__restrict__ residual, uint64_t res_bytes, const uint64_t *__restrict__ off, const uint64_t *__restrict__ a,
                                                             const uint64_t *__restrict__ res, const uint64_t *__restrict__ m, uint8_t *__restrict__ out, uint32_t *__restrict__ flag)
{
	const uint64_t r = ((uint64_t)blockIdx.x * OA_THREADS + threadIdx.x) / OA_LANES;
	const uint32_t lane = threadIdx.x % OA_LANES;
	if (r >= Y.n_odd) return;
	const OaRead R = oa_read_of(off, r);
	if (!R.ok) return;
	if (!oa_bit(member + Y.aligned, r)) {
		const uint64_t from = res[r];
		if (from > res_bytes || R.l > res_bytes - from) { if (lane == 0) atomicOr(flag, (uint32_t)OA_F_COUNT); return; }
		for (uint32_t j = lane; j < R.l; j += OA_LANES) out[R.at + j] = residual[from + j];
		return;
	}
	if (lane) return;                                                          // the mismatch list is a serial walk
	const uint64_t k = a[r];
	if (k >= Y.n_aligned) { atomicOr(flag, (uint32_t)OA_F_COUNT); return; }
	const uint64_t mm = m[k];
	const uint32_t d = member[Y.d + k];
	if (mm > Y.n_mm || d > Y.n_mm - mm) { atomicOr(flag, (uint32_t)OA_F_COUNT); return; }
	uint64_t p = 0;
	for (int b = 0; b < 5; ++b) p |= (uint64_t)member[Y.p + (uint64_t)b * Y.n_aligned + k] << (8 * b);
	const uint32_t f = oa_decode_read(t, t_bases, R.l, oa_bit(member + Y.strand, k), p, d, member + Y.mm_off + mm, member + Y.mm_base + mm, out + R.at);
	if (f) atomicOr(flag, f);
}

extern "C" int mcom_odd_align_decode(mcom_ctx *ctx, const uint8_t *d_member, uint64_t member_len, const uint64_t *d_t, uint64_t t_bases, const uint8_t *d_residual, uint64_t res_len,
                                     const uint64_t *d_off, uint64_t n_odd, uint64_t odd_bytes, uint8_t *d_out, uint32_t *flags)
{
	if (!ctx) return MCOM_E_ARG;
	if (!d_member || !d_off || !flags || (t_bases && !d_t) || (res_len && !d_residual) || (odd_bytes && !d_out)) return mcom_fail(ctx, MCOM_E_ARG, "odd_align_decode: null pointer");
	*flags = 0;
	if (n_odd >= OA_MAX_RECORDS || t_bases >= OA_MAX_T) return mcom_fail(ctx, MCOM_E_ARG, "odd_align_decode: %llu records, a text of %llu bases", (unsigned long long)n_odd, (unsigned long long)t_bases);
	auto refuse = [&](uint32_t f) { *flags = f; return mcom_fail(ctx, MCOM_E_ARG, "%s", oa_refusal(f)); };
	uint8_t head[OA_HEADER];
	memset(head, 0, sizeof head);
	const uint64_t head_len = member_len < OA_HEADER ? member_len : OA_HEADER;
	uint64_t last = 0;
	if (head_len) MCOM_HIP(ctx, hipMemcpyAsync(head, d_member, head_len, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(&last, d_off + n_odd, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	if (last != odd_bytes) return mcom_fail(ctx, MCOM_E_ARG, "odd_align_decode: the record offsets end at %llu, the text at %llu", (unsigned long long)last, (unsigned long long)odd_bytes);
	OaHeader H;
	const uint32_t hf = oa_header_check(head, member_len, n_odd, odd_bytes, t_bases, res_len, H);
	if (hf) return refuse(hf);
	const OaLayout Y = oa_layout(H.n_odd, H.n_aligned, H.n_mm);
	Blocks B(ctx);
	uint64_t *d_a = nullptr, *d_r = nullptr, *d_m = nullptr, tot[3] = {0, 0, 0};
	uint32_t *d_flag = nullptr, flag = 0;
	MCOM_HIP(ctx, B.get(&d_a, (n_odd + 1) * 8));
	MCOM_HIP(ctx, B.get(&d_r, (n_odd + 1) * 8));
	MCOM_HIP(ctx, B.get(&d_m, (Y.n_aligned + 1) * 8));
	MCOM_HIP(ctx, B.get(&d_flag, 4));
	MCOM_HIP(ctx, hipMemsetAsync(d_flag, 0, 4, ctx->stream));
	MCOM_LAUNCH(k_oa_dec_marks, dim3(blocks_for(n_odd + 1)), dim3(OA_THREADS), 0, ctx->stream, d_member, Y, d_off, d_a, d_r, d_m, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	int rc;
	if ((rc = mcom_scan_u64(ctx, d_a, d_a, n_odd + 1)) || (rc = mcom_scan_u64(ctx, d_r, d_r, n_odd + 1)) || (rc = mcom_scan_u64(ctx, d_m, d_m, Y.n_aligned + 1))) return rc;
	MCOM_HIP(ctx, hipMemcpyAsync(&tot[0], d_a + n_odd, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(&tot[1], d_m + Y.n_aligned, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(&tot[2], d_r + n_odd, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	if (flag & 0x80000000u) return mcom_fail(ctx, MCOM_E_ARG, "odd_align_decode: the record offsets do not ascend by 0 .. 256");
	if (tot[0] != H.n_aligned || tot[1] != H.n_mm || tot[2] != H.residual) flag |= OA_F_COUNT;
	if (flag) return refuse(flag);
	MCOM_LAUNCH(k_oa_dec_write, dim3(blocks_for(n_odd * OA_LANES)), dim3(OA_THREADS), 0, ctx->stream, d_member, Y, d_t, t_bases, d_residual, res_len, d_off, (const uint64_t*)d_a,
	            (const uint64_t*)d_r, (const uint64_t*)d_m, d_out, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	if (flag) return refuse(flag);
	uint32_t crc = 0;
	if ((rc = mcom_device_crc32(ctx, d_out, odd_bytes, &crc))) return rc;
	if (crc != H.crc) return refuse(OA_F_CRC);
	return MCOM_OK;
}
