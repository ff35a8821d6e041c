// minicom_amd/csrc/bwt.hip -- the block-sorting coder: `.bwt` members (format and checks: bwt_model.hpp; specification and cross-check:
// host/mcom_bwt.cpp).
//
// forward   k_bwt_rec0      one sort record per byte: x = block | byte + 1 | next byte + 1 (0 behind the block's end), y = position
//           (mcom_sort_by_x) the stable radix sort of sort.hip, only the passes the key's width asks for
//           k_bwt_flags     1 where a sorted record's key differs from the one in front of it; (mcom_scan_u32) makes group numbers of them
//           k_bwt_rank      rank[position] = group number (1-based, over all blocks: the block is the key's top part from round 0 on)
//           k_bwt_rec       the next round's records: x = rank[i] | rank[i + h] (0 behind the block's end)
//           ... until every group is one suffix (one read-back per round: the scan's total from the pinned ring), at most blk_log2 + 1 rounds
//           k_bwt_emit      one thread per position: the transformed byte of its row, the primary index, the anchors
// MTF       k_mtf_pass1     one lane per stretch of 2 KiB, list in LDS: the stretch's operations applied to the identity list
//           k_mtf_compose   one wave per block walks its stretches in order and leaves every stretch its start list
//           k_mtf_pass2     the same lanes code (decode) their stretch from that list
//           Coding moves SYMBOLS to the front, so a stretch's effect on any list is: its distinct symbols in order of last use, then
//           the list's other symbols in the order they had (pass 1 keeps the count of distinct symbols beside the list).  Decoding moves
//           POSITIONS, so its effect is a permutation and the lists compose as such.  Both are exact.
// inverse   k_bwt_tile_hist 256 counters in LDS per tile of 2 KiB, stored [block][byte][tile]: one scan over all of them gives, minus the
//           (mcom_scan_u32) block's first value, "bytes of the block below c + equal bytes in earlier tiles"
//           k_bwt_lf        one wave per tile, 64 bytes a step: equal bytes found by eight ballots; table[j] = byte << 24 | row that follows
//           k_bwt_walk      one workgroup per block, a lane per anchor stretch: a chain of dependent 4-byte loads over the block's table (4 MiB for 1 MiB of text)
// Untrusted input: header arithmetic, the embedded member's header and every index row are judged on the host before a launch; the walk
// raises the flag word and stops where a row is the one without a byte or no row of its block, and where a stretch does not end in the
// row the index gives for its start.  The table itself is made from the bytes and cannot point outside its block.
#include "mcom_dev.hpp"
#include "bwt_model.hpp"

using namespace mcom_bwt;

#define BW_THREADS 256
#define BW_LIST_PITCH 260                      // bytes of LDS per lane's list: 65 words, so that neighbouring lanes start on neighbouring banks
enum { BW_F_ROW = 1, BW_F_CHAIN = 2 };

__device__ __forceinline__ uint64_t bw_block_len(uint64_t n, uint64_t b, uint32_t blk_log2)
{
	const uint64_t at = b << blk_log2, blk = (uint64_t)1 << blk_log2;
	return n - at < blk ? n - at : blk;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BW_THREADS) void k_bwt_rec0(const uint8_t *__restrict__ in, uint64_t n, uint32_t blk_log2, mcom_mm128 *__restrict__ rec)
{
	const uint64_t i = (uint64_t)blockIdx.x * BW_THREADS + threadIdx.x;
	if (i >= n) return;
	const uint64_t b = i >> blk_log2;
	const uint64_t c0 = (uint64_t)in[i] + 1, c1 = i + 1 < n && ((i + 1) >> blk_log2) == b ? (uint64_t)in[i + 1] + 1 : 0;
	rec[i] = mcom_mm128{(b << 18) | (c0 << 9) | c1, i};
}

// f[j] = 1 where sorted record j opens a group; f[n] = 0, so that the exclusive scan ends with the number of groups
__global__ __launch_bounds__(BW_THREADS) void k_bwt_flags(const mcom_mm128 *__restrict__ rec, uint64_t n, uint32_t *__restrict__ f)
{
	const uint64_t j = (uint64_t)blockIdx.x * BW_THREADS + threadIdx.x;
	if (j > n) return;
	f[j] = j < n && (j == 0 || rec[j].x != rec[j - 1].x) ? 1u : 0u;
}

// e: the exclusive scan of the flags
__global__ __launch_bounds__(BW_THREADS) void k_bwt_rank(const mcom_mm128 *__restrict__ rec, const uint32_t *__restrict__ e, uint64_t n, uint32_t *__restrict__ rank)
{
	const uint64_t j = (uint64_t)blockIdx.x * BW_THREADS + threadIdx.x;
	if (j >= n) return;
	const mcom_mm128 r = rec[j];
	const uint32_t opens = j == 0 || r.x != rec[j - 1].x ? 1u : 0u;
	if (r.y < n) rank[r.y] = e[j] + opens;
}

__global__ __launch_bounds__(BW_THREADS) void k_bwt_rec(const uint32_t *__restrict__ rank, uint64_t n, uint32_t blk_log2, uint64_t h, uint32_t rank_bits,
                                                        mcom_mm128 *__restrict__ rec)
{
	const uint64_t i = (uint64_t)blockIdx.x * BW_THREADS + threadIdx.x;
	if (i >= n) return;
	const uint64_t r2 = i + h < n && ((i + h) >> blk_log2) == (i >> blk_log2) ? rank[i + h] : 0;
	rec[i] = mcom_mm128{((uint64_t)rank[i] << rank_bits) | r2, i};
}

// rank: final, every suffix its own: rank - block start = the row.  idx: anchors_full u32 per block.
__global__ __launch_bounds__(BW_THREADS) void k_bwt_emit(const uint8_t *__restrict__ in, const uint32_t *__restrict__ rank, uint64_t n, uint32_t blk_log2, uint32_t anc_log2,
                                                         uint64_t anchors_full, uint8_t *__restrict__ out, uint32_t *__restrict__ idx)
{
	const uint64_t i = (uint64_t)blockIdx.x * BW_THREADS + threadIdx.x;
	if (i >= n) return;
	const uint64_t b = i >> blk_log2, s = b << blk_log2, len = bw_block_len(n, b, blk_log2), p = i - s;
	const uint64_t r = (uint64_t)rank[i] - s, r0 = (uint64_t)rank[s] - s;
	if (r < 1 || r > len || r0 < 1 || r0 > len) return;                       // (cannot be: the ranks of a block are a permutation of its rows)
	if (p == 0) out[s] = in[s + len - 1];                                     // row 0, the empty suffix: the block's last byte
	else out[s + (r < r0 ? r : r - 1)] = in[i - 1];
	if ((p & (((uint64_t)1 << anc_log2) - 1)) == 0) idx[b * anchors_full + (p >> anc_log2)] = (uint32_t)r;
}

// ---- move-to-front ---------------------------------------------------------------------------------------------------------------------
// One lane per stretch of 2^s_log2 bytes (stretches never straddle a block: a block is a whole number of them).  PASS 1: from the identity
// list, the final list to perm[stretch] (and, coding, the number of distinct symbols to cnt[stretch]); PASS 2: from start[stretch], the
// ranks (bytes) to out.  DEC: src holds ranks.
template <int DEC, int PASS>
__global__ __launch_bounds__(64) void k_mtf_pass(const uint8_t *__restrict__ src, uint64_t n, uint32_t s_log2, uint64_t n_str, const uint8_t *__restrict__ start,
                                                 uint8_t *__restrict__ perm, uint32_t *__restrict__ cnt, uint8_t *__restrict__ out)
{
	__shared__ __attribute__((aligned(4))) uint8_t lists[64 * BW_LIST_PITCH];
	const uint64_t q = (uint64_t)blockIdx.x * 64 + threadIdx.x;
	if (q >= n_str) return;
	uint8_t *list = lists + (size_t)threadIdx.x * BW_LIST_PITCH;
	uint32_t *list32 = (uint32_t*)list;
	if (PASS == 1) { for (uint32_t k = 0; k < 64; ++k) list32[k] = (4 * k) | (4 * k + 1) << 8 | (4 * k + 2) << 16 | (4 * k + 3) << 24; }
	else { const uint32_t *st = (const uint32_t*)(start + q * 256); for (uint32_t k = 0; k < 64; ++k) list32[k] = st[k]; }
	const uint64_t at = q << s_log2;
	const uint32_t len = n - at < ((uint64_t)1 << s_log2) ? (uint32_t)(n - at) : 1u << s_log2;
	const uint8_t *s = src + at;
	uint8_t *o = out + at;
	uint32_t distinct = 0, acc = 0;
	for (uint32_t i = 0; i < len; ++i) {
		const uint32_t v = s[i];
		uint32_t k, c;
		if (DEC) { k = v; c = list[k]; }
		else { c = v; k = 0; while (k < 255 && list[k] != c) ++k; if (k >= distinct) ++distinct; }
		for (uint32_t j = k; j > 0; --j) list[j] = list[j - 1];
		list[0] = (uint8_t)c;
		if (PASS == 2) {
			acc |= (DEC ? c : k) << ((i & 3) * 8);
			if ((i & 3) == 3) { *(uint32_t*)(o + i - 3) = acc; acc = 0; }
		}
	}
	if (PASS == 2) for (uint32_t i = len & ~3u; i < len; ++i) o[i] = (uint8_t)(acc >> ((i & 3) * 8));
	if (PASS == 1) {
		uint32_t *p = (uint32_t*)(perm + q * 256);
		for (uint32_t k = 0; k < 64; ++k) p[k] = list32[k];
		if (!DEC) cnt[q] = distinct;
	}
}

// one wave per block: start[q] for its stretches q, in order
template <int DEC>
__global__ __launch_bounds__(64) void k_mtf_compose(const uint8_t *__restrict__ perm, const uint32_t *__restrict__ cnt, uint64_t n_str, uint32_t spb_log2,
                                                    uint8_t *__restrict__ start)
{
	__shared__ __attribute__((aligned(4))) uint8_t cur[256], nxt[256];
	__shared__ uint32_t mask[8];
	const uint32_t l = threadIdx.x;
	const uint64_t q0 = (uint64_t)blockIdx.x << spb_log2;
	const uint64_t q1 = q0 + ((uint64_t)1 << spb_log2) < n_str ? q0 + ((uint64_t)1 << spb_log2) : n_str;
	((uint32_t*)cur)[l] = (4 * l) | (4 * l + 1) << 8 | (4 * l + 2) << 16 | (4 * l + 3) << 24;
	__syncthreads();
	for (uint64_t q = q0; q < q1; ++q) {
		((uint32_t*)(start + q * 256))[l] = ((const uint32_t*)cur)[l];
		const uint32_t pw = ((const uint32_t*)(perm + q * 256))[l];
		if (DEC) {
#pragma unroll
			for (int k = 0; k < 4; ++k) nxt[4 * l + k] = cur[(pw >> (8 * k)) & 0xFFu];
		} else {
			const uint32_t m = cnt[q] > 256 ? 256u : cnt[q];
			if (l < 8) mask[l] = 0;
			__syncthreads();
#pragma unroll
			for (int k = 0; k < 4; ++k) if (4 * l + k < m) { const uint32_t c = (pw >> (8 * k)) & 0xFFu; atomicOr(&mask[c >> 5], 1u << (c & 31)); nxt[4 * l + k] = (uint8_t)c; }
			__syncthreads();
			const uint32_t cw = ((const uint32_t*)cur)[l];
			uint32_t keep = 0, mine = 0;
#pragma unroll
			for (int k = 0; k < 4; ++k) { const uint32_t c = (cw >> (8 * k)) & 0xFFu; if (!((mask[c >> 5] >> (c & 31)) & 1u)) { keep |= 1u << k; ++mine; } }
			uint32_t incl = mine;
#pragma unroll
			for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(incl, d); if (l >= (uint32_t)d) incl += t; }
			uint32_t pos = m + incl - mine;
#pragma unroll
			for (int k = 0; k < 4; ++k) if ((keep >> k) & 1u) { if (pos < 256) nxt[pos] = (uint8_t)(cw >> (8 * k)); ++pos; }
		}
		__syncthreads();
		((uint32_t*)cur)[l] = ((const uint32_t*)nxt)[l];
		__syncthreads();
	}
}

// ---- inverse ---------------------------------------------------------------------------------------------------------------------------
// hist[((block * 256 + byte) << spb_log2) + tile of the block]; one wave per tile of 2^s_log2 transformed bytes
__global__ __launch_bounds__(64) void k_bwt_tile_hist(const uint8_t *__restrict__ bwt, uint64_t n, uint32_t s_log2, uint32_t spb_log2, uint32_t *__restrict__ hist)
{
	__shared__ uint32_t h[256];
	const uint32_t l = threadIdx.x;
	for (int k = 0; k < 4; ++k) h[l + 64 * k] = 0;
	__syncthreads();
	const uint64_t q = blockIdx.x, at = q << s_log2;
	const uint32_t len = n - at < ((uint64_t)1 << s_log2) ? (uint32_t)(n - at) : 1u << s_log2;
	for (uint32_t i = l; i < len; i += 64) atomicAdd(&h[bwt[at + i]], 1u);
	__syncthreads();
	const uint64_t b = q >> spb_log2, t = q & (((uint64_t)1 << spb_log2) - 1);
	for (int k = 0; k < 4; ++k) hist[((b * 256 + l + 64 * k) << spb_log2) + t] = h[l + 64 * k];
}

// scanned: the exclusive scan of hist.  table[j] = byte << 24 | the row that follows transformed byte j of the block (1 .. its length)
__global__ __launch_bounds__(64) void k_bwt_lf(const uint8_t *__restrict__ bwt, uint64_t n, uint32_t s_log2, uint32_t spb_log2, const uint32_t *__restrict__ scanned,
                                               uint32_t *__restrict__ table)
{
	__shared__ uint32_t run[256];
	const uint32_t l = threadIdx.x;
	const uint64_t q = blockIdx.x, at = q << s_log2;
	const uint64_t b = q >> spb_log2, t = q & (((uint64_t)1 << spb_log2) - 1);
	const uint32_t base = scanned[(b * 256) << spb_log2];
	for (int k = 0; k < 4; ++k) run[l + 64 * k] = scanned[((b * 256 + l + 64 * k) << spb_log2) + t] - base;
	__syncthreads();
	const uint32_t len = n - at < ((uint64_t)1 << s_log2) ? (uint32_t)(n - at) : 1u << s_log2;
	for (uint32_t i0 = 0; i0 < len; i0 += 64) {
		const bool on = i0 + l < len;
		const uint32_t c = on ? bwt[at + i0 + l] : 0u;
		uint64_t same = __ballot(on);
#pragma unroll
		for (int bit = 0; bit < 8; ++bit) { const uint64_t v = __ballot((c >> bit) & 1u); same &= (c >> bit) & 1u ? v : ~v; }
		const uint32_t below = (uint32_t)__popcll(same & (((uint64_t)1 << l) - 1));
		uint32_t r = 0;
		if (on) r = run[c] + below;
		__syncthreads();
		if (on) {
			table[at + i0 + l] = c << 24 | ((1u + r) & 0xFFFFFFu);
			if (below == 0) run[c] = r + (uint32_t)__popcll(same);               // the first of the equal ones counts them all
		}
		__syncthreads();
	}
}

// One workgroup of 256 lanes per block, a lane per anchor stretch (at 1 MiB blocks and 4 KiB anchors: every lane one stretch; with more
// stretches a lane takes every 256th), so that the block's table is read through ONE L2 -- workgroups are dealt to the XCDs in turn.
// From the row of the suffix at the stretch's end (the index entry of the next stretch; row 0 at the block's end) backwards: the byte of
// the row is the text byte in front of the suffix, the table gives the row of the suffix that starts there.  Exactly the stretch's length
// in steps; it must arrive at the row the index gives for the stretch's start.
__global__ __launch_bounds__(BW_THREADS) void k_bwt_walk(const uint32_t *__restrict__ table, const uint32_t *__restrict__ idx, uint64_t n, uint32_t blk_log2, uint32_t anc_log2,
                                                         uint64_t anchors_full, uint8_t *__restrict__ out, uint32_t *__restrict__ flag)
{
	const uint64_t b = blockIdx.x, s = b << blk_log2;
	if (s >= n) return;
	const uint64_t len = bw_block_len(n, b, blk_log2), A = (uint64_t)1 << anc_log2, na = (len + A - 1) >> anc_log2;
	const uint32_t *ix = idx + b * anchors_full;
	const uint32_t r0 = ix[0];
	uint32_t bad = 0;
	for (uint64_t k = threadIdx.x; k < na && !bad; k += BW_THREADS) {
		const uint64_t lo = k * A, hi = lo + A < len ? lo + A : len;
		uint32_t r = hi == len ? 0u : ix[k + 1];
		for (uint64_t p = hi; p > lo; ) {
			if (r == r0 || r > len) { bad = BW_F_ROW; break; }                  // the row without a byte, or no row of this block: nothing is read
			const uint32_t w = table[s + (r < r0 ? r : r - 1)];
			out[s + --p] = (uint8_t)(w >> 24);
			r = w & 0xFFFFFFu;
		}
		if (!bad && r != ix[k]) bad = BW_F_CHAIN;
	}
	if (bad) atomicOr(flag, bad);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
namespace {
struct Blocks {                                             // pooled device blocks of one call, back to the pool once the stream has passed them
	mcom_ctx *ctx; std::vector<void*> v;
	explicit Blocks(mcom_ctx *c) : ctx(c) {}
	~Blocks() { for (void *p : v) mcom_dfree_later(ctx, p); }
	template <class T> hipError_t get(T **out, size_t bytes) { hipError_t e = mcom_dmalloc((void**)out, bytes ? bytes : 16); if (e == hipSuccess) v.push_back(*out); return e; }
};
unsigned grid_for(uint64_t items, unsigned threads) { return (unsigned)((items + threads - 1) / threads); }
uint32_t bit_length(uint64_t v) { uint32_t b = 0; while (v) { ++b; v >>= 1; } return b; }
uint32_t stretch_log2(uint32_t blk_log2) { return blk_log2 < MTF_LOG2 ? blk_log2 : MTF_LOG2; }

// device memory the forward transform of n bytes holds at its peak, and the inverse
// (+ 2 n + 8 MiB: the rANS coder's runs of 1.5 n + 8 per segment, its offsets and its 3.5 MB of histograms, held while a member is coded)
uint64_t forward_room(uint64_t n) { return 16 * n + mcom_sort_ws_bytes(n) + 8 * (n + 1) + 2 * n + ((uint64_t)9 << 20); }
uint64_t inverse_room(uint64_t n, uint32_t blk_log2) { return 4 * n + 2 * n + 3 * ((n >> stretch_log2(blk_log2)) + 1) * 1024 + ((uint64_t)9 << 20); }
int room_check(mcom_ctx *ctx, const char *who, uint64_t need)
{
	size_t fr = 0, tot = 0;
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	mcom_pool_trim();                                                           // free blocks of the library's own pool count as free
	MCOM_HIP(ctx, hipMemGetInfo(&fr, &tot));
	if (need > fr) return mcom_fail(ctx, MCOM_E_OVERFLOW, "%s: %llu bytes of device memory are needed, %zu are free (members are not split)", who, (unsigned long long)need, fr);
	return MCOM_OK;
}

// The stages, each in ONE place: the codec calls below and the hooks of include/mcom_test.h go through these.
// d_bwt: n bytes; d_idx: hd.n_anchors() u32 (4-byte aligned); n > 0
int forward_transform(mcom_ctx *ctx, const uint8_t *d_in, const Header &hd, uint8_t *d_bwt, uint32_t *d_idx, int *rounds_out)
{
	const uint64_t n = hd.raw_len;
	Blocks B(ctx);
	mcom_mm128 *rec = nullptr; void *ws = nullptr; uint32_t *rank = nullptr, *flags = nullptr;
	MCOM_HIP(ctx, B.get(&rec, n * sizeof(mcom_mm128)));
	MCOM_HIP(ctx, B.get(&ws, mcom_sort_ws_bytes(n)));
	MCOM_HIP(ctx, B.get(&rank, (n + 1) * 4));
	MCOM_HIP(ctx, B.get(&flags, (n + 1) * 4));
	const uint32_t rank_bits = bit_length(n);
	MCOM_LAUNCH(k_bwt_rec0, dim3(grid_for(n, BW_THREADS)), dim3(BW_THREADS), 0, ctx->stream, d_in, n, (uint32_t)hd.blk_log2, rec);
	MCOM_LAUNCH_CHECK(ctx);
	int bits = 18 + (int)bit_length(hd.n_blocks() - 1), rounds = 0;
	for (uint64_t h = 2; ; h *= 2) {
		int rc = mcom_sort_by_x(ctx, rec, n, bits, ws);
		if (rc) return rc;
		MCOM_LAUNCH(k_bwt_flags, dim3(grid_for(n + 1, BW_THREADS)), dim3(BW_THREADS), 0, ctx->stream, (const mcom_mm128*)rec, n, flags);
		MCOM_LAUNCH_CHECK(ctx);
		rc = mcom_scan_u32(ctx, flags, flags, n + 1, nullptr);
		if (rc) return rc;
		uint32_t groups = 0;
		MCOM_HIP(ctx, mcom_d2h_async(ctx, &groups, flags + n, 4));             // (the scan's last element: it waits in the pinned ring)
		MCOM_LAUNCH(k_bwt_rank, dim3(grid_for(n, BW_THREADS)), dim3(BW_THREADS), 0, ctx->stream, (const mcom_mm128*)rec, (const uint32_t*)flags, n, rank);
		MCOM_LAUNCH_CHECK(ctx);
		MCOM_HIP(ctx, mcom_stream_sync(ctx));
		++rounds;
		if (groups == n) break;
		if (rounds > (int)hd.blk_log2 + 1) return mcom_fail(ctx, MCOM_E_HIP, "bwt: %u groups of %llu suffixes after %d rounds", groups, (unsigned long long)n, rounds);
		MCOM_LAUNCH(k_bwt_rec, dim3(grid_for(n, BW_THREADS)), dim3(BW_THREADS), 0, ctx->stream, (const uint32_t*)rank, n, (uint32_t)hd.blk_log2, h, rank_bits, rec);
		MCOM_LAUNCH_CHECK(ctx);
		bits = 2 * (int)rank_bits;
	}
	if (rounds_out) *rounds_out = rounds;
	MCOM_LAUNCH(k_bwt_emit, dim3(grid_for(n, BW_THREADS)), dim3(BW_THREADS), 0, ctx->stream, d_in, (const uint32_t*)rank, n, (uint32_t)hd.blk_log2, (uint32_t)hd.anc_log2,
	            hd.anchors_full(), d_bwt, d_idx);
	MCOM_LAUNCH_CHECK(ctx);
	return MCOM_OK;
}

// src, dst: n bytes each, 4-byte aligned (the library's own buffers); dec: ranks -> bytes
int mtf_run(mcom_ctx *ctx, const uint8_t *src, uint64_t n, uint32_t blk_log2, uint8_t *dst, bool dec)
{
	const uint32_t s_log2 = stretch_log2(blk_log2), spb_log2 = blk_log2 - s_log2;
	const uint64_t n_str = (n + ((uint64_t)1 << s_log2) - 1) >> s_log2, n_blk = (n + ((uint64_t)1 << blk_log2) - 1) >> blk_log2;
	Blocks B(ctx);
	uint8_t *perm = nullptr, *start = nullptr; uint32_t *cnt = nullptr;
	MCOM_HIP(ctx, B.get(&perm, n_str * 256));
	MCOM_HIP(ctx, B.get(&start, n_str * 256));
	MCOM_HIP(ctx, B.get(&cnt, n_str * 4));
	const dim3 g(grid_for(n_str, 64)), t(64);
	if (dec) {
		MCOM_LAUNCH((k_mtf_pass<1, 1>), g, t, 0, ctx->stream, src, n, s_log2, n_str, (const uint8_t*)start, perm, cnt, dst);
		MCOM_LAUNCH(k_mtf_compose<1>, dim3((unsigned)n_blk), t, 0, ctx->stream, (const uint8_t*)perm, (const uint32_t*)cnt, n_str, spb_log2, start);
		MCOM_LAUNCH((k_mtf_pass<1, 2>), g, t, 0, ctx->stream, src, n, s_log2, n_str, (const uint8_t*)start, perm, cnt, dst);
	} else {
		MCOM_LAUNCH((k_mtf_pass<0, 1>), g, t, 0, ctx->stream, src, n, s_log2, n_str, (const uint8_t*)start, perm, cnt, dst);
		MCOM_LAUNCH(k_mtf_compose<0>, dim3((unsigned)n_blk), t, 0, ctx->stream, (const uint8_t*)perm, (const uint32_t*)cnt, n_str, spb_log2, start);
		MCOM_LAUNCH((k_mtf_pass<0, 2>), g, t, 0, ctx->stream, src, n, s_log2, n_str, (const uint8_t*)start, perm, cnt, dst);
	}
	MCOM_LAUNCH_CHECK(ctx);
	return MCOM_OK;
}

// d_bwt: n transformed bytes (4-byte aligned); d_idx: the checked index; d_out: n bytes at any address; *flag_out: what the walk raised
int inverse_transform(mcom_ctx *ctx, const uint8_t *d_bwt, const Header &hd, const uint32_t *d_idx, uint8_t *d_out, uint32_t *flag_out)
{
	const uint64_t n = hd.raw_len, n_blk = hd.n_blocks();
	const uint32_t s_log2 = stretch_log2(hd.blk_log2), spb_log2 = hd.blk_log2 - s_log2;
	const uint64_t n_str = (n + ((uint64_t)1 << s_log2) - 1) >> s_log2, n_hist = (n_blk * 256) << spb_log2;
	Blocks B(ctx);
	uint32_t *hist = nullptr, *table = nullptr, *d_flag = nullptr;
	MCOM_HIP(ctx, B.get(&hist, n_hist * 4));
	MCOM_HIP(ctx, B.get(&table, n * 4));
	MCOM_HIP(ctx, B.get(&d_flag, 16));
	MCOM_HIP(ctx, hipMemsetAsync(hist, 0, n_hist * 4, ctx->stream));
	MCOM_HIP(ctx, hipMemsetAsync(d_flag, 0, 4, ctx->stream));
	MCOM_LAUNCH(k_bwt_tile_hist, dim3((unsigned)n_str), dim3(64), 0, ctx->stream, d_bwt, n, s_log2, spb_log2, hist);
	MCOM_LAUNCH_CHECK(ctx);
	int rc = mcom_scan_u32(ctx, hist, hist, n_hist, nullptr);
	if (rc) return rc;
	MCOM_LAUNCH(k_bwt_lf, dim3((unsigned)n_str), dim3(64), 0, ctx->stream, d_bwt, n, s_log2, spb_log2, (const uint32_t*)hist, table);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_LAUNCH(k_bwt_walk, dim3((unsigned)n_blk), dim3(BW_THREADS), 0, ctx->stream, (const uint32_t*)table, d_idx, n, (uint32_t)hd.blk_log2, (uint32_t)hd.anc_log2,
	            hd.anchors_full(), d_out, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, mcom_d2h_async(ctx, flag_out, d_flag, 4));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}
}  // namespace

extern "C" uint64_t mcom_bwt_bound(uint64_t n) { return HEADER_BYTES + mcom_rans::HEADER_BYTES + n + 4 * ((n >> ANC_LOG2) + (n >> BLK_LOG2) + 2); }

extern "C" int mcom_bwt_encode(mcom_ctx *ctx, const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t cap, uint64_t *out_len)
{
	if (!ctx) return MCOM_E_ARG;
	if (!out_len || !d_out || (n && !d_in)) return mcom_fail(ctx, MCOM_E_ARG, "bwt_encode: null pointer");
	*out_len = 0;
	if (n > RAW_MAX) return mcom_fail(ctx, MCOM_E_ARG, "bwt_encode: %llu bytes (members below 4 GiB)", (unsigned long long)n);
	Blocks B(ctx);
	Header hd; hd.raw_len = n;
	// the plain coding of the bytes: the fallback, and its header holds the CRC-32 of the raw bytes
	uint8_t *d_plain = nullptr, *d_coded = nullptr, *d_bwt = nullptr, *d_ranks = nullptr; uint32_t *d_idx = nullptr;
	uint64_t plain_len = 0, coded_len = 0;
	MCOM_HIP(ctx, B.get(&d_plain, mcom_rans::HEADER_BYTES + n));
	int rc = mcom_rans_encode(ctx, d_in, n, d_plain, mcom_rans::HEADER_BYTES + n, &plain_len, 0);
	if (rc) return rc;
	uint8_t ph[mcom_rans::HEADER_BYTES];
	MCOM_HIP(ctx, hipMemcpyAsync(ph, d_plain, mcom_rans::HEADER_BYTES, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	hd.crc = get_u32(ph + 16);
	const uint64_t index_bytes = 4 * hd.n_anchors();
	if (n) {
		rc = room_check(ctx, "bwt_encode", forward_room(n) + 3 * n + index_bytes);
		if (rc) return rc;
		MCOM_HIP(ctx, B.get(&d_bwt, n));
		MCOM_HIP(ctx, B.get(&d_ranks, n));
		MCOM_HIP(ctx, B.get(&d_idx, index_bytes));
		MCOM_HIP(ctx, B.get(&d_coded, mcom_rans::HEADER_BYTES + n));
		rc = forward_transform(ctx, d_in, hd, d_bwt, d_idx, nullptr);
		if (rc) return rc;
		rc = mtf_run(ctx, d_bwt, n, hd.blk_log2, d_ranks, false);
		if (rc) return rc;
		rc = mcom_rans_encode(ctx, d_ranks, n, d_coded, mcom_rans::HEADER_BYTES + n, &coded_len, 0);
		if (rc) return rc;
	}
	const bool use_bwt = n && index_bytes + coded_len < plain_len;              // a tie goes to plain
	hd.kind = use_bwt ? KIND_BWT : KIND_PLAIN;
	hd.index_bytes = use_bwt ? index_bytes : 0;
	hd.member_bytes = use_bwt ? coded_len : plain_len;
	const uint64_t total = HEADER_BYTES + hd.index_bytes + hd.member_bytes;
	if (total > cap) return mcom_fail(ctx, MCOM_E_OVERFLOW, "bwt_encode: %llu bytes, room for %llu", (unsigned long long)total, (unsigned long long)cap);
	uint8_t head[HEADER_BYTES];
	write_header(head, hd);
	MCOM_HIP(ctx, hipMemcpyAsync(d_out, head, HEADER_BYTES, hipMemcpyHostToDevice, ctx->stream));
	if (use_bwt) MCOM_HIP(ctx, hipMemcpyAsync(d_out + HEADER_BYTES, d_idx, index_bytes, hipMemcpyDeviceToDevice, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(d_out + HEADER_BYTES + hd.index_bytes, use_bwt ? d_coded : d_plain, hd.member_bytes, hipMemcpyDeviceToDevice, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	*out_len = total;
	return MCOM_OK;
}

extern "C" int mcom_bwt_decode(mcom_ctx *ctx, const uint8_t *d_in, uint64_t in_len, uint8_t *d_out, uint64_t cap, uint64_t *out_len)
{
	if (!ctx) return MCOM_E_ARG;
	if (!out_len || (in_len && !d_in)) return mcom_fail(ctx, MCOM_E_ARG, "bwt_decode: null pointer");
	*out_len = 0;
	if (in_len < HEADER_BYTES + mcom_rans::HEADER_BYTES) return mcom_fail(ctx, MCOM_E_ARG, "bwt_decode: not a .bwt member (%llu bytes)", (unsigned long long)in_len);
	uint8_t hb[HEADER_BYTES], eh[mcom_rans::HEADER_BYTES];
	MCOM_HIP(ctx, hipMemcpyAsync(hb, d_in, HEADER_BYTES, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	Header hd;
	if (!read_header(hb, in_len, hd)) return mcom_fail(ctx, MCOM_E_ARG, "bwt_decode: the header does not describe this member");
	const uint8_t *d_index = d_in + HEADER_BYTES, *d_member = d_index + hd.index_bytes;
	std::vector<uint8_t> index(hd.index_bytes);
	MCOM_HIP(ctx, hipMemcpyAsync(eh, d_member, mcom_rans::HEADER_BYTES, hipMemcpyDeviceToHost, ctx->stream));
	if (hd.index_bytes) MCOM_HIP(ctx, hipMemcpyAsync(index.data(), d_index, hd.index_bytes, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	// (check_embedded reads the 32 header bytes only)
	if (!check_embedded(eh, hd)) return mcom_fail(ctx, MCOM_E_ARG, "bwt_decode: the embedded member's header does not fit the outer one");
	if (hd.kind == KIND_BWT && !check_index(index.data(), hd)) return mcom_fail(ctx, MCOM_E_ARG, "bwt_decode: an index row outside its block");
	*out_len = hd.raw_len;
	if (hd.raw_len > cap) return mcom_fail(ctx, MCOM_E_OVERFLOW, "bwt_decode: %llu bytes, room for %llu", (unsigned long long)hd.raw_len, (unsigned long long)cap);
	if (hd.raw_len && !d_out) return mcom_fail(ctx, MCOM_E_ARG, "bwt_decode: null pointer");
	uint64_t got = 0;
	if (hd.kind == KIND_PLAIN) {
		const int rc = mcom_rans_decode(ctx, d_member, hd.member_bytes, d_out, cap, &got);
		if (rc || got != hd.raw_len) { *out_len = 0; return rc ? rc : mcom_fail(ctx, MCOM_E_ARG, "bwt_decode: the embedded member's length"); }
		return MCOM_OK;                                                         // (its CRC is the header's: check_embedded)
	}
	const uint64_t n = hd.raw_len;
	int rc = room_check(ctx, "bwt_decode", inverse_room(n, hd.blk_log2) + hd.index_bytes);
	if (rc) { *out_len = 0; return rc; }
	Blocks B(ctx);
	uint8_t *d_ranks = nullptr, *d_bwt = nullptr; uint32_t *d_idx = nullptr;
	MCOM_HIP(ctx, B.get(&d_ranks, n));
	MCOM_HIP(ctx, B.get(&d_bwt, n));
	MCOM_HIP(ctx, B.get(&d_idx, hd.index_bytes));
	MCOM_HIP(ctx, hipMemcpyAsync(d_idx, d_index, hd.index_bytes, hipMemcpyDeviceToDevice, ctx->stream));      // (to an aligned place)
	rc = mcom_rans_decode(ctx, d_member, hd.member_bytes, d_ranks, n, &got);
	if (rc || got != n) { *out_len = 0; return rc ? rc : mcom_fail(ctx, MCOM_E_ARG, "bwt_decode: the embedded member's length"); }
	rc = mtf_run(ctx, d_ranks, n, hd.blk_log2, d_bwt, true);
	if (rc) { *out_len = 0; return rc; }
	uint32_t flag = 0;
	rc = inverse_transform(ctx, d_bwt, hd, d_idx, d_out, &flag);
	if (rc) { *out_len = 0; return rc; }
	if (flag) { *out_len = 0; return mcom_fail(ctx, MCOM_E_ARG, "bwt_decode: corrupt member (flag 0x%x)", flag); }
	uint32_t crc = 0;
	rc = mcom_device_crc32(ctx, d_out, n, &crc);
	if (rc) { *out_len = 0; return rc; }
	if (crc != hd.crc) { *out_len = 0; return mcom_fail(ctx, MCOM_E_ARG, "bwt_decode: CRC mismatch"); }
	return MCOM_OK;
}

// ---- test hooks (include/mcom_test.h) --------------------------------------------------------------------------------------------------
extern "C" int mcom_test_bwt_forward(mcom_ctx *ctx, const uint8_t *d_in, uint64_t n, uint8_t *d_bwt, uint32_t *d_idx, int *h_rounds)
{
	if (!ctx) return MCOM_E_ARG;
	if (!d_in || !n || !d_bwt || !d_idx || n > RAW_MAX) return mcom_fail(ctx, MCOM_E_ARG, "test_bwt_forward: null pointer or no bytes");
	Header hd; hd.raw_len = n;
	int rc = forward_transform(ctx, d_in, hd, d_bwt, d_idx, h_rounds);
	if (rc) return rc;
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}

extern "C" int mcom_test_bwt_mtf(mcom_ctx *ctx, const uint8_t *d_src, uint64_t n, uint8_t *d_dst, int decode)
{
	if (!ctx) return MCOM_E_ARG;
	if (!d_src || !n || !d_dst || n > RAW_MAX || (((uintptr_t)d_src | (uintptr_t)d_dst) & 3)) return mcom_fail(ctx, MCOM_E_ARG, "test_bwt_mtf: null or unaligned pointer, or no bytes");
	int rc = mtf_run(ctx, d_src, n, BLK_LOG2, d_dst, decode != 0);
	if (rc) return rc;
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}
