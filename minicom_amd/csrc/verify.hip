// minicom_amd/csrc/verify.hip -- are two tables of reads in HBM the same reads?  
//
// A table is n rows of L characters, `pitch` bytes apart, at any address (the ingested reads: pitch L; the decoder's file image: pitch
// L + 1, rows aligned to nothing).  A record is a row, or -- paired form -- a row and the row of the same number of a second table, or
// in general the rows of the same number of up to four parts (mcom_verify_multiset_parts: a read with its quality line, a pair with both).
//   ordered    record i against record i: how many differ below min(n_a, n_b), and the first one                      (k_vf_ordered)
//   multiset   a 64-bit hash per record (k_vf_hash), {hash, record} sorted by hash on both sides (mcom_radix_sort_128x: stable, so the
//              records of a run of equal hashes stay in index order), then every sorted position finds its run on the other side by
//              bisection and takes the record of its own rank there as partner (k_vf_match); partners are compared byte for byte
//              (k_vf_compare).  A position without a partner is a record the other side does not give back (k_vf_count) -- unless a pair
//              of its run differed: such a run (equal hashes, unequal records: a collision) is marked, left out of the counts, listed
//              (k_vf_dirty_runs) and settled on the host as a multiset of its full records (vf_settle).  The verdict is exact.
// Sixteen lanes per record as in decode.hip: lane q takes bytes [16 q, 16 q + 16) of the row as the aligned 32-bit words that cover them,
// shifted into place -- never a byte outside the table, whatever the address.  Nothing here reads a file: sizes are the caller's.
#include "mcom_dev.hpp"
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#define VF_THREADS 256
#define VF_G 16                          // lanes per record
#define VF_RPB (VF_THREADS / VF_G)
#define VF_GOLD 0x9E3779B97F4A7C15ull

struct VfTable { const uint8_t *part[4]; int np; uint64_t pitch, n; };      // a record: row i of part[0 .. np)

// ---- sixteen bytes of a row -------------------------------------------------------------------------------------------------
// w = bytes [p, p + nb) (nb <= 16; the rest zero) as four little-endian words.  [tb, te) is the table: an aligned word that lies inside
// it is loaded whole, one that crosses its first or last byte is put together from the bytes inside.
__device__ __forceinline__ void vf_chunk(uintptr_t tb, uintptr_t te, uintptr_t p, int nb, uint32_t w[4])
{
	w[0] = w[1] = w[2] = w[3] = 0;
	if (nb <= 0) return;
	const uint32_t sh = (uint32_t)(p & 3);
	const uintptr_t a = p - sh;
	const int nd = (int)(sh + (uint32_t)nb + 3) >> 2;                      // aligned words covering the bytes: 1 .. 5
	uint32_t d[5];
#pragma unroll
	for (int i = 0; i < 5; ++i) {
		uint32_t v = 0;
		if (i < nd) {
			const uintptr_t q = a + 4 * (uintptr_t)i;
			if (q >= tb && q + 4 <= te) v = *(const uint32_t*)q;
			else for (int j = 0; j < 4; ++j) if (q + j >= tb && q + j < te) v |= (uint32_t)*(const uint8_t*)(q + j) << (8 * j);
		}
		d[i] = v;
	}
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		uint32_t v = (uint32_t)((((uint64_t)d[i + 1] << 32) | d[i]) >> (8 * sh));
		const int rem = nb - 4 * i;
		if (rem <= 0) v = 0; else if (rem < 4) v &= (1u << (8 * rem)) - 1u;
		w[i] = v;
	}
}

__device__ __forceinline__ uintptr_t vf_begin(const uint8_t *rows) { return (uintptr_t)rows; }
__device__ __forceinline__ uintptr_t vf_end(const uint8_t *rows, uint64_t pitch, uint64_t n, int L) { return (uintptr_t)rows + (n - 1) * pitch + (uint64_t)L; }

__device__ __forceinline__ uint64_t vf_mix(uint64_t z)
{
	z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
	z ^= z >> 27; z *= 0x94D049BB133111EBull;
	z ^= z >> 31;
	return z;
}

// hash of one row: word j = bytes [8 j, 8 j + 8) little-endian, zero-padded behind byte L - 1;
// h1 = mix(L + sum over j < ceil(L / 8) of mix(word j + (j + 1) GOLD)).  Called by all sixteen lanes of the group.
__device__ __forceinline__ uint64_t vf_row_hash(const uint8_t *rows, uint64_t pitch, uint64_t n, uint64_t i, int L, int lane, bool live)
{
	uint64_t s = 0;
	if (live) {
		uint32_t w[4];
		int nb = L - 16 * lane; if (nb > 16) nb = 16;
		vf_chunk(vf_begin(rows), vf_end(rows, pitch, n, L), (uintptr_t)rows + i * pitch + 16 * (uint64_t)lane, nb, w);
		const int j0 = 2 * lane;
		if (8 * j0 < L) s += vf_mix((w[0] | ((uint64_t)w[1] << 32)) + (uint64_t)(j0 + 1) * VF_GOLD);
		if (8 * (j0 + 1) < L) s += vf_mix((w[2] | ((uint64_t)w[3] << 32)) + (uint64_t)(j0 + 2) * VF_GOLD);
	}
#pragma unroll
	for (int o = VF_G / 2; o; o >>= 1) s += __shfl_xor((unsigned long long)s, o, VF_G);
	return vf_mix(s + (uint64_t)L);
}

__global__ __launch_bounds__(VF_THREADS) void k_vf_hash(const VfTable t, int L, uint64_t mask, mcom_mm128 *__restrict__ rec)
{
	const int g = threadIdx.x / VF_G, lane = threadIdx.x % VF_G;
	const uint64_t i = (uint64_t)blockIdx.x * VF_RPB + g;
	const bool live = i < t.n;
	uint64_t h = vf_row_hash(t.part[0], t.pitch, t.n, i, L, lane, live);
	for (int q = 1; q < t.np; ++q) h = vf_mix(h + VF_GOLD * vf_row_hash(t.part[q], t.pitch, t.n, i, L, lane, live));
	if (live && lane == 0) { mcom_mm128 r; r.x = h & mask; r.y = i; rec[i] = r; }
}

// does record ia of a differ from record ib of b?  This lane's sixteen bytes only; the caller joins the lanes
__device__ __forceinline__ bool vf_rows_differ(const uint8_t *ra, uint64_t pa, uint64_t na, uint64_t ia, const uint8_t *rb, uint64_t pb, uint64_t nb_rows, uint64_t ib,
                                               int L, int lane)
{
	int nb = L - 16 * lane; if (nb > 16) nb = 16;
	if (nb <= 0) return false;
	uint32_t u[4], v[4];
	vf_chunk(vf_begin(ra), vf_end(ra, pa, na, L), (uintptr_t)ra + ia * pa + 16 * (uint64_t)lane, nb, u);
	vf_chunk(vf_begin(rb), vf_end(rb, pb, nb_rows, L), (uintptr_t)rb + ib * pb + 16 * (uint64_t)lane, nb, v);
	return ((u[0] ^ v[0]) | (u[1] ^ v[1]) | (u[2] ^ v[2]) | (u[3] ^ v[3])) != 0;
}
__device__ __forceinline__ bool vf_records_differ(const VfTable &a, uint64_t ia, const VfTable &b, uint64_t ib, int L, int lane)
{
	bool d = false;
	for (int q = 0; q < a.np; ++q) d = d || vf_rows_differ(a.part[q], a.pitch, a.n, ia, b.part[q], b.pitch, b.n, ib, L, lane);
	return d;
}
// the four groups of a wave: bit q = some lane of group q says yes
__device__ __forceinline__ uint32_t vf_group_bits(bool yes)
{
	const unsigned long long m = __ballot(yes);
	uint32_t gb = 0;
#pragma unroll
	for (int q = 0; q < 64 / VF_G; ++q) if ((m >> (VF_G * q)) & 0xFFFFull) gb |= 1u << q;
	return gb;
}

// ---- ordered ------------------------------------------------------------------------------------------------------------------
// out[0] += records below n that differ, out[1] = min(out[1], the first of them): one pair of atomics per wave that found any
__global__ __launch_bounds__(VF_THREADS) void k_vf_ordered(const VfTable a, const VfTable b, int L, uint64_t n, unsigned long long *__restrict__ out)
{
	const int g = threadIdx.x / VF_G, lane = threadIdx.x % VF_G;
	const uint64_t i = (uint64_t)blockIdx.x * VF_RPB + g;
	const bool diff = i < n && vf_records_differ(a, i, b, i, L, lane);
	const uint32_t gb = vf_group_bits(diff);
	if (gb && (threadIdx.x & 63) == 0) {
		atomicAdd(out, (unsigned long long)__popc(gb));
		atomicMin(out + 1, (unsigned long long)(i + (uint64_t)(__ffs(gb) - 1)));       // (lane 0 of the wave holds the wave's first record)
	}
}

// ---- multiset -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t vf_lower(const mcom_mm128 *__restrict__ r, uint64_t n, uint64_t x)      // first i in [0, n] with r[i].x >= x
{
	uint64_t lo = 0, hi = n;
	while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (r[mid].x < x) lo = mid + 1; else hi = mid; }
	return lo;
}
__device__ __forceinline__ uint64_t vf_upper(const mcom_mm128 *__restrict__ r, uint64_t n, uint64_t x)      // first i in [0, n] with r[i].x > x
{
	uint64_t lo = 0, hi = n;
	while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (r[mid].x <= x) lo = mid + 1; else hi = mid; }
	return lo;
}
// first position of the run of x that holds position i: a few steps back (most runs are short), then bisection
__device__ __forceinline__ uint64_t vf_run_head(const mcom_mm128 *__restrict__ r, uint64_t i, uint64_t x)
{
	uint64_t k = i;
	for (int s = 0; s < 8 && k > 0 && r[k - 1].x == x; ++s) --k;
	if (k > 0 && r[k - 1].x == x) k = vf_lower(r, k, x);
	return k;
}

// partner[i] = the position on the other side of the record of the same hash and the same rank inside its run, or ~0
__global__ __launch_bounds__(VF_THREADS) void k_vf_match(const mcom_mm128 *__restrict__ me, uint64_t n_me, const mcom_mm128 *__restrict__ other, uint64_t n_other,
                                                         uint64_t *__restrict__ partner)
{
	const uint64_t i = (uint64_t)blockIdx.x * VF_THREADS + threadIdx.x;
	if (i >= n_me) return;
	const uint64_t x = me[i].x;
	const uint64_t j = vf_lower(other, n_other, x) + (i - vf_run_head(me, i, x));
	partner[i] = (j < n_other && other[j].x == x) ? j : ~0ull;
}

// every partnered position of side A against its partner, in full; a pair that differs marks its run at the run's first position
__global__ __launch_bounds__(VF_THREADS) void k_vf_compare(const VfTable a, const VfTable b, int L, const mcom_mm128 *__restrict__ ra, const mcom_mm128 *__restrict__ rb,
                                                           const uint64_t *__restrict__ partner, uint8_t *__restrict__ dirty, unsigned long long *__restrict__ n_bad)
{
	const int g = threadIdx.x / VF_G, lane = threadIdx.x % VF_G;
	const uint64_t i = (uint64_t)blockIdx.x * VF_RPB + g;
	bool diff = false;
	uint64_t j = ~0ull;
	if (i < a.n) j = partner[i];
	if (j != ~0ull) diff = vf_records_differ(a, ra[i].y, b, rb[j].y, L, lane);
	const uint32_t gb = vf_group_bits(diff);
	if (!gb) return;
	if (lane == 0 && ((gb >> ((threadIdx.x & 63) / VF_G)) & 1u)) dirty[vf_run_head(ra, i, ra[i].x)] = 1;
	if ((threadIdx.x & 63) == 0) atomicAdd(n_bad, (unsigned long long)__popc(gb));
}

// cand[i] (= partner[i], in place) becomes the record index of a position that has no partner and whose run is not marked, else ~0;
// *count += their number.  is_a: `me` is side A itself, else side B (whose run is marked where A's run of the same hash is).
__global__ __launch_bounds__(VF_THREADS) void k_vf_count(const mcom_mm128 *__restrict__ me, uint64_t n_me, uint64_t *__restrict__ cand, const mcom_mm128 *__restrict__ ra,
                                                         uint64_t n_a, const uint8_t *__restrict__ dirty, int is_a, unsigned long long *__restrict__ count)
{
	const uint64_t i = (uint64_t)blockIdx.x * VF_THREADS + threadIdx.x;
	bool lone = false;
	if (i < n_me) {
		lone = cand[i] == ~0ull;
		if (lone) {
			const uint64_t x = me[i].x;
			if (is_a) lone = !dirty[vf_run_head(me, i, x)];
			else { const uint64_t sa = vf_lower(ra, n_a, x); if (sa < n_a && ra[sa].x == x && dirty[sa]) lone = false; }
		}
		cand[i] = lone ? me[i].y : ~0ull;
	}
	const unsigned long long m = __ballot(lone);
	if (m && (threadIdx.x & 63) == 0) atomicAdd(count, (unsigned long long)__popcll(m));
}

// the marked runs: {first position and length on side A, first position and length on side B}.  list == nullptr: only counted
__global__ __launch_bounds__(VF_THREADS) void k_vf_dirty_runs(const mcom_mm128 *__restrict__ ra, uint64_t n_a, const mcom_mm128 *__restrict__ rb, uint64_t n_b,
                                                              const uint8_t *__restrict__ dirty, uint64_t *__restrict__ list, uint64_t cap, unsigned long long *__restrict__ count)
{
	const uint64_t i = (uint64_t)blockIdx.x * VF_THREADS + threadIdx.x;
	if (i >= n_a || !dirty[i]) return;
	const uint64_t slot = atomicAdd(count, 1ull);
	if (!list || slot >= cap) return;
	const uint64_t x = ra[i].x, sb = vf_lower(rb, n_b, x);
	list[4 * slot] = i; list[4 * slot + 1] = vf_upper(ra, n_a, x) - i;
	list[4 * slot + 2] = sb; list[4 * slot + 3] = vf_upper(rb, n_b, x) - sb;
}

// the records at sorted positions [first, first + len) back to back (a record: L bytes per part), for the host
__global__ __launch_bounds__(VF_THREADS) void k_vf_gather(const VfTable t, int L, const mcom_mm128 *__restrict__ rec, uint64_t first, uint64_t len, uint8_t *__restrict__ out)
{
	const uint64_t rl = (uint64_t)t.np * (uint64_t)L;
	const uint64_t at = (uint64_t)blockIdx.x * VF_THREADS + threadIdx.x;
	if (at >= len * rl) return;
	const uint64_t r = at / rl, c = at % rl, y = rec[first + r].y;
	if (y >= t.n) { out[at] = 0; return; }
	out[at] = t.part[c / (uint64_t)L][y * t.pitch + c % (uint64_t)L];
}

// *out = min(*out, the smallest cand[i] that is not ~0 and, with has_prev, above prev): one atomic per wave that holds one
__global__ __launch_bounds__(VF_THREADS) void k_vf_min_above(const uint64_t *__restrict__ cand, uint64_t n, uint64_t prev, int has_prev, unsigned long long *__restrict__ out)
{
	const uint64_t i = (uint64_t)blockIdx.x * VF_THREADS + threadIdx.x;
	unsigned long long v = ~0ull;
	if (i < n) { const uint64_t c = cand[i]; if (c != ~0ull && (!has_prev || c > prev)) v = c; }
#pragma unroll
	for (int o = 32; o; o >>= 1) { const unsigned long long t = __shfl_xor(v, o, 64); if (t < v) v = t; }
	if ((threadIdx.x & 63) == 0 && v != ~0ull) atomicMin(out, v);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
namespace {

struct VfBlocks {                                   // device blocks of one call, back to the pool when it returns
	std::vector<void*> p;
	~VfBlocks() { for (void *q : p) mcom_dfree(q); }
	template <class T> hipError_t get(T **out, uint64_t n) { void *q = nullptr; hipError_t e = mcom_dmalloc(&q, (size_t)((n ? n : 1) * sizeof(T))); if (e == hipSuccess) p.push_back(q); *out = (T*)q; return e; }
};

inline unsigned vf_blocks(uint64_t n, uint64_t per) { return (unsigned)((n + per - 1) / per); }
inline uint64_t vf_mask(int bits) { return bits >= 64 ? ~0ull : bits <= 0 ? 0ull : ((1ull << bits) - 1); }

int vf_check(mcom_ctx *ctx, const mcom_verify_table *a, const mcom_verify_table *b, int L, mcom_verify_report *rep, const char *who)
{
	if (!a || !b || !rep) return mcom_fail(ctx, MCOM_E_ARG, "%s: null pointer", who);
	if (L < 1 || L > 256) return mcom_fail(ctx, MCOM_E_ARG, "%s: L = %d not in 1..256", who, L);
	const mcom_verify_table *t[2] = {a, b};
	for (int s = 0; s < 2; ++s) {
		if (t[s]->n >= (1ull << 32)) return mcom_fail(ctx, MCOM_E_ARG, "%s: more than 2^32-1 records", who);
		if (t[s]->n && (!t[s]->d_rows || t[s]->pitch < (uint64_t)L)) return mcom_fail(ctx, MCOM_E_ARG, "%s: a table without rows, or a pitch below L", who);
	}
	if ((a->n && b->n) && ((a->d_mates != nullptr) != (b->d_mates != nullptr))) return mcom_fail(ctx, MCOM_E_ARG, "%s: one side is paired, the other is not", who);
	return MCOM_OK;
}

void vf_report_clear(mcom_verify_report *rep, uint64_t n_a, uint64_t n_b)
{
	*rep = mcom_verify_report();
	rep->n_a = n_a; rep->n_b = n_b; rep->first_diff = ~0ull;
	for (int q = 0; q < 8; ++q) rep->missing_ex[q] = rep->extra_ex[q] = ~0ull;
}

VfTable vf_table(const mcom_verify_table *t, bool paired) { VfTable v = {}; v.part[0] = t->d_rows; v.part[1] = paired ? t->d_mates : nullptr; v.np = paired ? 2 : 1; v.pitch = t->pitch; v.n = t->n; return v; }
VfTable vf_table(const mcom_verify_parts *t, int np) { VfTable v = {}; for (int q = 0; q < np; ++q) v.part[q] = t->d_part[q]; v.np = np; v.pitch = t->pitch; v.n = t->n; return v; }

// One marked run as a multiset of full records: the records of A that B does not give back and the converse, with multiplicity; within
// equal records the first ones (by record index) are the matched ones.
int vf_settle(mcom_ctx *ctx, const VfTable &A, const VfTable &B, int L, const mcom_mm128 *ra, const mcom_mm128 *rb, const uint64_t run[4],
              std::vector<uint64_t> &miss, std::vector<uint64_t> &extra)
{
	const uint64_t rl = (uint64_t)A.np * (uint64_t)L, la = run[1], lb = run[3], tot = la + lb;
	VfBlocks blk;
	uint8_t *d_rows = nullptr;
	MCOM_HIP(ctx, blk.get(&d_rows, tot * rl));
	MCOM_LAUNCH(k_vf_gather, dim3(vf_blocks(la * rl, VF_THREADS)), dim3(VF_THREADS), 0, ctx->stream, A, L, ra, run[0], la, d_rows);
	MCOM_LAUNCH_CHECK(ctx);
	if (lb) {
		MCOM_LAUNCH(k_vf_gather, dim3(vf_blocks(lb * rl, VF_THREADS)), dim3(VF_THREADS), 0, ctx->stream, B, L, rb, run[2], lb, d_rows + la * rl);
		MCOM_LAUNCH_CHECK(ctx);
	}
	std::vector<uint8_t> rows((size_t)(tot * rl));
	std::vector<mcom_mm128> rec((size_t)tot);
	MCOM_HIP(ctx, hipMemcpyAsync(rows.data(), d_rows, rows.size(), hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(rec.data(), ra + run[0], (size_t)la * sizeof(mcom_mm128), hipMemcpyDeviceToHost, ctx->stream));
	if (lb) MCOM_HIP(ctx, hipMemcpyAsync(rec.data() + la, rb + run[2], (size_t)lb * sizeof(mcom_mm128), hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	std::map<std::string, std::pair<std::vector<uint64_t>, std::vector<uint64_t>>> by;          // record -> its indices on side A, on side B (ascending: the sort is stable)
	for (uint64_t r = 0; r < tot; ++r) {
		auto &e = by[std::string((const char*)rows.data() + r * rl, (size_t)rl)];
		(r < la ? e.first : e.second).push_back(rec[(size_t)r].y);
	}
	for (const auto &kv : by) {
		const std::vector<uint64_t> &ia = kv.second.first, &ib = kv.second.second;
		for (size_t q = ib.size(); q < ia.size(); ++q) miss.push_back(ia[q]);
		for (size_t q = ia.size(); q < ib.size(); ++q) extra.push_back(ib[q]);
	}
	return MCOM_OK;
}

// the (up to) eight smallest record indices among cand[] and the host's own list, ascending
int vf_examples(mcom_ctx *ctx, const uint64_t *cand, uint64_t n, uint64_t n_dev, std::vector<uint64_t> &host, unsigned long long *d_slot, uint64_t ex[8], uint32_t *n_ex)
{
	std::vector<uint64_t> all(host);
	uint64_t prev = 0;
	for (int q = 0; q < 8 && (uint64_t)q < n_dev; ++q) {
		MCOM_HIP(ctx, hipMemsetAsync(d_slot, 0xFF, 8, ctx->stream));
		MCOM_LAUNCH(k_vf_min_above, dim3(vf_blocks(n, VF_THREADS)), dim3(VF_THREADS), 0, ctx->stream, cand, n, prev, q > 0, d_slot);
		MCOM_LAUNCH_CHECK(ctx);
		unsigned long long v = ~0ull;
		MCOM_HIP(ctx, hipMemcpyAsync(&v, d_slot, 8, hipMemcpyDeviceToHost, ctx->stream));
		MCOM_HIP(ctx, mcom_stream_sync(ctx));
		if (v == ~0ull) break;
		all.push_back(v); prev = v;
	}
	std::sort(all.begin(), all.end());
	*n_ex = (uint32_t)std::min<size_t>(8, all.size());
	for (uint32_t q = 0; q < *n_ex; ++q) ex[q] = all[q];
	return MCOM_OK;
}

} // namespace

extern "C" int mcom_set_verify_hash_bits(mcom_ctx *ctx, int bits)
{
	if (!ctx || bits > 64) return MCOM_E_ARG;
	ctx->verify_hash_bits = bits < 0 ? 64 : bits;
	return MCOM_OK;
}

extern "C" uint64_t mcom_verify_room(uint64_t n_a, uint64_t n_b)
{
	// records and partner words of both sides, the marks of side A, the sort's second buffer and histograms; the pool rounds a block up by a quarter
	const uint64_t own = (16 + 8) * (n_a + n_b) + n_a, big = n_a > n_b ? n_a : n_b;
	return own + own / 4 + (uint64_t)mcom_sort_ws_bytes((size_t)big) + ((uint64_t)64 << 20);
}

extern "C" int mcom_verify_ordered(mcom_ctx *ctx, const mcom_verify_table *a, const mcom_verify_table *b, int L, mcom_verify_report *rep)
{
	if (!ctx) return MCOM_E_ARG;
	int rc = vf_check(ctx, a, b, L, rep, "verify_ordered");
	if (rc) return rc;
	vf_report_clear(rep, a->n, b->n);
	const uint64_t n = a->n < b->n ? a->n : b->n;
	if (n) {
		VfBlocks blk;
		unsigned long long *d_out = nullptr, h_out[2] = {0, 0};
		MCOM_HIP(ctx, blk.get(&d_out, 2));
		MCOM_HIP(ctx, hipMemsetAsync(d_out, 0, 8, ctx->stream));
		MCOM_HIP(ctx, hipMemsetAsync(d_out + 1, 0xFF, 8, ctx->stream));
		const bool paired = a->d_mates && b->d_mates;
		MCOM_LAUNCH(k_vf_ordered, dim3(vf_blocks(n, VF_RPB)), dim3(VF_THREADS), 0, ctx->stream, vf_table(a, paired), vf_table(b, paired), L, n, d_out);
		MCOM_LAUNCH_CHECK(ctx);
		MCOM_HIP(ctx, hipMemcpyAsync(h_out, d_out, 16, hipMemcpyDeviceToHost, ctx->stream));
		MCOM_HIP(ctx, mcom_stream_sync(ctx));
		rep->differing = h_out[0]; rep->first_diff = h_out[1];
	}
	rep->identical = a->n == b->n && rep->differing == 0;
	return MCOM_OK;
}

// the multiset comparison over two checked sides of the same number of parts; rep is cleared
static int vf_multiset(mcom_ctx *ctx, const VfTable &A, const VfTable &B, int L, mcom_verify_report *rep)
{
	int rc;
	const uint64_t na = A.n, nb = B.n;
	if (na == 0 && nb == 0) { rep->identical = 1; return MCOM_OK; }
	const uint64_t mask = vf_mask(ctx->verify_hash_bits);
	VfBlocks blk;
	mcom_mm128 *ra = nullptr, *rb = nullptr;
	uint64_t *pa = nullptr, *pb = nullptr;
	uint8_t *dirty = nullptr;
	unsigned long long *cnt = nullptr;                 // [0] pairs that differ, [1] missing, [2] extra, [3] marked runs, [4] example slot
	MCOM_HIP(ctx, blk.get(&ra, na)); MCOM_HIP(ctx, blk.get(&rb, nb));
	MCOM_HIP(ctx, blk.get(&pa, na)); MCOM_HIP(ctx, blk.get(&pb, nb));
	MCOM_HIP(ctx, blk.get(&dirty, na)); MCOM_HIP(ctx, blk.get(&cnt, 8));
	MCOM_HIP(ctx, hipMemsetAsync(cnt, 0, 64, ctx->stream));
	if (na) {
		MCOM_HIP(ctx, hipMemsetAsync(dirty, 0, (size_t)na, ctx->stream));
		MCOM_LAUNCH(k_vf_hash, dim3(vf_blocks(na, VF_RPB)), dim3(VF_THREADS), 0, ctx->stream, A, L, mask, ra);
		MCOM_LAUNCH_CHECK(ctx);
		if ((rc = mcom_radix_sort_128x(ctx, ra, (size_t)na))) return rc;
	}
	if (nb) {
		MCOM_LAUNCH(k_vf_hash, dim3(vf_blocks(nb, VF_RPB)), dim3(VF_THREADS), 0, ctx->stream, B, L, mask, rb);
		MCOM_LAUNCH_CHECK(ctx);
		if ((rc = mcom_radix_sort_128x(ctx, rb, (size_t)nb))) return rc;
	}
	if (na) {
		MCOM_LAUNCH(k_vf_match, dim3(vf_blocks(na, VF_THREADS)), dim3(VF_THREADS), 0, ctx->stream, (const mcom_mm128*)ra, na, (const mcom_mm128*)rb, nb, pa);
		MCOM_LAUNCH_CHECK(ctx);
	}
	if (nb) {
		MCOM_LAUNCH(k_vf_match, dim3(vf_blocks(nb, VF_THREADS)), dim3(VF_THREADS), 0, ctx->stream, (const mcom_mm128*)rb, nb, (const mcom_mm128*)ra, na, pb);
		MCOM_LAUNCH_CHECK(ctx);
	}
	if (na && nb) {
		MCOM_LAUNCH(k_vf_compare, dim3(vf_blocks(na, VF_RPB)), dim3(VF_THREADS), 0, ctx->stream, A, B, L, (const mcom_mm128*)ra, (const mcom_mm128*)rb, (const uint64_t*)pa, dirty, cnt);
		MCOM_LAUNCH_CHECK(ctx);
	}
	if (na) {
		MCOM_LAUNCH(k_vf_count, dim3(vf_blocks(na, VF_THREADS)), dim3(VF_THREADS), 0, ctx->stream, (const mcom_mm128*)ra, na, pa, (const mcom_mm128*)ra, na, (const uint8_t*)dirty, 1, cnt + 1);
		MCOM_LAUNCH_CHECK(ctx);
	}
	if (nb) {
		MCOM_LAUNCH(k_vf_count, dim3(vf_blocks(nb, VF_THREADS)), dim3(VF_THREADS), 0, ctx->stream, (const mcom_mm128*)rb, nb, pb, (const mcom_mm128*)ra, na, (const uint8_t*)dirty, 0, cnt + 2);
		MCOM_LAUNCH_CHECK(ctx);
	}
	unsigned long long h[4] = {0, 0, 0, 0};
	MCOM_HIP(ctx, hipMemcpyAsync(h, cnt, 24, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	const uint64_t dev_missing = h[1], dev_extra = h[2];
	std::vector<uint64_t> miss, extra;
	if (h[0]) {
		// equal hashes, unequal records: list the marked runs (first counted, then written) and settle each in full on the host
		MCOM_LAUNCH(k_vf_dirty_runs, dim3(vf_blocks(na, VF_THREADS)), dim3(VF_THREADS), 0, ctx->stream, (const mcom_mm128*)ra, na, (const mcom_mm128*)rb, nb, (const uint8_t*)dirty,
		            (uint64_t*)nullptr, (uint64_t)0, cnt + 3);
		MCOM_LAUNCH_CHECK(ctx);
		MCOM_HIP(ctx, hipMemcpyAsync(h + 3, cnt + 3, 8, hipMemcpyDeviceToHost, ctx->stream));
		MCOM_HIP(ctx, mcom_stream_sync(ctx));
		const uint64_t n_runs = h[3];
		uint64_t *d_list = nullptr;
		MCOM_HIP(ctx, blk.get(&d_list, 4 * n_runs));
		MCOM_HIP(ctx, hipMemsetAsync(cnt + 3, 0, 8, ctx->stream));
		MCOM_LAUNCH(k_vf_dirty_runs, dim3(vf_blocks(na, VF_THREADS)), dim3(VF_THREADS), 0, ctx->stream, (const mcom_mm128*)ra, na, (const mcom_mm128*)rb, nb, (const uint8_t*)dirty,
		            d_list, n_runs, cnt + 3);
		MCOM_LAUNCH_CHECK(ctx);
		std::vector<uint64_t> list((size_t)(4 * n_runs));
		MCOM_HIP(ctx, hipMemcpyAsync(list.data(), d_list, list.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
		MCOM_HIP(ctx, mcom_stream_sync(ctx));
		std::vector<uint64_t> order((size_t)n_runs);
		for (uint64_t q = 0; q < n_runs; ++q) order[(size_t)q] = q;
		std::sort(order.begin(), order.end(), [&](uint64_t p, uint64_t q) { return list[4 * p] < list[4 * q]; });   // (the kernel lists them in any order)
		for (uint64_t q : order) if ((rc = vf_settle(ctx, A, B, L, ra, rb, &list[4 * q], miss, extra))) return rc;
		rep->exact_runs = n_runs;
	}
	rep->missing = dev_missing + miss.size();
	rep->extra = dev_extra + extra.size();
	if (rep->missing && (rc = vf_examples(ctx, pa, na, dev_missing, miss, cnt + 4, rep->missing_ex, &rep->n_missing_ex))) return rc;
	if (rep->extra && (rc = vf_examples(ctx, pb, nb, dev_extra, extra, cnt + 4, rep->extra_ex, &rep->n_extra_ex))) return rc;
	rep->identical = rep->missing == 0 && rep->extra == 0;
	return MCOM_OK;
}

extern "C" int mcom_verify_multiset(mcom_ctx *ctx, const mcom_verify_table *a, const mcom_verify_table *b, int L, mcom_verify_report *rep)
{
	if (!ctx) return MCOM_E_ARG;
	int rc = vf_check(ctx, a, b, L, rep, "verify_multiset");
	if (rc) return rc;
	vf_report_clear(rep, a->n, b->n);
	const bool paired = (a->n ? a->d_mates : b->d_mates) != nullptr;
	return vf_multiset(ctx, vf_table(a, paired), vf_table(b, paired), L, rep);
}

extern "C" int mcom_verify_multiset_parts(mcom_ctx *ctx, const mcom_verify_parts *a, const mcom_verify_parts *b, int L, mcom_verify_report *rep)
{
	if (!ctx) return MCOM_E_ARG;
	const char *who = "verify_multiset_parts";
	if (!a || !b || !rep) return mcom_fail(ctx, MCOM_E_ARG, "%s: null pointer", who);
	if (L < 1 || L > 256) return mcom_fail(ctx, MCOM_E_ARG, "%s: L = %d not in 1..256", who, L);
	if (a->n_parts < 1 || a->n_parts > 4 || b->n_parts != a->n_parts) return mcom_fail(ctx, MCOM_E_ARG, "%s: %d and %d parts (1 .. 4, the same on both sides)", who, a->n_parts, b->n_parts);
	const mcom_verify_parts *t[2] = {a, b};
	for (int s = 0; s < 2; ++s) {
		if (t[s]->n >= (1ull << 32)) return mcom_fail(ctx, MCOM_E_ARG, "%s: more than 2^32-1 records", who);
		if (t[s]->n && t[s]->pitch < (uint64_t)L) return mcom_fail(ctx, MCOM_E_ARG, "%s: a pitch below L", who);
		for (int q = 0; q < t[s]->n_parts; ++q) if (t[s]->n && !t[s]->d_part[q]) return mcom_fail(ctx, MCOM_E_ARG, "%s: part %d without rows", who, q);
	}
	vf_report_clear(rep, a->n, b->n);
	return vf_multiset(ctx, vf_table(a, a->n_parts), vf_table(b, a->n_parts), L, rep);
}
