// minicom_amd/csrc/digest.hip -- the digest of a FASTQ file (`minicom -K`): the definition is digest_model.hpp's.
//
//   k_fastq_record_hashes  sixteen lanes per record, sixteen records per workgroup, from the line index of mcom_decode_line_index as
//                          k_fastq_lengths works: the record checks, then lane q takes bytes [16 q, 16 q + 16) of every line of the record
//                          from the unaligned text (two words, put together from aligned loads as vf_chunk does), mixes them, and the
//                          sixteen partial sums are added across the lane group.  hS, hQ, hN of record first_record + r, two words each.
//                          Untrusted text: a record that fails a check is flagged and gets no hash; nothing is read outside the piece.
//   k_digest_reduce        the ordered and the multiset sums of the hash arrays (of both files for a pair): 2048 records per workgroup,
//                          sixteen running sums per thread, added across the wave, then across the waves through LDS, then one 64-bit
//                          atomic add per sum and workgroup.  Addition mod 2^64: the result does not depend on the order.
#include "mcom_dev.hpp"
#include "digest_model.hpp"

namespace dg = mcom_digest_model;

#define DG_THREADS 256
#define DG_G 16                                             // lanes per record
#define DG_PER_THREAD 8                                     // records per thread of the reduction
#define DG_WAVES (DG_THREADS / 64)

// w = bytes [p, p + nb) of the text (nb <= 16, p + nb <= n_bytes; the rest zero) as two little-endian words.  An aligned word that lies
// inside the text is loaded whole, one that crosses its first or last byte is put together from the bytes inside.
__device__ __forceinline__ void dg_chunk(const uint8_t *text, uint64_t n_bytes, uint64_t p, uint32_t nb, uint64_t w[2])
{
	w[0] = w[1] = 0;
	if (!nb) return;
	const uintptr_t tb = (uintptr_t)text, te = tb + n_bytes, at = tb + p;
	const uint32_t sh = (uint32_t)(at & 3);
	const uintptr_t a = at - sh;
	const uint32_t nd = (sh + nb + 3) >> 2;                                    // aligned words covering the bytes: 1 .. 5
	uint32_t d[5], x[4];
#pragma unroll
	for (uint32_t i = 0; i < 5; ++i) {
		uint32_t v = 0;
		if (i < nd) {
			const uintptr_t q = a + 4 * (uintptr_t)i;
			if (q >= tb && q + 4 <= te) v = *(const uint32_t*)q;
			else for (uint32_t j = 0; j < 4; ++j) if (q + j >= tb && q + j < te) v |= (uint32_t)*(const uint8_t*)(q + j) << (8 * j);
		}
		d[i] = v;
	}
#pragma unroll
	for (uint32_t i = 0; i < 4; ++i) {
		uint32_t v = (uint32_t)((((uint64_t)d[i + 1] << 32) | d[i]) >> (8 * sh));
		const int rem = (int)nb - 4 * (int)i;
		if (rem <= 0) v = 0; else if (rem < 4) v &= (1u << (8 * rem)) - 1u;
		x[i] = v;
	}
	w[0] = x[0] | ((uint64_t)x[1] << 32);
	w[1] = x[2] | ((uint64_t)x[3] << 32);
}

__device__ __forceinline__ uint64_t dg_add16(uint64_t v)
{
#pragma unroll
	for (int o = DG_G / 2; o; o >>= 1) v += __shfl_xor((unsigned long long)v, o, DG_G);
	return v;
}

// H of the line [p, p + m) for both seeds, by the sixteen lanes of a record together (m <= 256: sixteen bytes a lane)
__device__ __forceinline__ void dg_line(const uint8_t *text, uint64_t n_bytes, uint64_t p, uint32_t m, uint32_t lane, uint64_t h[2])
{
	const uint32_t from = 16 * lane, nb = m > from ? (m - from < 16 ? m - from : 16) : 0;
	uint64_t w[2];
	dg_chunk(text, n_bytes, p + from, nb, w);
	const uint32_t j0 = 2 * lane;
#pragma unroll
	for (int s = 0; s < 2; ++s) {
		const uint64_t K = dg::seed(s);
		uint64_t t = 0;
		if (8 * j0 < m) t += dg::word_term(w[0], j0, K);
		if (8 * (j0 + 1) < m) t += dg::word_term(w[1], j0 + 1, K);
		h[s] = dg::line_hash(dg_add16(t), m);
	}
}

__global__ __launch_bounds__(DG_THREADS) void k_fastq_record_hashes(const uint8_t *__restrict__ text, uint64_t n_bytes, const uint64_t *__restrict__ start, uint64_t first_record,
                                                                    uint64_t n_records, uint32_t lpr, uint64_t *__restrict__ hS, uint64_t *__restrict__ hQ, uint64_t *__restrict__ hN,
                                                                    uint32_t *__restrict__ flag)
{
	const uint64_t r = ((uint64_t)blockIdx.x * DG_THREADS + threadIdx.x) / DG_G;
	const uint32_t lane = threadIdx.x % DG_G;
	if (r >= n_records) return;                                                // (all sixteen lanes of a record together, here and below)
	uint32_t bad = 0;
	uint64_t a = 0, b = 0, c = 0, d = 0, sl = 0;
	if (lpr == 4) {
		a = start[4 * r]; b = start[4 * r + 1]; c = start[4 * r + 2]; d = start[4 * r + 3];
		const uint64_t e = start[4 * r + 4];
		if (!(a < b && b < c && c < d && d < e && e <= n_bytes)) bad = MCOM_FASTQ_F_LENGTH;     // (cannot be: the index is made of this text)
		else {
			if (b - 1 - a < 1 || text[a] != '@') bad |= MCOM_FASTQ_F_NAME;
			if (d - 1 - c < 1 || text[c] != '+') bad |= MCOM_FASTQ_F_PLUS;
			sl = c - 1 - b;
			if (e - 1 - d != sl || sl < 1 || sl > dg::LINE_BYTES) bad |= MCOM_FASTQ_F_LENGTH;
			if (!bad && (b - 2 - a > dg::NAME_BYTES || d - 2 - c > dg::NAME_BYTES)) bad |= MCOM_FASTQ_F_LONG;
		}
	} else {
		b = start[r];
		const uint64_t e = start[r + 1];
		if (!(b < e && e <= n_bytes)) bad = MCOM_FASTQ_F_LENGTH;
		else { sl = e - 1 - b; if (sl < 1 || sl > dg::LINE_BYTES) bad = MCOM_FASTQ_F_LENGTH; }
	}
	if (bad) {
		if (lane == 0) { atomicOr(&flag[0], bad); atomicMin(&flag[1], (uint32_t)(first_record + r)); }
		return;
	}
	const uint64_t at = 2 * (first_record + r);
	uint64_t h[2];
	dg_line(text, n_bytes, b, (uint32_t)sl, lane, h);
	if (lane == 0) { hS[at] = h[0]; hS[at + 1] = h[1]; }
	if (lpr != 4) return;
	if (hQ) {
		dg_line(text, n_bytes, d, (uint32_t)sl, lane, h);
		if (lane == 0) { hQ[at] = h[0]; hQ[at + 1] = h[1]; }
	}
	if (hN) {
		uint64_t g[2];
		dg_line(text, n_bytes, a + 1, (uint32_t)(b - 2 - a), lane, h);
		dg_line(text, n_bytes, c + 1, (uint32_t)(d - 2 - c), lane, g);
		if (lane == 0) { hN[at] = dg::combine(h[0], g[0], dg::seed(0)); hN[at + 1] = dg::combine(h[1], g[1], dg::seed(1)); }
	}
}

extern "C" int mcom_fastq_record_hashes(mcom_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_line_start, uint64_t first_record, uint64_t n_records,
                                        int lines_per_record, uint64_t n_total, uint64_t *d_hS, uint64_t *d_hQ, uint64_t *d_hN, uint32_t *d_flag)
{
	if (!ctx) return MCOM_E_ARG;
	if (!d_flag || (n_records && (!d_text || !d_line_start || !d_hS))) return mcom_fail(ctx, MCOM_E_ARG, "fastq_record_hashes: null pointer");
	if ((lines_per_record != 4 && lines_per_record != 1) || n_total >= ((uint64_t)1 << 32) || first_record > n_total || n_records > n_total - first_record)
		return mcom_fail(ctx, MCOM_E_ARG, "fastq_record_hashes: %d lines a record (4 or 1), %llu records from %llu of %llu", lines_per_record, (unsigned long long)n_records,
		                 (unsigned long long)first_record, (unsigned long long)n_total);
	if (!n_records) return MCOM_OK;
	MCOM_LAUNCH(k_fastq_record_hashes, dim3((unsigned)((n_records * DG_G + DG_THREADS - 1) / DG_THREADS)), dim3(DG_THREADS), 0, ctx->stream, d_text, n_bytes, d_line_start, first_record,
	            n_records, (uint32_t)lines_per_record, d_hS, d_hQ, d_hN, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}

// ---- the reductions -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DG_THREADS) void k_digest_reduce(const uint64_t *__restrict__ hS1, const uint64_t *__restrict__ hQ1, const uint64_t *__restrict__ hN1,
                                                              const uint64_t *__restrict__ hS2, const uint64_t *__restrict__ hQ2, const uint64_t *__restrict__ hN2, uint64_t n,
                                                              unsigned long long *__restrict__ sums)
{
	__shared__ uint64_t part[DG_WAVES][dg::N_SUMS];
	uint64_t acc[dg::N_SUMS];
#pragma unroll
	for (int k = 0; k < dg::N_SUMS; ++k) acc[k] = 0;
	const uint64_t base = (uint64_t)blockIdx.x * (DG_THREADS * DG_PER_THREAD);
	for (int k = 0; k < DG_PER_THREAD; ++k) {
		const uint64_t i = base + (uint64_t)k * DG_THREADS + threadIdx.x;
		if (i >= n) break;
#pragma unroll
		for (int s = 0; s < 2; ++s) {
			const uint64_t K = dg::seed(s);
			const uint64_t s1 = hS1[2 * i + s];
			uint64_t rs = s1, rr = 0;
			acc[2 * dg::SEQ_ORDERED_1 + s] += dg::ordered_term(s1, i, K);
			if (hQ1) { const uint64_t q1 = hQ1[2 * i + s]; acc[2 * dg::QUAL_ORDERED_1 + s] += dg::ordered_term(q1, i, K); rr = dg::combine(s1, q1, K); }
			if (hN1) acc[2 * dg::NAME_ORDERED_1 + s] += dg::ordered_term(hN1[2 * i + s], i, K);
			if (hS2) {
				const uint64_t s2 = hS2[2 * i + s];
				acc[2 * dg::SEQ_ORDERED_2 + s] += dg::ordered_term(s2, i, K);
				rs = dg::combine(s1, s2, K);
				if (hQ2) { const uint64_t q2 = hQ2[2 * i + s]; acc[2 * dg::QUAL_ORDERED_2 + s] += dg::ordered_term(q2, i, K); rr = dg::combine(rr, dg::combine(s2, q2, K), K); }
				if (hN2) acc[2 * dg::NAME_ORDERED_2 + s] += dg::ordered_term(hN2[2 * i + s], i, K);
			}
			acc[2 * dg::SEQ_MULTISET + s] += dg::multiset_term(rs);
			if (hQ1) acc[2 * dg::REC_MULTISET + s] += dg::multiset_term(rr);
		}
	}
	const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
	for (int k = 0; k < dg::N_SUMS; ++k) {
		uint64_t v = acc[k];
#pragma unroll
		for (int o = 32; o; o >>= 1) v += __shfl_xor((unsigned long long)v, o, 64);
		if (lane == 0) part[wave][k] = v;
	}
	__syncthreads();
	if (threadIdx.x < dg::N_SUMS) {
		uint64_t v = 0;
#pragma unroll
		for (int q = 0; q < DG_WAVES; ++q) v += part[q][threadIdx.x];
		atomicAdd(&sums[threadIdx.x], (unsigned long long)v);
	}
}

extern "C" int mcom_digest_reduce(mcom_ctx *ctx, const uint64_t *d_hS1, const uint64_t *d_hQ1, const uint64_t *d_hN1, const uint64_t *d_hS2, const uint64_t *d_hQ2, const uint64_t *d_hN2,
                                  uint64_t n, uint64_t sums[16])
{
	if (!ctx) return MCOM_E_ARG;
	if (!sums || (n && !d_hS1)) return mcom_fail(ctx, MCOM_E_ARG, "digest_reduce: null pointer");
	for (int k = 0; k < dg::N_SUMS; ++k) sums[k] = 0;
	if (n >= ((uint64_t)1 << 32)) return mcom_fail(ctx, MCOM_E_ARG, "digest_reduce: %llu records (below 2^32)", (unsigned long long)n);
	if ((!d_hS2 && (d_hQ2 || d_hN2)) || (d_hS2 && ((d_hQ1 != nullptr) != (d_hQ2 != nullptr) || (d_hN1 != nullptr) != (d_hN2 != nullptr))))
		return mcom_fail(ctx, MCOM_E_ARG, "digest_reduce: the arrays of the second file must be those of the first");
	if (!n) return MCOM_OK;
	unsigned long long *d_sums = nullptr;
	MCOM_HIP(ctx, mcom_dmalloc((void**)&d_sums, dg::N_SUMS * 8));
	struct Back { mcom_ctx *c; void *p; ~Back() { mcom_dfree_later(c, p); } } back{ctx, d_sums};
	MCOM_HIP(ctx, hipMemsetAsync(d_sums, 0, dg::N_SUMS * 8, ctx->stream));
	const uint64_t per_block = (uint64_t)DG_THREADS * DG_PER_THREAD;
	MCOM_LAUNCH(k_digest_reduce, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(DG_THREADS), 0, ctx->stream, d_hS1, d_hQ1, d_hN1, d_hS2, d_hQ2, d_hN2, n, d_sums);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, hipMemcpyAsync(sums, d_sums, dg::N_SUMS * 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}
