// minicom_amd/csrc/qual_agree.hip -- consensus-guided lossy quality values (`minicom -a Q[:C]`): every quality
// value whose bit of the agreement mask is set becomes 33 + Q, every other value stays as it is.  The mask (csrc/decode.hip,
// mcom_agree_mask) has a row of (L + 7) / 8 bytes per decoder row, column i in bit i & 7 of byte i >> 3; quality row r of the call
// belongs to mask row first_mask_row + r.
//
//   k_qual_agree   a thread takes one aligned 16-byte piece of one row: one vector load, the piece's sixteen mask bits from at most
//                  three mask bytes, one vector store; the pieces that reach over a row's ends go byte by byte, so nothing outside
//                  [0, L) of a row is read or written.  2 n L bytes of quality values and n (L + 7) / 8 mask bytes moved.
// The report (bytes changed, sum |d|, sum d^2, max |d|, mask bits set) is counted in the same pass as in qual_lossy.hip: per lane, summed
// per wave by shuffles, per workgroup through LDS, then one atomic per counter and workgroup.
#include "mcom_dev.hpp"
#include <string.h>

#define QA_THREADS 256
#define QA_L_MAX 256

namespace {

// the five counters of every lane -> one atomic each per workgroup.  All threads of the block call it.
__device__ __forceinline__ void qa_report(unsigned long long changed, unsigned long long sum_abs, unsigned long long sum_sq, unsigned long long max_abs, unsigned long long bits,
                                          unsigned long long *__restrict__ rep)
{
	__shared__ unsigned long long s_red[QA_THREADS / 64][5];
	for (int o = 32; o > 0; o >>= 1) {
		changed += __shfl_down(changed, o); sum_abs += __shfl_down(sum_abs, o); sum_sq += __shfl_down(sum_sq, o); bits += __shfl_down(bits, o);
		const unsigned long long m = __shfl_down(max_abs, o);
		max_abs = m > max_abs ? m : max_abs;
	}
	if ((threadIdx.x & 63) == 0) { unsigned long long *w = s_red[threadIdx.x >> 6]; w[0] = changed; w[1] = sum_abs; w[2] = sum_sq; w[3] = max_abs; w[4] = bits; }
	__syncthreads();
	if (threadIdx.x < 5) {
		unsigned long long v = 0;
		for (int w = 0; w < QA_THREADS / 64; ++w) v = threadIdx.x == 3 ? (s_red[w][3] > v ? s_red[w][3] : v) : v + s_red[w][threadIdx.x];
		if (v) { if (threadIdx.x == 3) atomicMax(rep + 3, v); else atomicAdd(rep + threadIdx.x, v); }
	}
}

// pieces = 16-byte pieces a row can take part in, (L + 30) / 16
__global__ __launch_bounds__(QA_THREADS) void k_qual_agree(uint8_t *__restrict__ rows, uint64_t n_rows, uint32_t L, uint64_t pitch, uint64_t pieces,
                                                           const uint8_t *__restrict__ mask, uint64_t mask_pitch, uint64_t first_mask_row, uint32_t to,
                                                           unsigned long long *__restrict__ rep)
{
	unsigned long long changed = 0, sum_abs = 0, sum_sq = 0, bits = 0;
	uint32_t max_abs = 0;
	auto one = [&](uint32_t v, uint32_t masked) {
		if (!masked) return v;
		const uint32_t d = v > to ? v - to : to - v;
		++bits; changed += d != 0; sum_abs += d; sum_sq += d * d; max_abs = d > max_abs ? d : max_abs;
		return to;
	};
	const uint32_t mask_bytes = (L + 7) >> 3;
	const uint64_t total = n_rows * pieces;
	for (uint64_t c = (uint64_t)blockIdx.x * QA_THREADS + threadIdx.x; c < total; c += (uint64_t)gridDim.x * QA_THREADS) {
		const uint64_t g = c / pieces, k = c % pieces;
		uint8_t *row = rows + g * pitch;
		const uint8_t *mrow = mask + (first_mask_row + g) * mask_pitch;
		const uint64_t lead = (uint64_t)((uintptr_t)row & 15);
		if (k * 16 >= lead + L) continue;                                   // (a piece behind the row's last byte)
		if (k * 16 >= lead && k * 16 - lead + 16 <= L) {
			const uint32_t at = (uint32_t)(k * 16 - lead), b0 = at >> 3;    // columns at .. at + 15: bits of mask bytes b0 .. b0 + 2
			uint32_t mw = mrow[b0];
			if (b0 + 1 < mask_bytes) mw |= (uint32_t)mrow[b0 + 1] << 8;
			if (b0 + 2 < mask_bytes) mw |= (uint32_t)mrow[b0 + 2] << 16;
			mw = (mw >> (at & 7)) & 0xFFFFu;
			if (!mw) continue;
			uint4 *p = (uint4*)(row + at);                                  // 16-byte aligned: row + k * 16 - lead
			uint4 v = *p;
			uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
			for (int q = 0; q < 4; ++q) {
				const uint32_t m4 = mw >> (4 * q);
				w[q] = one(w[q] & 255u, m4 & 1u) | one((w[q] >> 8) & 255u, m4 & 2u) << 8 | one((w[q] >> 16) & 255u, m4 & 4u) << 16 | one(w[q] >> 24, m4 & 8u) << 24;
			}
			v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
			*p = v;
		} else {
			const uint64_t b = k * 16 >= lead ? k * 16 - lead : 0, e = k * 16 + 16 - lead < L ? k * 16 + 16 - lead : L;
			for (uint64_t i = b; i < e; ++i) if ((mrow[i >> 3] >> (i & 7)) & 1u) row[i] = (uint8_t)one(row[i], 1u);
		}
	}
	qa_report(changed, sum_abs, sum_sq, max_abs, bits, rep);
}

}  // namespace

extern "C" int mcom_qual_agree(mcom_ctx *ctx, uint8_t *d_rows, uint64_t n_rows, uint32_t L, uint64_t pitch, const uint8_t *d_mask, uint64_t mask_pitch,
                               uint64_t first_mask_row, uint32_t Q, mcom_qual_agree_report *h_report)
{
	if (!ctx) return MCOM_E_ARG;
	if (n_rows && (!d_rows || !d_mask)) return mcom_fail(ctx, MCOM_E_ARG, "qual_agree: null pointer");
	if (Q > 93 || L < 1 || L > QA_L_MAX || pitch < L || mask_pitch < (uint64_t)((L + 7) / 8) || n_rows >= ((uint64_t)1 << 32))
		return mcom_fail(ctx, MCOM_E_ARG, "qual_agree: Q %u, L %u, pitch %llu, mask pitch %llu, %llu rows (Q 0 .. 93, L 1 .. 256, pitch >= L, mask pitch >= (L + 7) / 8, below 2^32 rows)", Q, L,
		                 (unsigned long long)pitch, (unsigned long long)mask_pitch, (unsigned long long)n_rows);
	mcom_qual_agree_report r;
	memset(&r, 0, sizeof r);
	if (n_rows) {
		unsigned long long *d_rep = nullptr;                                // the five counters
		MCOM_HIP(ctx, mcom_dmalloc(&d_rep, 64));
		struct Back { mcom_ctx *c; void *p; ~Back() { mcom_dfree_later(c, p); } } back = {ctx, d_rep};
		MCOM_HIP(ctx, hipMemsetAsync(d_rep, 0, 64, ctx->stream));
		const uint64_t pieces = ((uint64_t)L + 30) / 16;
		uint64_t grid = (n_rows * pieces + QA_THREADS - 1) / QA_THREADS;
		const uint64_t gmax = (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 64) * 16;
		if (grid > gmax) grid = gmax;
		MCOM_LAUNCH(k_qual_agree, dim3((unsigned)grid), dim3(QA_THREADS), 0, ctx->stream, d_rows, n_rows, L, pitch, pieces, d_mask, mask_pitch, first_mask_row, 33u + Q, d_rep);
		MCOM_LAUNCH_CHECK(ctx);
		MCOM_HIP(ctx, hipMemcpyAsync(&r, d_rep, sizeof r, hipMemcpyDeviceToHost, ctx->stream));
		MCOM_HIP(ctx, mcom_stream_sync(ctx));
	}
	if (h_report) memcpy(h_report, &r, sizeof r);
	return MCOM_OK;
}
