// minicom_amd/csrc/qual_lossy.hip -- lossy quality values: a row-local transform of the n x L quality matrix in HBM, in place, between
// the gather of the rows and mcom_qual_encode (`minicom -b SPEC`; the transform itself: qual_lossy.hpp; specification and cross-check:
// host/mcom_qual_lossy.cpp).
//
//   k_qual_lut     the byte maps (ill8, thr, a general idempotent map).  The matrix is a list of segments -- ONE segment of n * L bytes
//                  when the rows lie back to back, otherwise one per row -- and a thread takes the aligned 16-byte pieces of a segment:
//                  one vector load, sixteen look-ups in the map in LDS, one vector store; the pieces that reach over a segment's ends
//                  go byte by byte, so nothing outside [0, L) of a row is read or written.  2 n L bytes moved.
//   k_qual_pblock  the P-block walk is sequential along a row, and one lane per row straight from HBM would read bytes a row apart.  So a
//                  workgroup stages a tile of QL_TILE_ROWS whole rows in LDS: sixteen lanes per row load the row's aligned 16-byte
//                  pieces (ragged ends by bytes) and write them as dwords; then ONE lane walks ONE row in LDS (pblock_row: 2 L steps,
//                  the same for every lane); then the tile goes back the way it came.  Row r of the tile starts at r * P + (its global
//                  address mod 4), P a multiple of 4 with P / 4 odd: a piece's dwords stay dword-aligned in LDS, and the 32 lanes of a
//                  bank group, one row each at about the same column, fall into 32 different banks (a column that straddles a dword
//                  edge for some of them: two-way at the worst).  P <= 260, so a tile takes at most 33 280 bytes: four workgroups
//                  (eight waves) per CU at L = 256, eight (sixteen waves) at L = 150 -- the walk is a chain of dependent LDS byte
//                  accesses, and resident waves are what hides it.  2 n L bytes moved.
// Both kernels count the report (bytes changed, sum |d|, sum d^2, max |d|) in the same pass: per lane, summed per wave by shuffles, per
// workgroup through LDS, then ONE atomic per counter and workgroup.
#include "mcom_dev.hpp"
#include "../../include/mcom_test.h"
#include "qual_lossy.hpp"
#include <string.h>

using namespace mcom_qlossy;

#define QL_THREADS 256
#define QL_TILE_ROWS 128                                    // rows of a k_qual_pblock tile = its threads
#define QL_L_MAX 256

static_assert(sizeof(Spec) == sizeof(mcom_qual_lossy_spec) && sizeof(Report) == sizeof(mcom_qual_lossy_report), "qual_lossy.hpp states the layouts of include/mcom.h");

namespace {

// the four counters of every lane -> one atomic each per workgroup.  All threads of the block call it.
template <int THREADS>
__device__ __forceinline__ void ql_report(unsigned long long changed, unsigned long long sum_abs, unsigned long long sum_sq, unsigned long long max_abs, unsigned long long *__restrict__ rep)
{
	__shared__ unsigned long long s_red[THREADS / 64][4];
	for (int o = 32; o > 0; o >>= 1) {
		changed += __shfl_down(changed, o); sum_abs += __shfl_down(sum_abs, o); sum_sq += __shfl_down(sum_sq, o);
		const unsigned long long m = __shfl_down(max_abs, o);
		max_abs = m > max_abs ? m : max_abs;
	}
	if ((threadIdx.x & 63) == 0) { unsigned long long *w = s_red[threadIdx.x >> 6]; w[0] = changed; w[1] = sum_abs; w[2] = sum_sq; w[3] = max_abs; }
	__syncthreads();
	if (threadIdx.x < 4) {
		unsigned long long v = 0;
		for (int w = 0; w < THREADS / 64; ++w) v = threadIdx.x == 3 ? (s_red[w][3] > v ? s_red[w][3] : v) : v + s_red[w][threadIdx.x];
		if (v) { if (threadIdx.x == 3) atomicMax(rep + 3, v); else atomicAdd(rep + threadIdx.x, v); }
	}
}

// segment g = the bytes [base + g * pitch, + seg_len); pieces = 16-byte pieces a segment can take part in, (seg_len + 30) / 16
__global__ __launch_bounds__(QL_THREADS) void k_qual_lut(uint8_t *__restrict__ base, uint64_t n_seg, uint64_t seg_len, uint64_t pitch, uint64_t pieces,
                                                         const uint8_t *__restrict__ lut, unsigned long long *__restrict__ rep)
{
	__shared__ uint8_t s_lut[256];
	s_lut[threadIdx.x] = lut[threadIdx.x];
	__syncthreads();
	unsigned long long changed = 0, sum_abs = 0, sum_sq = 0;
	uint32_t max_abs = 0;
	auto one = [&](uint32_t v) {
		const uint32_t o = s_lut[v], d = v > o ? v - o : o - v;
		changed += d != 0; sum_abs += d; sum_sq += d * d; max_abs = d > max_abs ? d : max_abs;
		return o;
	};
	const uint64_t total = n_seg * pieces;
	for (uint64_t c = (uint64_t)blockIdx.x * QL_THREADS + threadIdx.x; c < total; c += (uint64_t)gridDim.x * QL_THREADS) {
		const uint64_t g = c / pieces, k = c % pieces;
		uint8_t *seg = base + g * pitch;
		const uint64_t lead = (uint64_t)((uintptr_t)seg & 15);
		if (k * 16 >= lead + seg_len) continue;                             // (a piece behind the segment's last byte)
		if (k * 16 >= lead && k * 16 - lead + 16 <= seg_len) {
			uint4 *p = (uint4*)(seg + (k * 16 - lead));                     // 16-byte aligned: seg + k * 16 - lead
			uint4 v = *p;
			uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
			for (int q = 0; q < 4; ++q) w[q] = one(w[q] & 255u) | one((w[q] >> 8) & 255u) << 8 | one((w[q] >> 16) & 255u) << 16 | one(w[q] >> 24) << 24;
			v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
			*p = v;
		} else {
			const uint64_t b = k * 16 >= lead ? k * 16 - lead : 0, e = k * 16 + 16 - lead < seg_len ? k * 16 + 16 - lead : seg_len;
			for (uint64_t i = b; i < e; ++i) seg[i] = (uint8_t)one(seg[i]);
		}
	}
	ql_report<QL_THREADS>(changed, sum_abs, sum_sq, max_abs, rep);
}

// LDS pitch of a tile row: room for L bytes behind up to 3 bytes of lead, a multiple of 4 whose quarter is odd
__host__ __device__ inline uint32_t ql_lds_pitch(uint32_t L) { const uint32_t p = (L + 3 + 3) & ~3u; return (p >> 2) & 1 ? p : p + 4; }

// to_lds: row -> tile; otherwise tile -> row.  Sixteen lanes per row; the aligned 16-byte pieces of the ROW IN HBM as vectors there and as
// four dwords in LDS, the ragged ends by bytes.  Only [0, L) of a row is touched.
template <bool TO_LDS>
__device__ __forceinline__ void ql_move_tile(uint8_t *__restrict__ rows, uint64_t r0, uint32_t n_tile, uint32_t L, uint64_t pitch, uint8_t *s_tile, uint32_t P)
{
	const int lane = threadIdx.x & 15, iL = (int)L;
	for (uint32_t rr = threadIdx.x >> 4; rr < n_tile; rr += QL_TILE_ROWS >> 4) {
		uint8_t *g = rows + (r0 + rr) * pitch;
		const int lead = (int)((uintptr_t)g & 15);
		uint8_t *s = s_tile + rr * P + (lead & 3);
		const int n_pieces = (lead + iL + 15) >> 4;                         // at most 17
		for (int k = lane; k < n_pieces; k += 16) {
			const int at = k * 16 - lead;
			if (at >= 0 && at + 16 <= iL) {
				uint32_t *sw = (uint32_t*)(s + at);                             // dword-aligned: rr * P + (lead & 3) + k * 16 - lead
				if (TO_LDS) { const uint4 v = *(const uint4*)(g + at); sw[0] = v.x; sw[1] = v.y; sw[2] = v.z; sw[3] = v.w; }
				else { uint4 v; v.x = sw[0]; v.y = sw[1]; v.z = sw[2]; v.w = sw[3]; *(uint4*)(g + at) = v; }
			} else {
				const int b = at < 0 ? 0 : at, e = at + 16 < iL ? at + 16 : iL;
				for (int i = b; i < e; ++i) { if (TO_LDS) s[i] = g[i]; else g[i] = s[i]; }
			}
		}
	}
}

__global__ __launch_bounds__(QL_TILE_ROWS) void k_qual_pblock(uint8_t *__restrict__ rows, uint64_t n_rows, uint32_t L, uint64_t pitch, uint32_t P_block,
                                                              unsigned long long *__restrict__ rep)
{
	extern __shared__ uint32_t s_words[];
	uint8_t *s_tile = (uint8_t*)s_words;
	const uint32_t P = ql_lds_pitch(L);
	const uint64_t r0 = (uint64_t)blockIdx.x * QL_TILE_ROWS;
	const uint32_t n_tile = n_rows - r0 < QL_TILE_ROWS ? (uint32_t)(n_rows - r0) : (uint32_t)QL_TILE_ROWS;
	ql_move_tile<true>(rows, r0, n_tile, L, pitch, s_tile, P);
	__syncthreads();
	RowStat st;
	if (threadIdx.x < n_tile) {
		const uint32_t lead = (uint32_t)((uintptr_t)(rows + (r0 + threadIdx.x) * pitch) & 3);
		pblock_row(s_tile + threadIdx.x * P + lead, L, P_block, st);
	}
	__syncthreads();
	ql_move_tile<false>(rows, r0, n_tile, L, pitch, s_tile, P);
	ql_report<QL_TILE_ROWS>(st.changed, st.sum_abs, st.sum_sq, st.max_abs, rep);
}

}  // namespace

extern "C" uint32_t mcom_test_qual_pblock_tile_rows(void) { return QL_TILE_ROWS; }

extern "C" int mcom_qual_transform(mcom_ctx *ctx, uint8_t *d_rows, uint64_t n_rows, uint32_t L, uint64_t pitch, const mcom_qual_lossy_spec *spec, mcom_qual_lossy_report *h_report)
{
	if (!ctx) return MCOM_E_ARG;
	if (!spec || (n_rows && !d_rows)) return mcom_fail(ctx, MCOM_E_ARG, "qual_transform: null pointer");
	if (L < 1 || L > QL_L_MAX || pitch < L || n_rows >= ((uint64_t)1 << 32))
		return mcom_fail(ctx, MCOM_E_ARG, "qual_transform: L %u, pitch %llu, %llu rows (L 1 .. 256, pitch >= L, below 2^32 rows)", L, (unsigned long long)pitch, (unsigned long long)n_rows);
	Spec s;
	memcpy(&s, spec, sizeof s);
	uint8_t lut[256];
	if (!resolve(s, lut))
		return mcom_fail(ctx, MCOM_E_ARG, "qual_transform: not a spec (kind %u, %u %u %u): ill8, thr with LO < T <= HI <= 93, pblock 1 .. 47, or an idempotent byte map", s.kind, s.p[0], s.p[1], s.p[2]);
	Report r = {0, 0, 0, 0};
	if (n_rows) {
		uint8_t *d_work = nullptr;                                          // report (32 bytes) | map (256 bytes)
		MCOM_HIP(ctx, mcom_dmalloc(&d_work, 512));
		struct Back { mcom_ctx *c; void *p; ~Back() { mcom_dfree_later(c, p); } } back = {ctx, d_work};
		unsigned long long *d_rep = (unsigned long long*)d_work;
		MCOM_HIP(ctx, hipMemsetAsync(d_rep, 0, 32, ctx->stream));
		if (s.kind == K_PBLOCK) {
			const uint64_t tiles = (n_rows + QL_TILE_ROWS - 1) / QL_TILE_ROWS;  // below 2^25
			MCOM_LAUNCH(k_qual_pblock, dim3((unsigned)tiles), dim3(QL_TILE_ROWS), (size_t)QL_TILE_ROWS * ql_lds_pitch(L), ctx->stream, d_rows, n_rows, L, pitch, s.p[0], d_rep);
		} else {
			MCOM_HIP(ctx, hipMemcpyAsync(d_work + 64, lut, 256, hipMemcpyHostToDevice, ctx->stream));
			const bool flat = pitch == L;
			const uint64_t n_seg = flat ? 1 : n_rows, seg_len = flat ? n_rows * L : L, pieces = (seg_len + 30) / 16;
			uint64_t grid = (n_seg * pieces + QL_THREADS - 1) / QL_THREADS;
			const uint64_t gmax = (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 64) * 16;
			if (grid > gmax) grid = gmax;
			MCOM_LAUNCH(k_qual_lut, dim3((unsigned)grid), dim3(QL_THREADS), 0, ctx->stream, d_rows, n_seg, seg_len, pitch, pieces, (const uint8_t*)(d_work + 64), d_rep);
		}
		MCOM_LAUNCH_CHECK(ctx);
		MCOM_HIP(ctx, hipMemcpyAsync(&r, d_rep, 32, hipMemcpyDeviceToHost, ctx->stream));
		MCOM_HIP(ctx, mcom_stream_sync(ctx));
	}
	if (h_report) memcpy(h_report, &r, sizeof r);
	return MCOM_OK;
}
